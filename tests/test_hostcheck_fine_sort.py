"""The fused fine level of the MSM's sort (k_fine_sort, myzkp_amd/csrc/mzk_msm.hip): the plan the kernels share with the host
(mzk_msm_plan.h: which workgroup takes which bin or slice, the whole-bin capacity, the slice bounds of over-full bins, the grid size)
run by tests/hostcheck/fine_sort_shim.cpp, a stand-alone program built with -fsanitize=address,undefined, over arrays of exactly the
kernels' sizes.  Bin lengths: all empty, all equal, one bin at capacity - 1, capacity and capacity + 1, one bin holding everything,
whole, sliced and empty bins side by side, and lengths whose slices are exactly the extra workgroups the grid has.  Every record must be
taken exactly once and inside its bin, no workgroup past the grid may be needed, the bucket offsets must be monotone and end at the
total, and every bucket's run must hold its own records.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fine_sort") / "fine_sort_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "fine_sort_shim.cpp")])
    return exe


def test_every_record_is_placed_once_inside_its_bin_and_no_index_leaves_the_arrays(shim):
    r = subprocess.run([shim], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 60 and int(words[2]) >= 15000, r.stdout


def test_the_plan_takes_the_fused_form_where_a_bin_fits_a_workgroup(shim):
    """17-bit tables at 2^20 points, the flagship commit: 512 bins of 128 buckets, one workgroup each plus the slices over-full bins
    can need; the form is chosen from the first two-level size on, at every width whose counters fit (13 .. 20 bits on a short SRS)"""
    def plan(c, stride):
        out = subprocess.run([shim, "plan", str(c), str(stride)], capture_output=True, text=True, check=True).stdout.split()
        return dict(zip(out[0::2], (int(v) for v in out[1::2])))
    p = plan(17, 1 << 20)
    assert (p["fused_at_stride"], p["F"], p["bins"], p["cap"]) == (1, 128, 512, 33 * 1024)
    for c in range(13, 21):
        p = plan(c, 1 << 15)
        assert p["fused"] == 1 and p["fused_plus3"] == 1 and p["fine_wgs"] >= p["bins"], (c, p)
    assert plan(21, 1 << 15)["fused"] == 0        # 4096 buckets per bin: the counters and the window no longer fit twice on a CU
