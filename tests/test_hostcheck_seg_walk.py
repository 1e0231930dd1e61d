"""The index logic of k_seg_accumulate's pipelined loop (seg_span / seg_first_bucket / seg_walk in myzkp_amd/csrc/mzk_msm_plan.h: which
entry is current, which loads are in flight, where a lane stops) run on the host by tests/hostcheck/seg_walk_shim.cpp, a stand-alone
program built with -fsanitize=address,undefined: segment lengths 1, 2, 3 and 8; totals 0, 1, seg - 1, seg, seg + 1 and k seg + 1; a
bucket boundary on a segment's first and last entry; runs of empty buckets; sentinel tails.  Every lane must add the (entry, bucket)
pairs of a plain loop without look-ahead, and no load may leave the arrays, which have exactly the kernel's sizes.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("seg_walk") / "seg_walk_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "seg_walk_shim.cpp")])
    return exe


def test_every_lane_walks_like_the_plain_loop_and_stays_inside_the_arrays(shim):
    r = subprocess.run([shim], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 140 and int(words[2]) >= 5000, r.stdout
