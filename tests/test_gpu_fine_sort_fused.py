"""The fused fine level of the MSM's sort (k_fine_sort, myzkp_amd/csrc/mzk_msm.hip): one workgroup sorts a whole coarse bin from
registers; a bin above the capacity (33 x 1024 records) is cut into slices that extra workgroups of the same launch count and a second
launch of k_fine_scatter places.  Commits through mzk_srs_from_device_ex handles at every window width msm_plan selects the form for
(13 .. 20 bits), with the smallest n at which the plan takes the two-level sort at that width (read from the plan through
tests/hostcheck/fine_sort_shim.cpp: 16385, 4097, 4096 or 1 pairs) and with n + 3, which is no multiple of 1024.

Scalars: uniform; all zero (no entries at all); all equal (every window in one bucket); bytes; 16-bit values; half uniform and half one
repeated value.  At those sizes no bin is over-full, so at 13, 16 and 17 bits the patterns that fill bins are also committed at the
sizes at which they do: all equal at capacity + 4 pairs (every window's bin is sliced), half and half at 2 (capacity + 1) + 3 pairs
(whole bins and sliced bins in one launch), and constructed sets of exactly capacity and capacity + 1 scalars whose only non-zero
window holds a digit of one bin -- the last bin a workgroup sorts alone and the first it must leave to slices.

Every commitment is compared with the oracle's Pippenger (orc.msm_fast), and with the same call on the tuning build with
MZK_FINE_FUSED=0 (k_fine_count + k_fine_scatter, the two passes), point for point."""
import ctypes, functools, os, subprocess, sys
import numpy as np
import pytest
import orc
from orc import FR

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
WIDTHS = tuple(range(13, 21))
BIG_WIDTHS = (13, 16, 17)
PATTERNS = ("uniform", "zero", "equal", "bytes", "u16", "half")


@functools.lru_cache(maxsize=None)
def shim():
    exe = os.path.join(HERE, "hostcheck", "fine_sort_shim.cpp")
    import tempfile
    out = os.path.join(tempfile.mkdtemp(prefix="fine_sort_plan"), "fine_sort_shim")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", out, exe])
    return out


@functools.lru_cache(maxsize=None)
def plan(c, stride):
    out = subprocess.run([shim(), "plan", str(c), str(stride)], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(out[0::2], (int(v) for v in out[1::2])))


@functools.lru_cache(maxsize=None)
def sizes(c):
    """(smallest two-level n, n + 3) of width c; the handle holds n + 3 points"""
    n0 = plan(c, 1 << 15)["n"]
    p = plan(c, n0 + 3)
    assert p["n"] == n0 and p["fused"] == 1 and p["fused_plus3"] == 1, (c, p)
    return n0, n0 + 3


@functools.lru_cache(maxsize=None)
def capacity():
    return plan(17, 1 << 15)["cap"]


@functools.lru_cache(maxsize=None)
def points(n):
    return orc.synth_points(51, 2 * (capacity() + 1) + 3)[:n]


@functools.lru_cache(maxsize=None)
def scalars(pattern, n):
    """does not depend on the window width: one oracle result serves every width"""
    u = orc.synth_vector(FR, 52, n)
    if pattern == "uniform":
        return u
    s = np.zeros((n, 4), dtype=np.uint64)
    rng = np.random.default_rng(53)
    if pattern == "equal":
        s[:] = u[n // 2]
    elif pattern == "bytes":
        s[:, 0] = rng.integers(0, 256, size=n).astype(np.uint64)
    elif pattern == "u16":
        s[:, 0] = rng.integers(0, 1 << 16, size=n).astype(np.uint64)
    elif pattern == "half":
        s[:] = u
        s[n // 2:] = u[0]
    else:
        assert pattern == "zero"
    return s


@functools.lru_cache(maxsize=None)
def one_bin(c, n, stride):
    """n scalars whose only non-zero window is window 1, its digit in bin 3 of the coarse sort and spread over that bin's buckets: n
    records in one bin, none anywhere else (digits below half a window: no carry)"""
    p = plan(c, stride)
    F, bins = p["F"], p["bins"]
    assert bins * F == 1 << (c - 1) and 4 * F <= 1 << (c - 1)
    d = 3 * F + 1 + np.arange(n, dtype=np.int64) % F          # bucket d - 1 in [3 F, 4 F)
    return orc.to_limbs([int(v) << c for v in d], 4)


def big_cases(c):
    """name -> (scalars, n): the sizes at which bins are over-full"""
    cap = capacity()
    n_eq, n_half = cap + 4, 2 * (cap + 1) + 3
    for n in (n_eq, n_half, cap, cap + 1):
        p = plan(c, n)
        assert p["fused_at_stride"] == 1, (c, n, p)
    return {"equal_over": (scalars("equal", n_eq), n_eq), "half_over": (scalars("half", n_half), n_half),
            "at_capacity": (one_bin(c, cap, cap), cap), "capacity_plus_1": (one_bin(c, cap + 1, cap + 1), cap + 1)}


def all_cases():
    """(name, width, scalars, n points of the handle = the plan's table stride)"""
    for c in WIDTHS:
        n0, n3 = sizes(c)
        for pat in PATTERNS:
            yield "%s_%d_n0" % (pat, c), c, scalars(pat, n0), n3
            yield "%s_%d_n3" % (pat, c), c, scalars(pat, n3), n3
    for c in BIG_WIDTHS:
        for name, (s, n) in big_cases(c).items():
            yield "%s_%d" % (name, c), c, s, n


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def run_cases(mz):
    import torch
    L = mz.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    handles, res = {}, {}
    for name, c, scal, n_srs in all_cases():
        if (c, n_srs) not in handles:
            d_p, h = _dev(points(n_srs)), ctypes.c_void_p()
            assert L.mzk_srs_from_device_ex(ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(n_srs), c, ctypes.byref(h), st) == 0, L.mzk_last_error()
            torch.cuda.synchronize()
            assert (L.mzk_srs_window_bits(h), L.mzk_srs_bucket_sets(h)) == (c, 1)
            handles[(c, n_srs)] = h
        d_c, out = _dev(scal), torch.full((8,), -1, dtype=torch.int64, device="cuda")
        assert L.mzk_kzg_commit_srs_dev(handles[(c, n_srs)], ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(scal.shape[0]), ctypes.c_void_p(out.data_ptr()), 0, st) == 0, L.mzk_last_error()
        torch.cuda.synchronize()
        res[name] = mz.array_to_points(out.cpu().numpy().view(np.uint64).reshape(1, 8))[0]
    for h in handles.values():
        L.mzk_srs_free(h)
    return res


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import myzkp_amd as mz
import test_gpu_fine_sort_fused as t
mz.init(0)
print(repr(t.run_cases(mz)))
'''


@pytest.fixture(scope="module")
def want():
    """the oracle once per (scalars, points): the small patterns are shared by the widths"""
    @functools.lru_cache(maxsize=None)
    def ref(key):
        return orc.msm_fast(by_key[key][0], by_key[key][1])
    by_key, names = {}, {}
    for name, c, scal, n_srs in all_cases():
        key = (id(scal), scal.shape[0])
        by_key[key] = (scal, points(n_srs)[:scal.shape[0]])
        names[name] = key
    return {name: ref(key) for name, key in names.items()}


@pytest.fixture(scope="module")
def shipped():
    import myzkp_amd
    myzkp_amd.init(0)
    return run_cases(myzkp_amd)


@pytest.fixture(scope="module")
def two_pass():
    """the same calls with k_fine_count + k_fine_scatter forced: the switch is read once per process"""
    import myzkp_amd.build as b
    tuning = b.build(tuning=True)
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, MZK_HIP_LIB=tuning, MZK_FINE_FUSED="0"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return eval(p.stdout.strip().splitlines()[-1])


def test_the_constructed_sets_fill_one_bin_to_capacity_and_one_past_it():
    """the digits of the constructed scalars, recoded as walk_digits does: capacity (+ 1) records, all in bin 3, every bucket of it used"""
    cap = capacity()
    assert cap == 33 * 1024
    for c in BIG_WIDTHS:
        for n in (cap, cap + 1):
            F = plan(c, n)["F"]
            vals = orc.from_limbs(one_bin(c, n, n))
            digits = [(v >> c) & ((1 << c) - 1) for v in vals]
            assert all(v == d << c for v, d in zip(vals, digits)) and max(digits) <= 1 << (c - 1)
            bins = {(d - 1) // F for d in digits}
            assert bins == {3} and len({d for d in digits}) == F and len(digits) == n


@pytest.mark.parametrize("c", WIDTHS)
def test_commits_equal_the_oracle_at_the_smallest_two_level_sizes(want, shipped, c):
    n0, n3 = sizes(c)
    assert n3 % 1024 != 0
    for pat in PATTERNS:
        for tag in ("n0", "n3"):
            name = "%s_%d_%s" % (pat, c, tag)
            assert shipped[name] == want[name], name


@pytest.mark.parametrize("c", BIG_WIDTHS)
def test_commits_equal_the_oracle_where_bins_are_over_full(want, shipped, c):
    for name in ("equal_over", "half_over", "at_capacity", "capacity_plus_1"):
        assert shipped["%s_%d" % (name, c)] == want["%s_%d" % (name, c)], (name, c)


def test_the_two_pass_form_gives_the_same_points(want, shipped, two_pass):
    assert set(two_pass) == set(shipped) == set(want)
    for name, w in want.items():
        assert two_pass[name] == w and shipped[name] == w, name
