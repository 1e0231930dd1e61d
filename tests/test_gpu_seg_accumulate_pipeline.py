"""k_seg_accumulate's two-deep pipeline (myzkp_amd/csrc/mzk_msm.hip; the index logic alone: tests/test_hostcheck_seg_walk.py) on the
device, at the sizes where its look-ahead meets an end: the smallest n on the segmented path (SMALL_MAX_N of mzk_msm_plan.h) and the
next one, entry counts that leave the LAST segment one entry and two entries, fixed segment lengths 1, 2 and 3 (tuning build) and the
sentinel form of the grid-batched commitments.  The commit against an SRS handle and the generic MSM, with an infinity point, P next
to -P and repeats among the inputs, against the oracle's Pippenger."""
import ctypes, os, subprocess, sys
import numpy as np
import pytest
import orc
from orc import FR, P_FQ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SMALL_MAX_N = 4097           # mzk_msm_plan.h: merged layouts below it (and generic ones below SMALL_MAX_N - 1) take the short paths
SEG_MIN = 8                  # mzk_msm.hip: the shortest segment the kernels derive from the entry count
PLAIN, TABLES = 0, 2


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """msm_plan through tests/hostcheck/msm_plan_shim.cpp: path, segment length and segment count of a call"""
    import torch
    so = str(tmp_path_factory.mktemp("seg_pipeline") / "libmsmplan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(HERE, "hostcheck", "msm_plan_shim.cpp")])
    L = ctypes.CDLL(so)
    L.plan_fields.restype = ctypes.c_char_p
    L.plan.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    names = L.plan_fields().decode().split()
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count

    def f(n, kind, stride):
        out = (ctypes.c_uint64 * len(names))()
        assert L.plan(n, n, n, kind, stride, num_cu, 0, out) == len(names)
        return dict(zip(names, out))
    return f


@pytest.fixture(scope="module")
def glv_split():
    """glv_split of mzk_glv.h on the host (hc_glv_split of tests/hostcheck/hostcheck.cpp, the library test_hostcheck_probe.py builds)"""
    import glob
    src, so = os.path.join(HERE, "hostcheck", "hostcheck.cpp"), os.path.join(HERE, "hostcheck", "libhostcheck.so")
    hdrs = glob.glob(os.path.join(ROOT, "myzkp_amd", "csrc", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DMZK_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src])
    hc = ctypes.CDLL(so)

    def f(limbs4):
        k = np.zeros(8, dtype=np.uint32)
        k[:] = np.ascontiguousarray(limbs4, dtype=np.uint64).view(np.uint32)
        out = np.zeros(10, dtype=np.uint32)
        hc.hc_glv_split(k.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
        return [int(x) for x in out[:4]], int(out[4]), [int(x) for x in out[5:9]], int(out[9])
    return f


def _srs(mz, pts, width):
    import torch
    L = mz.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_p = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64).reshape(-1).copy()).cuda()
    h = ctypes.c_void_p()
    assert L.mzk_srs_from_device_ex(ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(pts.shape[0]), int(width), ctypes.byref(h), st) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    return h


def _commit(mz, h, coef):
    import torch
    L = mz.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_c = torch.from_numpy(np.ascontiguousarray(coef).view(np.int64).reshape(-1).copy()).cuda()
    d_o = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(coef.shape[0]), ctypes.c_void_p(d_o.data_ptr()), 0, st) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    return mz.array_to_points(d_o.cpu().numpy().view(np.uint64).reshape(1, 8))[0]


def _commit_many(mz, h, coefs):
    import torch
    L = mz.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    count, n = coefs.shape[0], coefs.shape[1]
    d_c = torch.from_numpy(np.ascontiguousarray(coefs).view(np.int64).reshape(-1).copy()).cuda()
    d_o = torch.full((count * 8,), -1, dtype=torch.int64, device="cuda")
    assert L.mzk_kzg_commit_srs_many_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(n), ctypes.c_size_t(count), ctypes.c_void_p(d_o.data_ptr()), st) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    return mz.array_to_points(d_o.cpu().numpy().view(np.uint64).reshape(-1, 8)[:count])


def edge_points(seed, n):
    """points with a run of repeats, P next to -P and points at infinity (test_edge_batch of test_gpu_msm.py)"""
    p = orc.synth_points(seed, n)
    p[300:340] = p[300]
    p[700] = p[701]
    p[700, 4:] = orc.to_limbs([P_FQ - orc.from_limbs(p[701:702, 4:])[0]], 4)[0]
    p[900:904] = 0
    p[n - 1] = 0                                 # the very last entry of the last window reads the point at infinity
    return p


def edge_scalars(seed, n):
    s = orc.synth_vector(FR, seed, n)
    s[0], s[1] = 0, orc.to_limbs([orc.P_FR - 1], 4)[0]
    s[10:60] = s[10]                             # repeated scalars
    s[300:340] = s[300]                          # ... on the repeated point: the bucket sees P + P
    s[700] = s[701]                              # ... and P + (-P)
    return s


def sparse_scalars(seed, n, c, windows, T, last):
    """scalars whose c-bit windows are zero or in [1, 2^(c-1)) -- no signed-digit carry, so the sort emits exactly one entry per
    non-zero window -- thinned until the segment length the kernels derive from the entry count (segment_length, mzk_msm.hip) leaves
    the last segment `last` entries.  Returns the scalars, the entry count and that segment length."""
    rng = np.random.default_rng(seed)
    ch = rng.integers(1, 1 << (c - 1), size=(n, windows), dtype=np.int64) * (rng.random((n, windows)) < 0.7)
    ch[10:60] = ch[10]
    ch[300:340] = ch[300]
    ch[700] = ch[701]
    ch[0] = 0
    total = int(np.count_nonzero(ch))
    live = [tuple(ix) for ix in np.argwhere(ch[1000:] != 0)]          # thin behind the structured rows
    seg = lambda t: max(SEG_MIN, -(-t // T))
    while total % seg(total) != last:
        i, w = live.pop()
        ch[1000 + i, w] = 0
        total -= 1
    vals = [sum(int(ch[i, w]) << (c * w) for w in range(windows)) for i in range(n)]
    assert max(vals) < orc.P_FR
    return orc.to_limbs(vals, 4), total, seg(total)


@pytest.mark.parametrize("width", [14, 16])
def test_commit_at_the_first_sizes_of_the_segmented_path(mz, plan, width):
    """14-bit tables: 8192 buckets, the widest layout that still has a short path below SMALL_MAX_N; 16-bit tables are the width the
    SRS sizes of this range get when they are part of a longer SRS"""
    N = SMALL_MAX_N + 3
    p = edge_points(70 + width, N)
    h = _srs(mz, p, width)
    kind = TABLES | (width << 8) | (1 << 16)
    if width == 14:
        assert plan(SMALL_MAX_N - 1, kind, N)["path"] <= 1 < plan(SMALL_MAX_N, kind, N)["path"]      # SmallScan / SmallSort below, sorted above
    for n in (SMALL_MAX_N, SMALL_MAX_N + 1):
        assert plan(n, kind, N)["path"] > 1
        s = edge_scalars(80 + n, n)
        assert _commit(mz, h, s) == orc.msm_fast(s, p[:n]), (width, n)
    mz.lib().mzk_srs_free(h)


@pytest.mark.parametrize("last", [1, 2])
def test_commit_whose_last_segment_has_one_or_two_entries(mz, plan, last):
    n, c = SMALL_MAX_N + 2, 16
    p = edge_points(91, n)
    h = _srs(mz, p, c)
    P = plan(n, TABLES | (c << 8) | (1 << 16), n)
    assert P["path"] > 1
    s, total, seg = sparse_scalars(92 + last, n, c, 15, int(P["T"]), last)      # (the 16th window holds 14 bits: left zero, the scalars stay below r)
    assert total % seg == last and total > 4 * seg
    assert _commit(mz, h, s) == orc.msm_fast(s, p), (total, seg)
    mz.lib().mzk_srs_free(h)


def test_generic_msm_at_the_first_sizes_of_the_segmented_path(mz, plan):
    assert plan(SMALL_MAX_N - 2, PLAIN, 0)["path"] <= 1          # SmallScan / SmallSort: the generic layout's short path ends one pair earlier
    for n in (SMALL_MAX_N - 1, SMALL_MAX_N):
        assert plan(n, PLAIN, 0)["path"] > 1
        s, p = edge_scalars(100 + n, n), edge_points(101 + n, n)
        assert mz.msm_g1(s, p) == orc.msm_fast(s, p), n


@pytest.mark.parametrize("last", [1, 2])
def test_generic_msm_whose_last_segment_has_one_or_two_entries(mz, plan, glv_split, last):
    """scalars below 2^100: the GLV split leaves them whole (k2 = 0), so the entries are the non-zero windows of the scalar itself"""
    n = SMALL_MAX_N + 1
    P = plan(n, PLAIN, 0)
    c = int(P["c"])
    assert P["path"] > 1 and 100 // c <= int(P["nwin"])
    s, total, seg = sparse_scalars(110 + last, n, c, 100 // c, int(P["T"]), last)
    assert total % seg == last and total > 4 * seg
    for row in s:                                # the entry count above is the kernel's only if the split leaves every scalar whole
        k1, neg1, k2, _ = glv_split(row)
        words = [int(x) for x in np.ascontiguousarray(row, dtype=np.uint64).view(np.uint32)]
        assert k1 == words[:4] and not any(words[4:]) and neg1 == 0 and not any(k2), row
    p = edge_points(111, n)
    assert mz.msm_g1(s, p) == orc.msm_fast(s, p), (total, seg)


CHILD = r'''
import ctypes, sys, numpy as np
sys.path.insert(0, "tests")
import orc, myzkp_amd as mz
import test_gpu_seg_accumulate_pipeline as t
mz.init(0)
n = 4096 + 3
s, p = t.edge_scalars(120, n), t.edge_points(121, n)
h = t._srs(mz, p, 16)
print(repr((t._commit(mz, h, s), mz.msm_g1(s, p))))
'''


def test_fixed_segment_lengths_one_two_three_in_the_tuning_build():
    """MZK_ACC_SEG = 1, 2, 3: segments as short as the look-ahead is deep, every entry its own segment at 1.  The switches are read
    once per process: one child per setting, one after the other."""
    import myzkp_amd.build as b
    tuning = b.build(tuning=True)
    n = 4096 + 3
    s, p = edge_scalars(120, n), edge_points(121, n)
    want = orc.msm_fast(s, p)
    for seg in (1, 2, 3):
        env = dict(os.environ, MZK_HIP_LIB=tuning, MZK_ACC_SEG=str(seg))
        r = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (seg, r.stderr[-2000:])
        commit, generic = eval(r.stdout.strip().splitlines()[-1])
        assert commit == want and generic == want, seg


def test_many_commits_of_31_byte_coefficients_equal_the_single_calls(mz):
    """4 x 2^10 coefficients of 31 bytes: the one-kernel sort's fixed-capacity regions end in runs of sentinels, which the accumulate
    must skip without forming a table address from them"""
    n, count = 1 << 10, 4                        # (at most MANY_CHUNK = 1024 coefficients: the one-kernel sort, the only caller of the sentinel form)
    p = edge_points(130, n)
    h = _srs(mz, p, 1)
    coefs = np.stack([orc.synth_vector(FR, 131 + k, n) for k in range(count)])
    coefs[:, :, 3] &= np.uint64((1 << 56) - 1)
    coefs[2][1:] = 0                             # a polynomial of one coefficient: its region is nearly all sentinels
    got = _commit_many(mz, h, coefs)
    for k in range(count):
        assert got[k] == orc.msm_fast(coefs[k], p), k
        assert got[k] == _commit(mz, h, coefs[k]), k
    mz.lib().mzk_srs_free(h)
