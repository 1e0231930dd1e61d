"""Every split of log2 n into passes that mzk_ntt.hip chooses between 2^15 and 2^23, Fr and M128, on real data and bit for bit against
the oracle's iterative transform: forward, inverse, the coset LDE with the pre-scale fused into the first strided pass, batches and
the in-place device call.

  lg     15     16     17       18       19       20                    21       22       23
  split  (8,7)  (8,8)  (6,6,5)  (6,6,6)  (7,6,6)  (10,10) | (7,7,6)     (7,7,7)  (8,7,7)  (8,8,7)

2^20 runs on the large tiles as a single transform and on (7,7,6) as a batch of three.  The write-through stores are on for
Fr 2^16 .. 2^21 and M128 2^17 .. 2^20 and off on both sides.  test_pass_counts reads the launch counts of the library's own phase
timers, so a change of ntt_plan (mzk_ntt_plan.h) that moves a size to another pass count fails here instead of leaving a split
untested.  test_gpu_ntt.py covers 2^0 .. 2^14, test_gpu_full_size.py 2^24."""
import ctypes
import numpy as np
import pytest
import orc
from orc import FR, M128

pytestmark = pytest.mark.gpu

FIDS = [FR, M128]
IDS = {FR: "Fr", M128: "M128"}
PH_NTT_PASS0 = 5                                   # MZK_PH_NTT_PASS0 .. PASS3 (include/mzk.h)
THREADS = 8


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    yield myzkp_amd
    _VEC.clear()
    _FWD.clear()


# ---- data and expected transforms, computed once -------------------------------------------------------------------------------
_VEC, _FWD = {}, {}


def ints(a):
    """(n, limbs) uint64 -> Python integers"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    w, raw = 8 * a.shape[1], a.tobytes()
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def limbs(vals, nl):
    return np.frombuffer(b"".join(v.to_bytes(8 * nl, "little") for v in vals), dtype=np.uint64).reshape(-1, nl).copy()


def vec(fid, lg, row=0):
    """synthetic elements with 0 first and p - 1 last; kept up to 2^21, the sizes that several tests share"""
    k = (fid, lg, row)
    if k in _VEC:
        return _VEC[k]
    v = orc.synth_vector(fid, 3000 + 64 * row + lg, 1 << lg, threads=THREADS)
    v[0] = 0
    v[-1] = limbs([orc.MOD[fid] - 1], orc.LIMBS[fid])[0]
    v.setflags(write=False)
    if lg <= 21:
        _VEC[k] = v
    return v


def oracle(fid, lg, v, inverse=False):
    rc, want = orc.ntt_fast(fid, orc.root_of(fid, lg), v, inverse=inverse, threads=THREADS)
    assert rc == 0
    return want


def fwd(fid, lg, row=0):
    """the oracle's transform of vec(fid, lg, row), kept like it"""
    k = (fid, lg, row)
    if k in _FWD:
        return _FWD[k]
    want = oracle(fid, lg, vec(fid, lg, row))
    want.setflags(write=False)
    if lg <= 21:
        _FWD[k] = want
    return want


# ---- forward and inverse ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg", range(15, 24))
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_forward_against_the_oracle(mz, fid, lg):
    got = mz.ntt(fid, orc.root_of(fid, lg), vec(fid, lg))
    assert np.array_equal(got, fwd(fid, lg))


@pytest.mark.parametrize("lg", range(15, 24))
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_inverse_against_the_oracle(mz, fid, lg):
    """up to 2^21 against the oracle's inverse; above, where the forward test has already paid for the oracle, intt(ntt(x)) == x"""
    w, v = orc.root_of(fid, lg), vec(fid, lg)
    if lg <= 21:
        assert np.array_equal(mz.intt(fid, w, v), oracle(fid, lg, v, inverse=True))
    else:
        assert np.array_equal(mz.intt(fid, w, mz.ntt(fid, w, v)), v)


# ---- the split that ran ------------------------------------------------------------------------------------------------------------
def pass_launches(mz, call):
    """launches per NTT pass phase while `call` runs"""
    L = mz.lib()
    assert L.mzk_prof_select(ctypes.c_uint32(0xffffffff)) == 0      # (the default: every phase)
    assert L.mzk_prof_enable(1) == 0
    try:
        assert L.mzk_prof_reset() == 0
        call()
        out = []
        for t in range(4):
            ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
            assert L.mzk_prof_read(PH_NTT_PASS0 + t, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            out.append(cnt.value)
        return out
    finally:
        L.mzk_prof_enable(0)
        L.mzk_prof_reset()


@pytest.mark.parametrize("lg", range(15, 24))
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_pass_counts(mz, fid, lg):
    """two passes at 2^15 and 2^16, three from 2^17 on, except the single 2^20 transform (two passes of 2^10 on the large tiles)"""
    x = np.zeros((1 << lg, orc.LIMBS[fid]), dtype=np.uint64)
    want = [1, 1, 0, 0] if lg <= 16 or lg == 20 else [1, 1, 1, 0]
    assert pass_launches(mz, lambda: mz.ntt(fid, orc.root_of(fid, lg), x)) == want


@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_pass_counts_of_a_batch_at_2_20(mz, fid):
    """three transforms of 2^20 leave the large tiles: (7,7,6)"""
    x = np.zeros((3, 1 << 20, orc.LIMBS[fid]), dtype=np.uint64)
    assert pass_launches(mz, lambda: mz.ntt_batch(fid, orc.root_of(fid, 20), x)) == [1, 1, 1, 0]


# ---- coset LDE: Polynomial::scale and the padding inside the first strided pass --------------------------------------------------
@pytest.mark.parametrize("lg,whole", [(15, False), (15, True), (17, False), (17, True), (18, False), (18, True), (19, False), (19, True), (21, False)])
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_coset_lde_fused_prescale(mz, fid, lg, whole):
    """order / 4 + 3 coefficients (an odd count: the zero padding starts inside a tile) or `order` of them (none).  The offsets
    alternate and then repeat, so the offset-power tables are built, rebuilt and reused.  Expected: coefficient i times offset^i in
    Python integers, padded, through the oracle's transform."""
    p, nl = orc.MOD[fid], orc.LIMBS[fid]
    order = 1 << lg
    ncoef = order if whole else order // 4 + 3
    gen = orc.root_of(fid, lg)
    coef = vec(fid, lg)[:ncoef]
    vals = ints(coef)
    want = {}
    for off in (orc.M128_GEN % p, 5, orc.M128_GEN % p, orc.M128_GEN % p):
        if off not in want:
            acc, sc = 1, []
            for x in vals:
                sc.append(x * acc % p)
                acc = acc * off % p
            padded = np.zeros((order, nl), dtype=np.uint64)
            padded[:ncoef] = limbs(sc, nl)
            want[off] = oracle(fid, lg, padded)
        assert np.array_equal(mz.coset_lde(fid, coef, off, gen, order), want[off]), off


# ---- batches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg,batch", [(15, 3), (17, 3), (19, 2), (20, 3), (21, 2)])
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_batch_against_the_oracle(mz, fid, lg, batch):
    """every row against the oracle's transform of that row, and back; (20, 3) is the batch that runs 2^20 as (7,7,6)"""
    w = orc.root_of(fid, lg)
    rows = np.stack([vec(fid, lg, r) for r in range(batch)])
    got = mz.ntt_batch(fid, w, rows)
    for r in range(batch):
        assert np.array_equal(got[r], fwd(fid, lg, r)), r
    assert np.array_equal(mz.ntt_batch(fid, w, got, inverse=True), rows)
    for r in range(1, batch):                      # row 0 serves the other tests
        _VEC.pop((fid, lg, r), None)
        _FWD.pop((fid, lg, r), None)


# ---- in place ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lg", [15, 18])
@pytest.mark.parametrize("fid", FIDS, ids=IDS.get)
def test_device_call_in_place(mz, fid, lg):
    """mzk_ntt_dev with d_in == d_out: the first pass reads the caller's buffer, the last one writes it"""
    import torch
    L, nl, n = mz.lib(), orc.LIMBS[fid], 1 << lg
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    root = limbs([orc.root_of(fid, lg)], nl)
    v = vec(fid, lg)
    d = torch.from_numpy(v.view(np.int64).reshape(-1).copy()).to(torch.device("cuda", 0))
    for inverse, want in ((0, fwd(fid, lg)), (1, v)):
        rc = L.mzk_ntt_dev(fid, root.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(d.data_ptr()), ctypes.c_void_p(d.data_ptr()), ctypes.c_size_t(n), inverse, st)
        assert rc == 0, L.mzk_last_error().decode()
        torch.cuda.synchronize()
        assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(-1, nl), want), inverse
