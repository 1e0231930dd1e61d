"""G2 arithmetic on the device against integers: the case tables of tests/g2_model.py through mzk_selftest_g2_probe (one function of
myzkp_amd/csrc/mzk_g2.h per call, raw limbs in, raw limbs out), as hipcc compiles the header for gfx950, judged by the integer model --
Fq2 sums and products limb for limb, the group operations against the affine law, every Fq of every output against the header's N2
bound.  The same tables pass the bounds-checked host build in tests/test_hostcheck_g2_probe.py, which is what shows every case to be
inside the callers' contracts; nothing is skipped or filtered here either."""
import ctypes, functools
import numpy as np
import pytest
import g2_model as gm

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import myzkp_amd as mz
    mz.init(0)
    return mz.lib()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _f2_table(op):
    return gm.f2_table(op)


@functools.lru_cache(maxsize=None)
def _g2_table(op):
    return gm.g2_table(op)


def run(L, op, cases):
    a, b, k = gm.pack(cases, "a"), gm.pack(cases, "b"), gm.pack(cases, "k")
    out = np.full((len(cases), gm.out_words(op)), 0xdeadbeef, dtype=np.uint32)
    rc = L.mzk_selftest_g2_probe(op, ctypes.c_size_t(len(cases)), _ptr(a), _ptr(b), _ptr(k), _ptr(out))
    assert rc == 0, L.mzk_last_error()
    return out


@pytest.mark.parametrize("op", gm.F2_OPS, ids=[gm.G2_NAMES[o] for o in gm.F2_OPS])
def test_fq2_op_on_the_device_against_integers(L, op):
    cases = _f2_table(op)
    assert len(cases) > 512           # several workgroups, every lane with work of its own
    for c, o in zip(cases, run(L, op, cases)):
        gm.check_f2(op, c, o)


@pytest.mark.parametrize("op", gm.GROUP_OPS, ids=[gm.G2_NAMES[o] for o in gm.GROUP_OPS])
def test_g2_op_on_the_device_against_the_affine_law(L, op):
    cases, cover = _g2_table(op)
    assert len(cases) > 512 or (op == gm.G2_SCALAR_MUL and 64 <= len(cases) <= 128)
    gm.assert_cover(op, cover)
    for c, o in zip(cases, run(L, op, cases)):
        gm.check_g2(op, c, o)


def test_g2_chains_feed_the_output_back(L):
    """the representations the device code itself produces: 32 mixed additions, 17 doublings, the 128-slot sum tree in k_g2_sum's
    order over random points and over equal points; 70 chains, so that more than one workgroup runs"""
    gm.run_chains(lambda op, cases: run(L, op, cases), chains=70)


def test_g2_probe_rejects_bad_arguments(L):
    """an unknown op, a null pointer the op needs, n above 2^20: MZK_E_ARG, nothing launched; n = 0 is fine"""
    buf = np.zeros(4 * 72, dtype=np.uint32)
    out = np.zeros(72, dtype=np.uint32)
    E_ARG = -1
    one = ctypes.c_size_t(1)
    for op in (14, -1, 99):
        assert L.mzk_selftest_g2_probe(op, one, _ptr(buf), _ptr(buf), _ptr(buf), _ptr(out)) == E_ARG, op
    assert L.mzk_selftest_g2_probe(gm.G2_ADD, one, None, _ptr(buf), _ptr(buf), _ptr(out)) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.G2_ADD, one, _ptr(buf), None, _ptr(buf), _ptr(out)) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.G2_MADD, one, _ptr(buf), None, None, _ptr(out)) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.F2_MUL, one, _ptr(buf), None, None, _ptr(out)) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.G2_SCALAR_MUL, one, _ptr(buf), None, None, _ptr(out)) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.G2_ADD, one, _ptr(buf), _ptr(buf), None, None) == E_ARG
    assert L.mzk_selftest_g2_probe(gm.G2_ADD, ctypes.c_size_t((1 << 20) + 1), _ptr(buf), _ptr(buf), None, _ptr(out)) == E_ARG
    assert b"g2_probe" in L.mzk_last_error()
    assert not out.any()
    assert L.mzk_selftest_g2_probe(gm.G2_ADD, ctypes.c_size_t(0), _ptr(buf), _ptr(buf), None, _ptr(out)) == 0       # n = 0: nothing to do
    assert L.mzk_selftest_g2_probe(gm.G2_DBL, one, _ptr(buf), None, None, _ptr(out)) == 0                          # b, k not needed
    assert not out.any()                                                                                           # 2 * infinity
