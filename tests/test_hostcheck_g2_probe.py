"""The case tables of tests/g2_model.py, WHOLE, through the host build of myzkp_amd/csrc/mzk_g2.h (tests/hostcheck: hc_g2_probe, the
per-lane forms of mzk_probe.h compiled by g++ with -DMZK_CHECK_BOUNDS), judged by the integer model: Fq2 sums and products limb for
limb, the group operations against the affine law, every Fq of every output against the header's N2 bound (normalised limbs, value
below 2.01 p).  This run is also what shows every case to be inside the callers' contracts (a case outside them trips a bounds
assertion of the headers here) before tests/test_gpu_g2_probe.py trusts it on the device.  No case is skipped or filtered.  CPU only."""
import ctypes, glob, os, subprocess
import numpy as np
import pytest
import g2_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def hc():
    src = os.path.join(HERE, "hostcheck", "hostcheck.cpp")
    so = os.path.join(HERE, "hostcheck", "libhostcheck.so")
    hdrs = glob.glob(os.path.join(ROOT, "myzkp_amd", "csrc", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DMZK_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run(hc, op, cases):
    a, b, k = gm.pack(cases, "a"), gm.pack(cases, "b"), gm.pack(cases, "k")
    assert a.shape == (len(cases), gm.a_words(op)) and (b is None) == (gm.b_words(op) == 0) and (k is None) == (op != gm.G2_SCALAR_MUL)
    assert b is None or b.shape == (len(cases), gm.b_words(op))
    out = np.full((len(cases), gm.out_words(op)), 0xdeadbeef, dtype=np.uint32)
    assert hc.hc_g2_probe(op, ctypes.c_size_t(len(cases)), _ptr(a), _ptr(b), _ptr(k), _ptr(out)) == 0
    return out


@pytest.mark.parametrize("op", gm.F2_OPS, ids=[gm.G2_NAMES[o] for o in gm.F2_OPS])
def test_fq2_op_whole_table_against_integers(hc, op):
    cases = gm.f2_table(op)
    assert len(cases) > 512
    for c, o in zip(cases, run(hc, op, cases)):
        gm.check_f2(op, c, o)


def test_is_zero_table_holds_every_multiple():
    """each coefficient k p for k = 0 .. KMAX + 2 (what the IS_ZERO_MOD tables of arith_model use relative to their KMAX), every pair"""
    p = gm.Q
    pairs = {(v0 // p, v1 // p) for v0, v1 in (gm.f2_of(c["a"]) for c in gm.f2_table(gm.F2_IS_ZERO, nrand=0)) if v0 % p == 0 and v1 % p == 0}
    assert pairs == {(a, b) for a in range(gm.G2_KMAX + 3) for b in range(gm.G2_KMAX + 3)}
    cl = " | ".join(c["cls"] for c in gm.f2_table(gm.F2_IS_ZERO, nrand=0))
    for need in ("(3p, nonzero)", "(nonzero, 3p)", "(3p+1, 3p)", "(3p, 3p-1)", "(4p, 0p)", "(0p, 4p)", "(2p+2^29, 1p)", "(1p, 2p+2^232)"):
        assert need in cl, need


@pytest.mark.parametrize("op", gm.GROUP_OPS, ids=[gm.G2_NAMES[o] for o in gm.GROUP_OPS])
def test_g2_op_whole_table_against_the_affine_law(hc, op):
    cases, cover = gm.g2_table(op)
    assert len(cases) > 512 or (op == gm.G2_SCALAR_MUL and 64 <= len(cases) <= 128)
    for c in cases:
        assert gm.on_curve2(c["A"]) and gm.on_curve2(c["B"])          # the off-curve doubling slots carry no point: A is None
    gm.assert_cover(op, cover)
    for c, o in zip(cases, run(hc, op, cases)):
        gm.check_g2(op, c, o)


def test_tables_hold_the_classes_they_are_built_for():
    for op in (gm.G2_MADD, gm.G2_ADD):
        cl = " | ".join(c["cls"] for c in gm.g2_table(op, nrand=32)[0])
        for need in ("another point", "the same point", "its negative", "the generator", "z=1", "z random", "z.c0=0", "z.c1=0", "jXY=0", "jXY=f",
                     "exceptional doubling", "exceptional cancelling", "random, equal or opposite"):
            assert need in cl, (gm.G2_NAMES[op], need)
        assert ("infinity + q" in cl) if op == gm.G2_MADD else all(n in cl for n in ("a + infinity", "infinity + b", "infinity + infinity"))
    assert sum(c["cls"] == "off-curve, completeness branch" for c in gm.g2_table(gm.G2_DBL)[0]) == 4
    ks = {c["K"] for c in gm.g2_table(gm.G2_SCALAR_MUL)[0]}
    assert {0, 1, 2, 3, gm.RORD - 1, 1 << 253, (1 << 253) - 1} <= ks and max(ks) < gm.RORD


def test_g2_model_agrees_with_the_oracle():
    """second opinion on the model's Fq2 and affine formulas (the expectation itself never calls the oracle)"""
    import orc
    assert gm.G2_GEN == orc.G2_GEN and gm.on_curve2(gm.G2_GEN)
    cases, _ = gm.g2_table(gm.G2_ADD, nrand=40)
    for c in cases[::97] + cases[-40::8]:
        A, B = c["A"] or orc.G2_INF, c["B"] or orc.G2_INF
        assert orc.g2_add(A, B) == (gm.aff2_add(c["A"], c["B"]) or orc.G2_INF)
    for c in gm.g2_table(gm.G2_SCALAR_MUL)[0][::9]:
        assert orc.g2_mul(c["A"], c["K"]) == (gm.aff2_mul(c["A"], c["K"]) or orc.G2_INF)


def test_g2_chains_feed_the_output_back(hc):
    """the representations the code itself produces: 32 mixed additions, 17 doublings, the 128-slot sum tree in k_g2_sum's order"""
    gm.run_chains(lambda op, cases: run(hc, op, cases))
