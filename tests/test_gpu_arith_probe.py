"""Device field and group arithmetic against integers, limb for limb: the case table of tests/arith_model.py through the arithmetic
probe (mzk_selftest_field_probe / mzk_selftest_g1_probe: one device function per call, raw limbs in, raw limbs out), every form a
function exists in -- portable as hipcc compiles it for gfx950, the generated inline-asm blocks, the quad- and row-cooperative
group operations, the wave-cooperative inversion -- judged by the integer model.  The same table passes the bounds-checked host
build in tests/test_hostcheck_probe.py, which is what shows every case to be inside the callers' contracts; nothing is skipped or
filtered here either.  A failure names field, op, form, case class, the operands and the first differing limb."""
import ctypes, functools, random
import numpy as np
import pytest
import arith_model as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import myzkp_amd as mz
    mz.init(0)
    return mz.lib()


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def _field_table(fid, op):
    f = [x for x in am.FIELDS if x.fid == fid][0]
    return am.field_table(f, op)


@functools.lru_cache(maxsize=None)
def _g1_table(op):
    return am.g1_table(op)


def run_field(L, f, op, form, cases):
    arr = am.pack_cases(cases, f.L)
    out = np.full((len(cases), f.L), 0xdeadbeef, dtype=np.uint32)
    rc = L.mzk_selftest_field_probe(f.fid, op, form, ctypes.c_size_t(len(cases)), _ptr(arr), _ptr(out))
    assert rc == 0, L.mzk_last_error()
    return out


FIELD_CASES = [(f, op, form) for f in am.FIELDS for op in am.field_ops(f) for form in am.field_forms(f, op)]


@pytest.mark.parametrize("f,op,form", FIELD_CASES, ids=["%s-%s-%s" % (f.name, am.OP_NAMES[op], am.FORM_NAMES[form]) for f, op, form in FIELD_CASES])
def test_field_op_on_the_device_against_integers(L, f, op, form):
    cases = _field_table(f.fid, op)
    assert len(cases) > 512           # several workgroups of 256, every lane with work of its own
    if form == am.FORM_WAVE:          # one case per wave: the edge classes in full, a share of the random ones
        cases = [c for c in cases if not c["cls"].startswith("random")] + [c for c in cases if c["cls"].startswith("random")][:256]
    out = run_field(L, f, op, form, cases)
    for c, o in zip(cases, out):
        am.check_field(f, op, form, c, o)


def test_asm_and_portable_products_return_the_same_limbs(L):
    """mzk_ec.h:65 promises it; both are pinned on the integers above, this names the pair if they ever part"""
    for f, op, form in FIELD_CASES:
        if form != am.FORM_ASM:
            continue
        cases = _field_table(f.fid, op)
        a, b = run_field(L, f, op, am.FORM_CPP, cases), run_field(L, f, op, am.FORM_ASM, cases)
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert bad.size == 0, (f.name, am.OP_NAMES[op], cases[bad[0]], a[bad[0]], b[bad[0]])


def run_g1(L, op, form, cases):
    n = len(cases)
    a = np.array([c["a"] for c in cases], dtype=np.uint32)
    b = None if cases[0]["b"] is None else np.array([c["b"] for c in cases], dtype=np.uint32)
    neg = np.array([c["neg"] for c in cases], dtype=np.uint8)
    out = np.full((n, 36), 0xdeadbeef, dtype=np.uint32)
    rc = L.mzk_selftest_g1_probe(op, form, ctypes.c_size_t(n), _ptr(a), _ptr(b), _ptr(neg), _ptr(out))
    assert rc == 0, L.mzk_last_error()
    return out


G1_CASES = [(op, form) for op in range(6) for form in am.g1_forms(op)]


@pytest.mark.parametrize("op,form", G1_CASES, ids=["%s-%s" % (am.G1_NAMES[op], am.FORM_NAMES[form]) for op, form in G1_CASES])
def test_g1_op_on_the_device_against_the_affine_law(L, op, form):
    cases, cover = _g1_table(op)
    # the table reaches every multiple of p the zero tests of the exceptional branches can meet, none above the KMAX the code passes
    for key, seen in cover.items():
        assert seen == am.G1_K_EXPECTED[(op, key)], (am.G1_NAMES[op], key, seen)
        assert max(seen) <= am.G1_KMAX[op][0 if key == "P" else 1]
    assert bool(cover) == (op in am.G1_KMAX)
    out = run_g1(L, op, form, cases)
    for c, o in zip(cases, out):
        am.check_g1_slot(op, form, c, o)
    if form == am.FORM_ASM:          # same column sums: identical limbs (mzk_ec.h:65)
        ref = run_g1(L, op, am.FORM_CPP, cases)
        for c, o, r in zip(cases, out, ref):
            d = am.first_diff(o, r)
            assert d is None, "G1 %s class=%s: FeAsm and FeCpp slots differ first at limb %d\n a=%s\n b=%s neg=%d" % (
                am.G1_NAMES[op], c["cls"], d, c["a"], c["b"], c["neg"])


def _chain(L, op, form, steps, chains, seed):
    """`chains` independent chains of `steps` dependent operations, the output slot of one step the accumulator of the next"""
    rng = random.Random(seed)
    pts = [am.aff_mul(am.G1_GEN, rng.randrange(1, am.FR.p)) for _ in range(chains)]
    state = [{"A": P, "a": am.slot_of(P, rng.randrange(1, am.Q), (1, 1, 0, 0))} for P in pts]
    for s in range(steps):
        cases = []
        for k, st in enumerate(state):
            if op == am.G1_MADD_SIGNED:      # alternating signs, the start point coming back every fifth step
                B = pts[k] if s % 5 == 0 else pts[(k + 1) % chains]
                cases.append({"cls": "chain %d step %d" % (k, s), "a": st["a"], "b": am.affine_limbs(B), "neg": s & 1, "A": st["A"], "B": B})
            else:
                cases.append({"cls": "chain %d step %d" % (k, s), "a": st["a"], "b": None, "neg": 0, "A": st["A"], "B": None})
        out = run_g1(L, op, form, cases)
        for c, o in zip(cases, out):
            am.check_g1_slot(op, form, c, o)
        state = [{"A": am.g1_expected(op, c), "a": [int(x) for x in o]} for c, o in zip(cases, out)]


@pytest.mark.parametrize("form", [am.FORM_CPP, am.FORM_ASM], ids=["cpp", "asm"])
def test_madd_signed_chain_feeds_its_output_back(L, form):
    _chain(L, am.G1_MADD_SIGNED, form, 32, 70, 5)


@pytest.mark.parametrize("form", [am.FORM_CPP, am.FORM_ASM, am.FORM_QUAD, am.FORM_ROW], ids=["cpp", "asm", "quad", "row"])
def test_dbl_chain_feeds_its_output_back(L, form):
    _chain(L, am.G1_DBL, form, 17, 70, 6)


def test_probe_rejects_bad_arguments(L):
    """unknown field / op / form, a form the op does not have, null pointers, n above 2^20: MZK_E_ARG, nothing launched"""
    buf = np.zeros(4 * 36, dtype=np.uint32)
    out = np.zeros(36, dtype=np.uint32)
    neg = np.zeros(4, dtype=np.uint8)
    E_ARG = -1
    one = ctypes.c_size_t(1)
    for fid, op, form in ((9, am.MUL, 0), (0, 26, 0), (0, -1, 0), (0, am.MUL, 7), (0, am.SMUL, 0), (2, am.SHOUP_MUL, 0), (1, am.SHOUP_MUL, 1),
                          (0, am.ADD, am.FORM_ASM), (0, am.INV, am.FORM_WAVE), (1, am.SMUL_C1, am.FORM_ASM), (2, am.MUL, am.FORM_QUAD)):
        assert L.mzk_selftest_field_probe(fid, op, form, one, _ptr(buf), _ptr(out)) == E_ARG, (fid, op, form)
    assert L.mzk_selftest_field_probe(0, am.MUL, 0, one, None, _ptr(out)) == E_ARG
    assert L.mzk_selftest_field_probe(0, am.MUL, 0, one, _ptr(buf), None) == E_ARG
    assert L.mzk_selftest_field_probe(0, am.MUL, 0, ctypes.c_size_t((1 << 20) + 1), _ptr(buf), _ptr(out)) == E_ARG
    for op, form in ((6, 0), (-1, 0), (am.G1_ADD, 5), (am.G1_MADD, am.FORM_QUAD), (am.G1_MADD_SIGNED, am.FORM_ROW), (am.G1_DBL_AFFINE, am.FORM_ASM),
                     (am.G1_TO_AFFINE, am.FORM_ROW), (am.G1_DBL, am.FORM_WAVE)):
        assert L.mzk_selftest_g1_probe(op, form, one, _ptr(buf), _ptr(buf), _ptr(neg), _ptr(out)) == E_ARG, (op, form)
    assert L.mzk_selftest_g1_probe(am.G1_ADD, 0, one, None, _ptr(buf), _ptr(neg), _ptr(out)) == E_ARG
    assert L.mzk_selftest_g1_probe(am.G1_ADD, 0, one, _ptr(buf), None, _ptr(neg), _ptr(out)) == E_ARG
    assert L.mzk_selftest_g1_probe(am.G1_MADD_SIGNED, 0, one, _ptr(buf), _ptr(buf), None, _ptr(out)) == E_ARG
    assert L.mzk_selftest_g1_probe(am.G1_ADD, 0, one, _ptr(buf), _ptr(buf), _ptr(neg), None) == E_ARG
    assert L.mzk_selftest_g1_probe(am.G1_ADD, 0, ctypes.c_size_t((1 << 20) + 1), _ptr(buf), _ptr(buf), _ptr(neg), _ptr(out)) == E_ARG
    assert L.mzk_selftest_field_probe(0, am.MUL, 0, ctypes.c_size_t(0), _ptr(buf), _ptr(out)) == 0       # n = 0: nothing to do
