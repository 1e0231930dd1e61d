"""The case table of tests/arith_model.py, WHOLE, through the host build of the device headers (tests/hostcheck: hc_field_probe /
hc_g1_probe, the portable per-lane forms of myzkp_amd/csrc/mzk_probe.h compiled by g++ with -DMZK_CHECK_BOUNDS), judged limb for
limb by the integer model.  Two jobs: the lazy-operand contracts of the products and the representation-dependent branches of the
group law are checked against integers without a GPU, and every case of the table is shown to respect the callers' contracts (a
case outside them trips a bounds assertion of the headers here) before tests/test_gpu_arith_probe.py trusts it on the device.  No
case is skipped or filtered.  CPU only."""
import ctypes, os, subprocess
import numpy as np
import pytest
import arith_model as am

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def hc():
    import glob
    src = os.path.join(HERE, "hostcheck", "hostcheck.cpp")
    so = os.path.join(HERE, "hostcheck", "libhostcheck.so")
    hdrs = glob.glob(os.path.join(ROOT, "myzkp_amd", "csrc", "*.h"))
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-DMZK_CHECK_BOUNDS", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_field(hc, f, op, cases):
    arr = am.pack_cases(cases, f.L)
    assert arr.shape == (len(cases), am.arity(op) * f.L)
    out = np.zeros((len(cases), f.L), dtype=np.uint32)
    assert hc.hc_field_probe(f.fid, op, ctypes.c_size_t(len(cases)), _ptr(arr), _ptr(out)) == 0
    return out


FIELD_OPS = [(f, op) for f in am.FIELDS for op in am.field_ops(f)]


@pytest.mark.parametrize("f,op", FIELD_OPS, ids=["%s-%s" % (f.name, am.OP_NAMES[op]) for f, op in FIELD_OPS])
def test_field_op_whole_table_against_integers(hc, f, op):
    cases = am.field_table(f, op)
    assert len(cases) > 30
    out = run_field(hc, f, op, cases)
    for c, o in zip(cases, out):
        am.check_field(f, op, am.FORM_CPP, c, o)


def test_table_covers_every_class_the_callers_produce():
    """the classes the table is built to hold are in it (a builder that silently dropped one would leave the tests green)"""
    for f in am.FIELDS:
        cl = " | ".join(c["cls"] for c in am.field_table(f, am.MUL, nrand=0))
        for need in ("zero", "one", "p-1", "2p-1", "all-ones", "single-limb-0", "single-limb-%d" % (f.L - 1), "4p-b", "8p-b", "a+8p-b", "doubled",
                     "lazy-random", "top-limb-max"):
            assert need in cl, (f.name, need)
    cl = " | ".join(c["cls"] for c in am.field_table(am.FQ, am.MUL_ADD2, nrand=0))
    assert "Rd Vd + (8p-Y1) PPP at the bounds" in cl
    # the borrow path: limb 0 of the biased, carried value below the folded quotient
    p = am.M128.p
    borrow = 0
    for c in am.field_table(am.M128, am.SREDUCE, nrand=0):
        x = am.slimbs(am.svalue(c["ops"][0]) + (1 << 12) * p, 5)
        borrow += x[0] < x[4] // am.M128.PT
    assert borrow >= 40
    sh = am.field_table(am.FR, am.SHOUP_MUL)
    assert len(sh) % 64 == 0
    for w in range(0, len(sh), 64):          # one constant pair per wave of 64 cases
        assert all(c["ops"][1:] == sh[w]["ops"][1:] for c in sh[w:w + 64])
        wv = am.value(sh[w]["ops"][1])
        assert am.value(sh[w]["ops"][2]) == wv * (1 << 261) // am.FR.p      # true constants
    for op, kmax in ((am.IS_ZERO_MOD6, 6), (am.IS_ZERO_MOD10, 10), (am.IS_ZERO_MOD12, 12)):
        ks = {am.value(c["ops"][0]) // am.FQ.p for c in am.field_table(am.FQ, op, nrand=0) if am.value(c["ops"][0]) % am.FQ.p == 0}
        assert ks == set(range(kmax + 3))


def run_g1(hc, op, cases):
    n = len(cases)
    a = np.array([c["a"] for c in cases], dtype=np.uint32)
    b = np.array([c["b"] if c["b"] is not None else [0] for c in cases], dtype=np.uint32)
    neg = np.array([c["neg"] for c in cases], dtype=np.uint8)
    out = np.zeros((n, 36), dtype=np.uint32)
    assert hc.hc_g1_probe(op, ctypes.c_size_t(n), _ptr(a), _ptr(b), _ptr(neg), _ptr(out)) == 0
    return out


@pytest.mark.parametrize("op", range(6), ids=am.G1_NAMES)
def test_g1_op_whole_table_against_the_affine_law(hc, op):
    cases, cover = am.g1_table(op)
    assert len(cases) >= 100
    for c in cases:
        assert am.on_curve(c["A"]) and am.on_curve(c["B"])
    out = run_g1(hc, op, cases)
    for c, o in zip(cases, out):
        am.check_g1_slot(op, am.FORM_CPP, c, o)
    # the exceptional branches met every multiple of p the zero tests can see, and none above the KMAX the code passes
    for key, seen in cover.items():
        assert seen == am.G1_K_EXPECTED[(op, key)], (am.G1_NAMES[op], key, seen)
        assert max(seen) <= am.G1_KMAX[op][0 if key == "P" else 1]
    if op in am.G1_KMAX:
        assert cover


def test_g1_model_agrees_with_the_oracle():
    """second opinion on the affine formulas of the model (the expectation itself never calls the oracle)"""
    import orc
    cases, _ = am.g1_table(am.G1_ADD, nrand=40)
    for c in cases[::7]:
        A, B = c["A"] or (0, 0), c["B"] or (0, 0)
        want = am.aff_add(c["A"], c["B"]) or (0, 0)
        assert tuple(orc.ec_add(0, A, B)) == want


def _chain(hc, op, steps, chains=8, seed=5):
    """`chains` independent chains of `steps` dependent operations: the output slot of one step is the accumulator of the next"""
    import random
    rng = random.Random(seed)
    pts = [am.aff_mul(am.G1_GEN, rng.randrange(1, am.FR.p)) for _ in range(chains)]
    state = [{"A": P, "a": am.slot_of(P, rng.randrange(1, am.Q), (1, 1, 0, 0))} for P in pts]
    for s in range(steps):
        cases = []
        for k, st in enumerate(state):
            if op == am.G1_MADD_SIGNED:      # alternating signs and a repeated point: + Q, - Q, + Q ... with Q == the start point now and then
                B = pts[k] if s % 5 == 0 else pts[(k + 1) % chains]
                cases.append({"cls": "chain step %d" % s, "a": st["a"], "b": am.affine_limbs(B), "neg": s & 1, "A": st["A"], "B": B})
            else:
                cases.append({"cls": "chain step %d" % s, "a": st["a"], "b": None, "neg": 0, "A": st["A"], "B": None})
        yield cases
        out = run_g1(hc, op, cases)
        for c, o in zip(cases, out):
            am.check_g1_slot(op, am.FORM_CPP, c, o)
        state = [{"A": am.g1_expected(op, c), "a": [int(x) for x in o]} for c, o in zip(cases, out)]


def test_g1_chains_feed_the_output_back(hc):
    """the representations the code itself produces: 32 signed mixed additions, 17 doublings, each result the next accumulator"""
    assert sum(1 for _ in _chain(hc, am.G1_MADD_SIGNED, 32)) == 32
    assert sum(1 for _ in _chain(hc, am.G1_DBL, 17)) == 17
