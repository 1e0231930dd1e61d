"""FastStark without a GPU: the model (tests/stark_model.py) runs the reference's own test_fast_stark, reproduces the golden vectors,
checks the two facts the device code relies on (the root-by-root floor quotient equals (tp - interpolant) / zerofier whether or not
the division is exact; fast_coset_divide of the transition polynomials is an exact division), and pins mzk_stark_plan of the BUILT
library -- host-only arithmetic -- against the model's numbers and error codes."""
import json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pytest
import mpoly_model as mm
import stark_model as sm

FR, M128 = 0, 1
P = mm.M128_P
E_ARG, E_NOT_POW2, E_LENGTH = -1, -2, -5


@pytest.fixture(scope="module")
def rescue():
    with open(os.path.join(HERE, "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    st = sm.FastStark(P, mm.M128_GEN, mm.m128_root(9), mm.m128_root(7), 4, 2, rp.m, rp.n + 1, 2)
    return rp, st, rp.transition_constraints(st.omicron), st.preprocess()[2]


def test_reference_parameters(rescue):
    rp, st, air, _ = rescue
    d = sm.plan(P, 4, 2, rp.m, rp.n + 1, 2, air, [(0, 1, 0), (rp.n, 0, 5)])
    assert (rp.m, rp.n) == (2, 27)
    assert (d["num_randomizers"], d["randomized_trace_length"], d["omicron_domain_length"], d["fri_domain_length"]) == (8, 36, 128, 512)
    assert d["transition_quotient_degree_bounds"] == [78, 78] and d["max_degree"] == 127 and d["randomizer_length"] == 128
    assert d["boundary_counts"] == [1, 1] and d["boundary_quotient_degree_bounds"] == [34, 34] and d["boundary_shifts"] == [93, 93]
    assert (d["fri_num_rounds"], d["fri_last_length"], d["num_indices"], d["n_weights"]) == (6, 16, 8, 9)
    assert (st.olen, st.flen) == (128, 512)


def test_fast_stark_hash_chain_accepts_true_and_rejects_false_outputs(rescue):
    """test_fast_stark of the reference (fast_stark.rs:618-): a Rescue-Prime chain from 123456789, 10 links, each proved for its output and
    for output + 1"""
    rp, st, air, tz_root = rescue
    rnd = random.Random(1)
    out = 123456789
    tz = st.transition_zerofier()
    for link in range(10):
        tr = rp.trace(out)
        out = tr[-1][0]
        for claimed, expected in ((out, True), ((out + 1) % P, "combination")):
            trace = [list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(st.nr)]
            boundary = [(0, 1, 0), (rp.n, 0, claimed)]
            pr = st.prove(trace, boundary, air, [rnd.randrange(P) for _ in range(128)])
            dbg = pr["_debug"]
            assert st.verify(pr, air, boundary, tz_root) == expected, (link, claimed == out)
            assert dbg["transition_zerofier_root"] == tz_root
            # the floor quotient by successive roots is the reference's (tp - I) / Z, exact division or not
            assert dbg["boundary_exact"] == (claimed == out)
            assert [sm.div_roots(tp, z, P) for tp, z in zip(dbg["trace_polynomials"], dbg["boundary_roots"])] == dbg["boundary_quotients"]
            # the transition polynomials vanish on the cycle: the coset division is the exact quotient, of the planned length
            for tp, q in zip(dbg["transition_polynomials"], dbg["transition_quotients"]):
                assert sm.pdivmod(tp, tz, P) == (mm.trim(q), [])
                assert len(q) <= 78 + 1
            assert len(dbg["combination"]) == 128 and len(dbg["indices"]) == 8
            assert dbg["indices"] == sorted(dbg["indices"]) and pr["fri"]["top_level_indices"] == sorted(pr["fri"]["top_level_indices"])


def test_verifier_rejects_a_tampered_proof(rescue):
    rp, st, air, tz_root = rescue
    rnd = random.Random(2)
    tr = rp.trace(123456789)
    boundary = [(0, 1, 0), (rp.n, 0, tr[-1][0])]
    pr = st.prove([list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(st.nr)], boundary, air,
                  [rnd.randrange(P) for _ in range(128)])
    assert st.verify(pr, air, boundary, tz_root) is True
    for key, want in (("bqc_points", "bqc path"), ("rdc_points", "rdc path"), ("tzc_points", "tzc path")):
        bad = dict(pr)
        bad[key] = [(pr[key][0] + 1) % P] + pr[key][1:]
        assert st.verify(bad, air, boundary, tz_root) == want
    for key, want in (("bqc_paths", "bqc path"), ("rdc_paths", "rdc path"), ("tzc_paths", "tzc path")):
        bad = dict(pr)
        flipped = bytes([pr[key][0][1][0] ^ 1]) + pr[key][0][1][1:]
        bad[key] = [[pr[key][0][0], flipped] + pr[key][0][2:]] + pr[key][1:]
        assert st.verify(bad, air, boundary, tz_root) == want
    bad = dict(pr)
    bad["rdc_root"] = bytes([pr["rdc_root"][0] ^ 1]) + pr["rdc_root"][1:]
    assert st.verify(bad, air, boundary, tz_root) is not True
    bad = dict(pr)
    bad["fri"] = dict(pr["fri"], last_codeword=[(pr["fri"]["last_codeword"][0] + 1) % P] + pr["fri"]["last_codeword"][1:])
    assert st.verify(bad, air, boundary, tz_root) == "fri"
    assert st.verify(pr, air, boundary, bytes(32)) == "tzc path"


def test_fast_coset_divide_model_is_literal():
    """inexact division: the reference's quotient codeword is not a polynomial's, so the result differs from long division -- the model
    follows ntt.rs, not the algebra; and the degree < 8 branch is plain long division"""
    rnd = random.Random(3)
    lhs, rhs = [rnd.randrange(P) for _ in range(40)], [rnd.randrange(P) for _ in range(12)]
    root = mm.m128_root(8)
    exact = mm.pmul(lhs, rhs, P)
    assert sm.fast_coset_divide(exact, rhs, mm.M128_GEN, root, 256, P) == lhs
    got = sm.fast_coset_divide(lhs, rhs, mm.M128_GEN, root, 256, P)
    assert len(got) == 40 - 12 + 1 and got != sm.pdivmod(lhs, rhs, P)[0]
    assert sm.fast_coset_divide(lhs[:8], rhs[:3], mm.M128_GEN, root, 256, P) == sm.pdivmod(lhs[:8], rhs[:3], P)[0]


def test_golden_vectors_reproduce(rescue):
    rp, st, air, tz_root = rescue
    with open(os.path.join(HERE, "golden", "stark_vectors.json")) as f:
        gold = json.load(f)
    assert gold["transition_zerofier_root"] == tz_root.hex() and len(gold["cases"]) >= 4
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_stark as mg
    full = 0
    for case in gold["cases"]:
        tr = rp.trace(int(case["input"]))
        claimed = int(case["claimed_output"])
        boundary = [(0, 1, 0), (rp.n, 0, claimed)]
        trace = [list(r) for r in tr] + [[int(v) for v in row] for row in case["random_rows"]]
        pr = st.prove(trace, boundary, air, [int(v) for v in case["randomizer"]])
        assert sm.proof_digest(pr) == case["digest"], case["name"]
        assert [r.hex() for r in pr["bqc_roots"]] == case["bqc_roots"] and pr["rdc_root"].hex() == case["rdc_root"]
        assert pr["_debug"]["indices"] == case["indices"] and pr["_debug"]["boundary_exact"] == case["boundary_exact"] == (claimed == tr[-1][0])
        if "proof" in case:
            assert mg.render(pr) == case["proof"]
            full += 1
    assert full == 1


# ---- mzk_stark_plan of the built library (host only) ----------------------------------------------------------------------------------
def two_register_air():
    """next0 - prev0^2 - prev1, next1 - prev0 prev1 - X over (X, prev0, prev1, next0, next1)"""
    return [[(1, (0, 0, 0, 1, 0)), (P - 1, (0, 2, 0, 0, 0)), (P - 1, (0, 0, 1, 0, 0))],
            [(1, (0, 0, 0, 0, 1)), (P - 1, (0, 1, 1, 0, 0)), (P - 1, (1, 0, 0, 0, 0))]]


def lib_plan(mz, fid, e, t, m, cycles, deg, cons, boundary):
    return mz.stark_plan(fid, e, t, m, cycles, deg, cons, boundary)


def test_library_exports_the_new_entry_points():
    import myzkp_amd as mz
    names = mz.exported_symbols()
    for n in ("mzk_poly_div_roots", "mzk_poly_div_roots_dev", "mzk_fast_coset_divide_batch_dev", "mzk_stark_plan", "mzk_stark_proof_layout", "mzk_stark_new",
              "mzk_stark_free", "mzk_stark_prove", "mzk_stark_prove_dev", "mzk_stark_transition_zerofier_root", "mzk_stark_dims_of"):
        assert n in names


def test_stark_plan_matches_the_model(rescue):
    import myzkp_amd as mz
    rp, st, air, _ = rescue
    cons = [mm.terms_of(a) for a in air]
    boundary = [(0, 1, 0), (rp.n, 0, 5)]
    assert lib_plan(mz, M128, 4, 2, 2, 28, 2, cons, boundary) == sm.plan(P, 4, 2, 2, 28, 2, cons, boundary)
    air2 = two_register_air()
    for T, olen, flen in ((20, 64, 256), (2000, 1 << 13, 1 << 15), (30000, 1 << 16, 1 << 18), (120000, 1 << 18, 1 << 20)):
        checks = 2 if T == 20 else 17
        b = [(0, 0, 3), (0, 1, 4), (T - 1, 0, 9)]
        d = lib_plan(mz, M128, 4, checks, 2, T, 2, air2, b)
        assert d == sm.plan(P, 4, checks, 2, T, 2, air2, b)
        assert (d["omicron_domain_length"], d["fri_domain_length"], d["boundary_counts"]) == (olen, flen, [2, 1])
    assert lib_plan(mz, FR, 8, 3, 2, 50, 2, air2, [(0, 0, 1)]) == sm.plan(mm.FR_P, 8, 3, 2, 50, 2, air2, [(0, 0, 1)])
    rnd = random.Random(9)
    for _ in range(300):
        m = rnd.randrange(0, 4)
        nv = 1 + 2 * m
        cons = [[(1, tuple(rnd.choice((0, 0, 0, 1, 1, 2, 3, 7)) for _ in range(nv))) for _ in range(rnd.randrange(0, 5))] for _ in range(rnd.randrange(1, 5))]
        args = (rnd.choice((1, 2, 4, 8, 16)), rnd.randrange(0, 20), m, rnd.randrange(1, 400), rnd.randrange(0, 4), cons,
                [(rnd.randrange(500), rnd.randrange(0, m + 2), 0) for _ in range(rnd.randrange(0, 6))])
        for fid, p in ((FR, mm.FR_P), (M128, P)):
            try:
                want = sm.plan(p, *args)
            except sm.PlanError as e:
                with pytest.raises(mz.MzkError) as got:
                    lib_plan(mz, fid, *args)
                assert got.value.code == e.code, (args, str(e))
            else:
                assert lib_plan(mz, fid, *args) == want, args


def test_stark_plan_error_codes():
    import ctypes
    import myzkp_amd as mz
    air2 = two_register_air()
    b = [(0, 0, 3), (0, 1, 4), (19, 0, 9)]

    def code(*a, **kw):
        with pytest.raises(mz.MzkError) as e:
            lib_plan(mz, *a, **kw)
        return e.value.code

    assert lib_plan(mz, M128, 4, 2, 2, 20, 2, air2, b)["max_degree"] == 63
    assert code(2, 4, 2, 2, 20, 2, air2, b) == E_ARG                                # Fq is not a STARK field
    assert code(M128, 3, 2, 2, 20, 2, air2, b) == E_NOT_POW2
    assert code(M128, 0, 2, 2, 20, 2, air2, b) == E_NOT_POW2
    assert code(M128, 4, 2, 2, 20, 2, [], b) == E_ARG                               # max of no quotient bounds
    assert code(M128, 4, 2, 2, 20, 2, [air2[0]] * 17, b) == E_ARG
    assert code(M128, 4, 2, 4, 20, 2, [[(1, (0,) * 9)]], b) == E_ARG                # nine variables
    assert code(M128, 4, 2, 2, 0, 2, air2, b) == E_LENGTH                           # original_trace_length - 1
    assert code(M128, 4, 2, 2, 20, 2, [[(1, (5, 0, 0, 0, 0))]], b) == E_LENGTH      # degree bound 5 below the zerofier's 19
    assert code(M128, 4, 2, 2, 20, 2, air2, [(0, 0, 0)] * 28) == E_LENGTH           # 28 boundary roots, trace degree 27
    assert code(M128, 4, 2, 2, 20, 2, [[(1, (0, 1, 0, 0, 0))]], b) == E_LENGTH      # max_degree 15 below the boundary bounds
    assert code(M128, 4, 2, 2, 1 << 30, 2, air2, b) == E_LENGTH                     # FRI domain 2^34
    assert code(FR, 4, 2, 2, 1 << 26, 2, air2, b) == E_LENGTH                       # 2^30 above Fr's 2^28
    assert code(M128, 4, 1 << 62, 2, 20, 2, air2, b) == E_LENGTH                    # 4 * checks overflows
    assert code(M128, 64, 0, 2, 1, 1, [[(1, (0, 0, 0, 0, 0))]], []) == E_LENGTH     # FRI domain 128 = 2 * expansion: one round
    assert lib_plan(mz, M128, 4, 2, 2, 20, 2, air2, [(0, 7, 1)] + b)["boundary_counts"] == [2, 1]   # register 7 does not exist: ignored
    # max_degree of a zero quotient bound: format!("{:b}", 0) has one digit
    d = lib_plan(mz, M128, 2, 0, 1, 5, 1, [[(1, (4, 0, 0))]], [(0, 0, 0), (1, 0, 0), (2, 0, 0)])
    assert (d["transition_quotient_degree_bounds"], d["max_degree"], d["boundary_quotient_degree_bounds"], d["boundary_shifts"]) == ([0], 1, [1], [0])
    L = mz.lib()
    sz = ctypes.c_size_t
    assert L.mzk_stark_plan(M128, sz(4), sz(2), sz(2), sz(20), sz(2), None, (sz * 2)(0, 0), sz(1), None, None, sz(0), None) == E_ARG
    dims = mz.StarkDims()
    assert L.mzk_stark_plan(M128, sz(4), sz(2), sz(2), sz(20), sz(2), None, (sz * 2)(0, 1), sz(1), None, None, sz(0), ctypes.byref(dims)) == E_ARG
    assert L.mzk_stark_plan(M128, sz(4), sz(2), sz(2), sz(20), sz(2), None, None, sz(1), None, None, sz(0), ctypes.byref(dims)) == E_ARG


def test_rust_struct_of_the_plan_matches_the_header_and_the_python_binding():
    """include/mzk_ffi.rs declares mzk_stark_dims as #[repr(C)]: the same fields, in the same order and of the same lengths, as the
    ctypes mirror the plan tests above go through"""
    import ctypes
    import myzkp_amd as mz
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import gen_rust_ffi as g
    (name, fields), = g.c_structs()
    assert name == "mzk_stark_dims"
    assert [(f, k) for f, k in fields] == [(f, None if t is ctypes.c_uint64 else t._length_) for f, t in mz.StarkDims._fields_]
    assert ctypes.sizeof(mz.StarkDims) == 8 * sum(k or 1 for _, k in fields)
    rs = open(os.path.join(os.path.dirname(HERE), "include", "mzk_ffi.rs")).read()
    assert "pub struct mzk_stark_dims {" in rs and "pub transition_shifts: [u64; 16]," in rs and "out: *mut mzk_stark_dims" in rs


def test_stark_proof_layout_matches_the_model(rescue):
    import ctypes
    import myzkp_amd as mz
    import fri_prove_model as fm
    rp, st, air, _ = rescue
    cons = [mm.terms_of(a) for a in air]
    d = mz.stark_plan(M128, 4, 2, 2, 28, 2, cons, [(0, 1, 0), (27, 0, 5)])
    sec, total = mz.stark_proof_layout(M128, d)
    assert (sec, total) == sm.proof_layout(2, d)
    assert list(sec) == list(sm.STARK_SECTIONS) and sec["status"] == (0, 8) and sec["fri"] == (8, fm.layout(2, 512, 4, 2)[2])
    assert sec["indices"][1] == 64 and sec["bqc_roots"][1] == 64 and sec["bqc_points"][1] == 16 * 2 * 8 and sec["tzc_paths"][1] == 48 * 8 * 9
    assert sec["path_lens"][1] == 8 * 4 * 8 * 9 and total == sec["path_lens"][0] + sec["path_lens"][1]
    air2 = two_register_air()
    for fid, limbs, p in ((M128, 2, P), (FR, 4, mm.FR_P)):
        for T, checks in ((20, 2), (2000, 17), (30000, 17), (120000, 17), (50, 3)):
            d = mz.stark_plan(fid, 4, checks, 2, T, 2, air2, [(0, 0, 3), (T - 1, 0, 9)])
            assert mz.stark_proof_layout(fid, d) == sm.proof_layout(limbs, d)
    L = mz.lib()
    total = ctypes.c_uint64()
    dims = mz.StarkDims()
    assert L.mzk_stark_proof_layout(None, M128, None, None, ctypes.byref(total)) == E_ARG
    assert L.mzk_stark_proof_layout(ctypes.byref(dims), 2, None, None, ctypes.byref(total)) == E_ARG        # Fq
    assert L.mzk_stark_proof_layout(ctypes.byref(dims), M128, None, None, ctypes.byref(total)) == E_LENGTH  # dims never planned
    assert L.mzk_stark_proof_layout(ctypes.byref(mz._lib._stark_dims_struct(d)), M128, None, None, None) == 0
