"""The model of evaluate_symbolic and of the weighted combination (tests/mpoly_model.py) against the reference's own tests and the figures
of the Rescue-Prime AIR, the golden vectors against the model, and the host plan of the built library (mzk_mpoly_compose_plan needs no
GPU)."""
import ctypes, json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import pytest
import mpoly_model as mm

FR, M128 = 0, 1
E_ARG, E_LENGTH = -1, -5


def rescue():
    with open(os.path.join(HERE, "golden", "rescue_prime_m128.json")) as f:
        par = json.load(f)
    return par, mm.RescuePrime(par)


@pytest.mark.parametrize("p", [mm.FR_P, mm.M128_P])
def test_known_answers_of_the_reference(p):
    """mpolynomials.rs:614-688: 2x + 3y at (t + 1, t^2) is 3t^2 + 2t + 2; the constant 5 is [5]"""
    point = [[1, 1], [0, 0, 1]]
    assert mm.evaluate_symbolic({(1, 0): 2, (0, 1): 3}, point, p) == [2, 2, 3]
    assert mm.evaluate_symbolic({(0, 0): 5}, point, p) == [5]
    assert mm.evaluate_symbolic({}, point, p) == []
    # Polynomial::pow: pow(0) is one even for the zero polynomial, a positive power of it is zero
    assert mm.ppow([], 0, p) == [1] and mm.ppow([0, 0], 0, p) == [1] and mm.ppow([], 3, p) == []
    assert mm.evaluate_symbolic({(0, 2): 5, (1, 0): 7}, [[], [1, 1]], p) == [5, 10, 5]
    # lift: sum_i c_i x_index^i over index + 1 variables; zero coefficients leave no term
    assert mm.lift([4, 0, 9], 1, p) == {(0, 0): 4, (0, 2): 9}
    assert mm.evaluate_symbolic(mm.lift([4, 0, 9], 0, p), [[1, 1]], p) == [13, 18, 9]


def test_rescue_prime_air_shape_and_real_trace():
    par, rp = rescue()
    p, om = mm.M128_P, mm.m128_root(7)
    assert pow(om, 128, p) == 1 and pow(om, 64, p) != 1
    air = rp.transition_constraints(om)
    assert [len(a) for a in air] == [272, 272]
    assert [[max(k[i] for k in a) for i in range(5)] for a in air] == [[78, 3, 3, 3, 3]] * 2
    tr = rp.trace(int(par["kats"][0]["input"]))
    assert len(tr) == 28 and tr[-1][0] == int(par["kats"][0]["hash"])
    dom = [pow(om, r, p) for r in range(28)]
    tps = [mm.interpolate(dom, [row[i] for row in tr], p) for i in range(rp.m)]
    assert all(mm.peval(tps[i], dom[r], p) == tr[r][i] for i in range(rp.m) for r in range(28))
    point = [[0, 1]] + tps + [mm.pscale(t, om, p) for t in tps]
    cons = [mm.terms_of(a) for a in air]
    assert mm.degree_bounds(cons, [len(q) for q in point]) == (128, 82, [82, 82])          # D = 81
    for a in air:
        tpoly = mm.evaluate_symbolic(a, point, p)
        assert len(tpoly) == 82
        assert all(mm.peval(tpoly, dom[r], p) == 0 for r in range(27)) and mm.peval(tpoly, dom[27], p) != 0


def test_rescue_prime_air_on_randomized_lengths_term_by_term_and_in_evaluation_form():
    par, rp = rescue()
    p, om = mm.M128_P, mm.m128_root(7)
    air = rp.transition_constraints(om)
    rnd = random.Random(11)
    point = [[0, 1]] + [[rnd.randrange(p) for _ in range(36)] for _ in range(4)]
    cons = [mm.terms_of(a) for a in air]
    n, smin, bounds = mm.degree_bounds(cons, [len(q) for q in point])
    assert (n, smin, bounds) == (128, 106, [106, 106])                                       # D = 105
    for a, terms in zip(air, cons):
        want = mm.evaluate_symbolic(a, point, p)
        assert len(want) == 106 and mm.compose_terms(terms, point, p) == want
        # evaluation form: the values over the subgroup of order N, interpolated back (an inverse DFT written out)
        ev = [[mm.peval(q, pow(om, j, p), p) for q in point] for j in range(n)]
        vals = []
        for j in range(n):
            acc = 0
            for c, k in terms:
                t = c
                for x, e in zip(ev[j], k):
                    t = t * pow(x, e, p) % p
                acc = (acc + t) % p
            vals.append(acc)
        ninv, ominv = pow(n, -1, p), pow(om, -1, p)
        back = [sum(v * pow(ominv, i * j, p) for j, v in enumerate(vals)) * ninv % p for i in range(n)]
        assert mm.trim(back) == want


@pytest.mark.parametrize("p", [mm.FR_P, mm.M128_P])
def test_lincomb_model_against_the_literal_polynomial_arithmetic(p):
    """fast_stark.rs:301-326: combination += [w_i] * term_i, the terms being every quotient once plain and once times x.pow(shift)"""
    rnd = random.Random(3)
    quot = [[rnd.randrange(p) for _ in range(n)] for n in (9, 14, 1, 6)]
    polys, shifts = [[rnd.randrange(p) for _ in range(16)]], [0]
    for q in quot:
        polys += [q, q]
        shifts += [0, 16 - len(q)]
    weights = [rnd.randrange(p) for _ in polys]
    want = mm.lincomb_reference(polys, weights, shifts, p)
    assert len(want) == 16 and mm.lincomb(polys, weights, shifts, p) == want
    assert mm.lincomb([quot[0], quot[0]], [5, p - 5], [3, 3], p) == mm.lincomb_reference([quot[0], quot[0]], [5, p - 5], [3, 3], p) == []
    assert mm.lincomb([quot[0]], [0], [2], p) == mm.lincomb_reference([quot[0]], [0], [2], p) == []
    assert mm.lincomb([], [], [], p) == []


def test_golden_vectors_are_what_the_generator_writes():
    with open(os.path.join(HERE, "golden", "mpoly_vectors.json")) as f:
        gold = json.load(f)
    assert os.path.getsize(os.path.join(HERE, "golden", "mpoly_vectors.json")) < (1 << 20)
    for case in gold["compose"]:
        p = mm.FR_P if case["field"] == FR else mm.M128_P
        cons = [[(int(c), tuple(k)) for c, k in terms] for terms in case["constraints"]]
        point = [[int(v) for v in q] for q in case["point"]]
        assert [mm.compose_terms(t, point, p) for t in cons] == [[int(v) for v in r] for r in case["expected"]], case["name"]
    names = [c["name"] for c in gold["compose"]]
    assert gold["compose"][names.index("2x+3y at (t+1, t^2)")]["expected"] == [["2", "2", "3"]]
    assert gold["compose"][names.index("x1 - x2 at (p, p)")]["expected"] == [[]]
    for case in gold["lincomb"]:
        p = mm.FR_P if case["field"] == FR else mm.M128_P
        polys = [[int(v) for v in q] for q in case["polys"]]
        assert mm.lincomb(polys, [int(w) for w in case["weights"]], case["shifts"], p) == [int(v) for v in case["expected"]], case["name"]


# ---- the host plan of the built library ---------------------------------------------------------------------------------------------------
def raw_plan(L, fid, exps, toff, nc, nv, poff, want_bounds=True):
    n, smin = ctypes.c_size_t(123), ctypes.c_size_t(456)
    bounds = (ctypes.c_size_t * max(nc, 1))()
    e = None if exps is None else np.ascontiguousarray(np.array(exps, dtype=np.uint32)).ctypes.data_as(ctypes.c_void_p)
    A = lambda v: None if v is None else (ctypes.c_size_t * len(v))(*v)
    rc = L.mzk_mpoly_compose_plan(fid, e, A(toff), ctypes.c_size_t(nc), ctypes.c_size_t(nv), A(poff), ctypes.byref(n), ctypes.byref(smin),
                                  bounds if want_bounds else None)
    return rc, n.value, smin.value, [int(bounds[a]) for a in range(nc)]


def test_compose_plan_of_the_built_library():
    """needs no GPU: mzk_mpoly_compose_plan is host arithmetic.  N and the bounds of the Rescue-Prime AIR, the conventions, the error codes."""
    import myzkp_amd as mz
    assert "mzk_mpoly_compose_plan" in mz.exported_symbols() and "mzk_poly_lincomb_dev" in mz.exported_symbols()
    par, rp = rescue()
    cons = [mm.terms_of(a) for a in rp.transition_constraints(mm.m128_root(7))]
    assert mz.mpoly_compose_plan(M128, cons, [2, 28, 28, 28, 28]) == (128, 82, [82, 82])
    assert mz.mpoly_compose_plan(M128, cons, [2, 36, 36, 36, 36]) == (128, 106, [106, 106])
    assert mz.mpoly_compose_plan(M128, cons[:1], [2, 36, 36, 36, 36]) == (128, 106, [106])
    rnd = random.Random(2)
    for fid in (FR, M128):
        for _ in range(20):
            nv = rnd.randrange(0, 6)
            lens = [rnd.randrange(0, 40) for _ in range(nv)]
            c = [[(1, tuple(rnd.randrange(5) for _ in range(nv))) for _ in range(rnd.randrange(0, 6))] for _ in range(rnd.randrange(0, 4))]
            assert mz.mpoly_compose_plan(fid, c, lens) == mm.degree_bounds(c, lens)
    L = mz.lib()
    # constants only: N = 1; an empty constraint: bound 0; a positive exponent on an empty polynomial does not count; trailing zeros do
    assert raw_plan(L, M128, [[0, 0], [0, 0]], [0, 2], 1, 2, [0, 5, 9])[:3] == (0, 1, 1)
    assert raw_plan(L, M128, [[1, 2]], [0, 0, 1], 2, 2, [0, 5, 9]) == (0, 16, 11, [0, 11])
    assert raw_plan(L, M128, [[7, 0], [0, 2]], [0, 2], 1, 2, [0, 0, 4]) == (0, 8, 7, [7])
    assert raw_plan(L, M128, [[7, 0]], [0, 1], 1, 2, [0, 0, 4]) == (0, 1, 0, [0])
    assert raw_plan(L, M128, [[1, 2]], [0, 1], 1, 2, [3, 8, 12], want_bounds=False)[:3] == (0, 16, 11)           # offsets need not start at 0
    assert raw_plan(L, M128, None, None, 0, 2, None)[:3] == (0, 0, 0)
    # errors
    assert raw_plan(L, 2, [[1, 2]], [0, 1], 1, 2, [0, 5, 9])[0] == E_ARG                                         # MZK_FIELD_FQ
    assert raw_plan(L, FR, [[1] * 9], [0, 1], 1, 9, list(range(0, 20, 2)))[0] == E_ARG                           # n_vars above MZK_MPOLY_MAX_VARS = 8
    assert raw_plan(L, FR, [[1] * 8], [0, 1], 1, 8, list(range(0, 18, 2)))[:3] == (0, 16, 9)
    assert raw_plan(L, FR, [[1, 2]], None, 1, 2, [0, 5, 9])[0] == E_ARG and raw_plan(L, FR, [[1, 2]], [0, 1], 1, 2, None)[0] == E_ARG
    assert raw_plan(L, FR, None, [0, 1], 1, 2, [0, 5, 9])[0] == E_ARG
    assert L.mzk_mpoly_compose_plan(FR, None, None, ctypes.c_size_t(0), ctypes.c_size_t(0), None, None, None, None) == E_ARG
    assert raw_plan(L, FR, [[1, 2]], [1, 0], 1, 2, [0, 5, 9])[0] == E_LENGTH and raw_plan(L, FR, [[1, 2]], [0, 1], 1, 2, [0, 9, 5])[0] == E_LENGTH
    # the size limit of transforms: 2^28 over Fr, 2^32 over M128
    assert raw_plan(L, FR, [[1]], [0, 1], 1, 1, [0, 1 << 28])[:3] == (0, 1 << 28, 1 << 28)
    assert raw_plan(L, FR, [[1]], [0, 1], 1, 1, [0, (1 << 28) + 1])[0] == E_LENGTH
    assert raw_plan(L, M128, [[1]], [0, 1], 1, 1, [0, (1 << 28) + 1])[:3] == (0, 1 << 29, (1 << 28) + 1)
    assert raw_plan(L, M128, [[2]], [0, 1], 1, 1, [0, (1 << 31) + 2])[0] == E_LENGTH
    # a degree bound that overflows 64 bits is reported, not wrapped
    assert raw_plan(L, M128, [[0xFFFFFFFF]], [0, 1], 1, 1, [0, 1 << 40])[0] == E_LENGTH
    assert raw_plan(L, M128, [[0xFFFFFFFF, 0xFFFFFFFF]], [0, 1], 1, 2, [0, 1 << 33, 1 << 34])[0] == E_LENGTH
    assert b"overflow" in L.mzk_last_error()
