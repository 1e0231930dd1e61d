"""evaluate_symbolic on the GPU (mzk_mpoly_compose*) and the weighted combination (mzk_poly_lincomb*): bit-exact against the model
(tests/mpoly_model.py) and the golden vectors, every documented error code, and large sizes by exact properties -- values at fixed
points by big-integer Horner, the degree bound, and exact divisibility of a real trace's transition polynomial by its zerofier."""
import ctypes, json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import pytest
import mpoly_model as mm

pytestmark = pytest.mark.gpu
FR, M128 = 0, 1
PRIME = {FR: mm.FR_P, M128: mm.M128_P}
NL = {FR: 4, M128: 2}
E_ARG, E_LENGTH, E_RANGE = -1, -5, -6


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as mz
    mz.init(0)
    return mz


def limbs(fid, vals):
    a = np.zeros((len(vals), NL[fid]), dtype=np.uint64)
    for j in range(NL[fid]):
        a[:, j] = np.array([(int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64) if len(vals) else 0
    return a


def ints(a):
    a = np.asarray(a, dtype=np.uint64)
    a = a.reshape(-1, a.shape[-1])
    acc = np.zeros(a.shape[0], dtype=object)
    for j in range(a.shape[1]):
        acc = acc + (a[:, j].astype(object) << (64 * j))
    return [int(v) for v in acc]


def compose(mz, fid, constraints, point, **kw):
    return [ints(r) for r in mz.mpoly_compose(fid, constraints, [limbs(fid, q) for q in point], **kw)]


def model(fid, constraints, point):
    return [mm.compose_terms(t, point, PRIME[fid]) for t in constraints]


def rand_poly(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


def rescue_air():
    with open(os.path.join(HERE, "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    return rp, [mm.terms_of(a) for a in rp.transition_constraints(mm.m128_root(7))]


# ---- bit-identical to the golden vectors and the model ------------------------------------------------------------------------------
def test_golden_vectors(mz):
    with open(os.path.join(HERE, "golden", "mpoly_vectors.json")) as f:
        gold = json.load(f)
    assert len(gold["compose"]) >= 12 and len(gold["lincomb"]) >= 4
    for case in gold["compose"]:
        cons = [[(int(c), tuple(k)) for c, k in terms] for terms in case["constraints"]]
        point = [[int(v) for v in q] for q in case["point"]]
        assert compose(mz, case["field"], cons, point) == [[int(v) for v in r] for r in case["expected"]], case["name"]
    for case in gold["lincomb"]:
        fid = case["field"]
        got = mz.poly_lincomb(fid, [limbs(fid, [int(v) for v in q]) for q in case["polys"]], [int(w) for w in case["weights"]], case["shifts"])
        assert ints(got) == [int(v) for v in case["expected"]], case["name"]


@pytest.mark.parametrize("fid", [FR, M128])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sparse_constraints_match_model(mz, fid, seed):
    rnd = random.Random(100 * fid + seed)
    p = PRIME[fid]
    nv = rnd.randrange(1, 6)
    point = [rand_poly(rnd, p, rnd.randrange(1, 12)) for _ in range(nv)]
    cons = []
    for _ in range(rnd.randrange(1, 5)):
        cons.append([(rnd.randrange(p), tuple(rnd.choice((0, 0, 1, 2, 3, 4, 5, 7, 11)) if rnd.random() < 0.6 else 0 for _ in range(nv)))
                     for _ in range(rnd.randrange(1, 30))])
    want = model(fid, cons, point)
    assert compose(mz, fid, cons, point) == want
    n, smin, bounds = mz.mpoly_compose_plan(fid, cons, [len(q) for q in point])
    assert (n, smin, bounds) == mm.degree_bounds(cons, [len(q) for q in point])
    assert all(len(w) <= b for w, b in zip(want, bounds))


def test_rescue_prime_constraints_together_and_alone(mz):
    """both transition constraints of the Rescue-Prime AIR (2 x 272 terms, exponents up to 78) over random trace polynomials of the
    randomized length: equal to the model term by term, and one call for both equals two single calls"""
    rp, cons = rescue_air()
    assert [len(t) for t in cons] == [272, 272]
    rnd = random.Random(7)
    p = mm.M128_P
    point = [[0, 1]] + [rand_poly(rnd, p, 36) for _ in range(4)]
    assert mz.mpoly_compose_plan(M128, cons, [len(q) for q in point]) == (128, 106, [106, 106])
    both = compose(mz, M128, cons, point)
    assert [len(r) for r in both] == [106, 106]
    assert both == model(M128, cons, point)
    assert [compose(mz, M128, [c], point)[0] for c in cons] == both


def test_rescue_prime_real_trace_vanishes_on_the_cycle(mz):
    rp, cons = rescue_air()
    p, om = mm.M128_P, mm.m128_root(7)
    tr = rp.trace(1)
    dom = [pow(om, r, p) for r in range(len(tr))]
    tps = [mm.interpolate(dom, [row[i] for row in tr], p) for i in range(rp.m)]
    point = [[0, 1]] + tps + [mm.pscale(t, om, p) for t in tps]
    got = compose(mz, M128, cons, point)
    assert [len(r) for r in got] == [82, 82]
    for r_ in got:
        assert all(mm.peval(r_, dom[r], p) == 0 for r in range(27)) and mm.peval(r_, dom[27], p) != 0


@pytest.mark.parametrize("fid", [FR, M128])
def test_edge_cases(mz, fid):
    p = PRIME[fid]
    rnd = random.Random(40 + fid)
    q, r = rand_poly(rnd, p, 6), rand_poly(rnd, p, 4)
    # a zero polynomial in the point: pow(0) is one, a positive power is zero -- empty and all-zero alike
    for zero in ([], [0, 0, 0]):
        cons = [[(5, (0, 2)), (7, (1, 0))], [(5, (1, 1)), (9, (2, 0))]]
        want = model(fid, cons, [zero, q])
        assert want == [mm.trim([5 * v % p for v in mm.pmul(q, q, p)]), []]
        assert compose(mz, fid, cons, [zero, q]) == want
    # an empty constraint next to a full one; a zero coefficient; duplicate exponent rows add up
    cons = [[], [(0, (3, 1)), (4, (1, 1))], [(2, (1, 2)), (3, (1, 2)), (p - 5, (1, 2)), (1, (0, 0))], [(2, (1, 2)), (3, (1, 2))]]
    got = compose(mz, fid, cons, [q, r])
    assert got == model(fid, cons, [q, r])
    assert got[0] == [] and got[2] == [1] and got[3] == mm.trim([5 * v % p for v in mm.pmul(q, mm.pmul(r, r, p), p)])
    # untrimmed point lengths: a larger bound, the same polynomials
    cons = [[(3, (2, 1)), (1, (0, 3))]]
    assert compose(mz, fid, cons, [q + [0] * 5, r + [0] * 9]) == compose(mz, fid, cons, [q, r]) == model(fid, cons, [q, r])
    assert mz.mpoly_compose_plan(fid, cons, [11, 13])[1] > mz.mpoly_compose_plan(fid, cons, [6, 4])[1]
    # cancellations: everything, and the leading terms only
    cons = [[(1, (1, 0)), (p - 1, (0, 1))]]
    assert compose(mz, fid, cons, [q, q]) == [[]]
    q2 = q[:3] + [(q[3] + 1) % p] + q[4:]
    assert compose(mz, fid, cons, [q, q2]) == [[0, 0, 0, p - 1]]
    # one exponent above 1000 on the point X, beside table-sized ones
    cons = [[(3, (1500, 0)), (2, (1001, 1)), (5, (6, 2)), (1, (4, 0)), (9, (0, 0))]]
    want = [9, 0, 0, 0, 1] + [0] * 1496
    want[1500] = 3
    for i, v in enumerate(r):
        want[1001 + i] = (want[1001 + i] + 2 * v) % p
    for i, v in enumerate(mm.pmul(r, r, p)):
        want[6 + i] = (want[6 + i] + 5 * v) % p
    assert compose(mz, fid, cons, [[0, 1], r]) == [mm.trim(want)]
    # N = 1: constants only, with and without variables; no constraints at all
    assert mz.mpoly_compose_plan(fid, [[(4, (0, 0)), (p - 1, (0, 0))]], [6, 4])[0] == 1
    assert compose(mz, fid, [[(4, (0, 0)), (p - 1, (0, 0))], [(2, (0, 0)), (p - 2, (0, 0))]], [q, r]) == [[3], []]
    assert compose(mz, fid, [[(4, ()), (6, ())]], []) == [[10]]
    assert compose(mz, fid, [], [q, r]) == []


# ---- the device form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [FR, M128])
def test_dev_form_equals_host_form_on_both_streams(mz, fid):
    import torch
    p = PRIME[fid]
    rnd = random.Random(60 + fid)
    point = [rand_poly(rnd, p, n) for n in (300, 17, 0, 256)]
    cons = [[(rnd.randrange(p), (rnd.randrange(5), rnd.randrange(3), rnd.randrange(2), rnd.randrange(4))) for _ in range(40)] for _ in range(3)]
    host = mz.mpoly_compose(fid, cons, [limbs(fid, q) for q in point])
    n, smin, bounds = mz.mpoly_compose_plan(fid, cons, [len(q) for q in point])
    stride = smin + 5
    flat = np.concatenate([limbs(fid, q) for q in point])
    d_in = torch.from_numpy(flat.view(np.int64).reshape(-1).copy()).cuda()
    side = torch.cuda.Stream()
    for stream in (mz.lib().mzk_ctx_stream(0), side.cuda_stream):
        d_out = torch.full((len(cons) * stride * NL[fid],), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        lens = mz.mpoly_compose_dev(fid, cons, d_in.data_ptr(), [len(q) for q in point], d_out.data_ptr(), stride, stream or 0)
        torch.cuda.synchronize()
        rows = d_out.cpu().numpy().view(np.uint64).reshape(len(cons), stride, NL[fid])
        for a in range(len(cons)):
            assert lens[a] == host[a].shape[0]
            assert np.array_equal(rows[a, :lens[a]], host[a]) and not rows[a, lens[a]:].any()


# ---- error codes -----------------------------------------------------------------------------------------------------------------------
def raw_compose(mz, fid, coefs, exps, toff, nc, nv, point, poff, out, stride, lens):
    P_ = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    A = lambda v: None if v is None else (ctypes.c_size_t * len(v))(*v)
    return mz.lib().mzk_mpoly_compose(fid, P_(coefs), P_(exps), A(toff), ctypes.c_size_t(nc), ctypes.c_size_t(nv), P_(point), A(poff), P_(out),
                                      ctypes.c_size_t(stride), lens)


@pytest.mark.parametrize("fid", [FR, M128])
def test_error_codes_leave_the_library_usable(mz, fid):
    p = PRIME[fid]
    good_cons, good_pt = [[(2, (1, 0)), (3, (0, 1))]], [[1, 1], [0, 0, 1]]

    def still_works():
        assert compose(mz, fid, good_cons, good_pt) == [[2, 2, 3]]

    def code_of(fn):
        with pytest.raises(mz.MzkError) as e:
            fn()
        still_works()
        return e.value.code

    still_works()
    assert code_of(lambda: mz.mpoly_compose(2, good_cons, [limbs(FR, q) for q in good_pt])) == E_ARG              # MZK_FIELD_FQ
    assert code_of(lambda: compose(mz, fid, [[(1, (1,) * 9)]], [[1, 1]] * 9)) == E_ARG                            # n_vars above the cap
    assert compose(mz, fid, [[(1, (1,) * 8)]], [[1, 1]] * 8) == [[1, 8, 28, 56, 70, 56, 28, 8, 1]]               # the cap itself works
    assert code_of(lambda: compose(mz, fid, [[(p, (1, 0))]], good_pt)) == E_RANGE                                 # coefficient = p
    assert code_of(lambda: compose(mz, fid, good_cons, [[1, p], [0, 0, 1]])) == E_RANGE                           # point coefficient = p
    assert code_of(lambda: compose(mz, fid, good_cons, good_pt, out_stride=2)) == E_LENGTH                        # out_stride < D + 1
    top = 28 if fid == FR else 32
    assert code_of(lambda: compose(mz, fid, [[(1, ((1 << top) - 1, 2))]], [[1, 1]] * 2, out_stride=4)) == E_LENGTH   # N = 2^(top + 1)
    # raw calls: null pointers and offset arrays that decrease
    coefs, exps = limbs(fid, [2, 3]), np.array([[1, 0], [0, 1]], dtype=np.uint32)
    pt, out, lens = limbs(fid, [1, 1, 0, 0, 1]), np.zeros((3, NL[fid]), dtype=np.uint64), (ctypes.c_size_t * 1)()
    assert raw_compose(mz, fid, coefs, exps, [0, 2], 1, 2, pt, [0, 2, 5], out, 3, lens) == 0 and ints(out) == [2, 2, 3] and lens[0] == 3
    for args in ((None, exps, [0, 2], 1, 2, pt, [0, 2, 5], out, 3, lens), (coefs, None, [0, 2], 1, 2, pt, [0, 2, 5], out, 3, lens),
                 (coefs, exps, None, 1, 2, pt, [0, 2, 5], out, 3, lens), (coefs, exps, [0, 2], 1, 2, None, [0, 2, 5], out, 3, lens),
                 (coefs, exps, [0, 2], 1, 2, pt, None, out, 3, lens), (coefs, exps, [0, 2], 1, 2, pt, [0, 2, 5], None, 3, lens),
                 (coefs, exps, [0, 2], 1, 2, pt, [0, 2, 5], out, 3, None)):
        assert raw_compose(mz, fid, *args) == E_ARG
        still_works()
    assert raw_compose(mz, fid, coefs, exps, [2, 0], 1, 2, pt, [0, 2, 5], out, 3, lens) == E_LENGTH
    assert raw_compose(mz, fid, coefs, exps, [0, 2], 1, 2, pt, [0, 5, 2], out, 3, lens) == E_LENGTH
    still_works()
    # n_constraints == 0: MZK_OK, nothing written
    out[:] = 77
    assert raw_compose(mz, fid, None, None, None, 0, 2, pt, [0, 2, 5], out, 3, None) == 0 and (out == 77).all()
    assert raw_compose(mz, 7, coefs, exps, [0, 2], 1, 2, pt, [0, 2, 5], out, 3, lens) == E_ARG
    # the device form reports the same codes
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    assert code_of(lambda: mz.mpoly_compose_dev(fid, [[(p, (1, 0))]], d.data_ptr(), [2, 3], d.data_ptr(), 3)) == E_RANGE
    assert code_of(lambda: mz.mpoly_compose_dev(fid, good_cons, d.data_ptr(), [2, 3], d.data_ptr(), 2)) == E_LENGTH
    assert code_of(lambda: mz.mpoly_compose_dev(fid, good_cons, 0, [2, 3], 0, 3)) == E_ARG
    # lincomb
    a = limbs(fid, [1, 2, 3])
    assert code_of(lambda: mz.poly_lincomb(2, [limbs(FR, [1, 2, 3])], [1], [0])) == E_ARG
    assert code_of(lambda: mz.poly_lincomb(fid, [a], [p], [0])) == E_RANGE
    assert code_of(lambda: mz.poly_lincomb(fid, [limbs(fid, [1, p])], [1], [0])) == E_RANGE
    assert code_of(lambda: mz.poly_lincomb(fid, [a, a], [1, 1], [0, 4], out_cap=6)) == E_LENGTH
    assert ints(mz.poly_lincomb(fid, [a, a], [1, 1], [0, 4], out_cap=7)) == [1, 2, 3, 0, 1, 2, 3]


def test_workspace_budget(mz):
    """the call lives in the context's grow-only workspace: a budget below its needs releases idle buffers and the result is the same"""
    rnd = random.Random(5)
    p = mm.M128_P
    point = [rand_poly(rnd, p, 2000), rand_poly(rnd, p, 1500)]
    cons = [[(rnd.randrange(p), (rnd.randrange(4), rnd.randrange(4))) for _ in range(20)]]
    want = compose(mz, M128, cons, point)
    held = mz.workspace_bytes()
    assert held > 0
    mz.set_workspace_budget(1 << 16)
    try:
        assert mz.workspace_bytes() < held
        assert compose(mz, M128, cons, point) == want
    finally:
        mz.set_workspace_budget(0)
    assert compose(mz, M128, cons, point) == want


# ---- large sizes by exact properties ---------------------------------------------------------------------------------------------------
def synthetic_air(mz, fid, log_t):
    """s_{r+1} = s_r^3 + k(omicron^r) over the subgroup of order T = 2^log_t: trace polynomial tp (inverse transform of the trace), the
    constraint next - prev^3 - k(X) over the point (X, tp, tp.scale(omicron)) with k a lifted univariate"""
    p, T = PRIME[fid], 1 << log_t
    om = mz.root_of_unity(fid, log_t)
    rnd = random.Random(900 + 10 * fid + log_t)
    k = rand_poly(rnd, p, 6)
    s, x, trace = rnd.randrange(p), 1, []
    for _ in range(T):
        trace.append(s)
        s = (s * s % p * s + mm.peval(k, x, p)) % p
        x = x * om % p
    tp = mz.intt(fid, om, limbs(fid, trace))
    nxt = mz.poly_scale(fid, tp, om)
    cons = [[(1, (0, 0, 1)), (p - 1, (0, 3, 0))] + [((-c) % p, (i, 0, 0)) for i, c in enumerate(k)]]
    return p, T, om, cons, [limbs(fid, [0, 1]), tp, nxt]


@pytest.mark.parametrize("fid,log_t", [(M128, 14), (M128, 18), (FR, 14)])
def test_large_synthetic_air_by_exact_properties(mz, fid, log_t):
    p, T, om, cons, point = synthetic_air(mz, fid, log_t)
    D = 3 * (T - 1)
    n, smin, bounds = mz.mpoly_compose_plan(fid, cons, [q.shape[0] for q in point])
    assert (n, smin, bounds) == (4 * T, D + 1, [D + 1])
    out = mz.mpoly_compose(fid, cons, point)[0]
    # (b) the degree bound
    assert 0 < out.shape[0] <= D + 1
    # (a) values at 8 fixed pseudo-random points, both sides by big-integer Horner
    oi, pi = ints(out), [ints(q) for q in point]
    rnd = random.Random(4242 + log_t)
    for _ in range(8):
        z = rnd.randrange(p)
        ev = [mm.peval(q, z, p) for q in pi]
        want = 0
        for c, ks in cons[0]:
            term = c
            for e, v in zip(ks, ev):
                term = term * pow(v, e, p) % p
            want = (want + term) % p
        assert mm.peval(oi, z, p) == want
    # (c) a real trace: the transition polynomial is divisible by the zerofier of the first T - 1 trace points, exactly
    big = mz.root_of_unity(fid, log_t + 2)
    dom, x = [], 1
    for _ in range(T - 1):
        dom.append(x)
        x = x * om % p
    zf = mz.fast_zerofier(fid, limbs(fid, dom), big, 4 * T)
    assert zf.shape[0] == T and ints(zf[-1:]) == [1]
    q = mz.fast_coset_divide(fid, out, zf, 3 if fid == M128 else 5, big, 4 * T)
    assert q.shape[0] == out.shape[0] - T + 1
    prod = mz.fast_multiply(fid, q, zf, big, 4 * T)
    assert np.array_equal(prod[:out.shape[0]], out) and not prod[out.shape[0]:].any()


# ---- the weighted combination ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [FR, M128])
def test_lincomb_matches_model(mz, fid):
    import torch
    p = PRIME[fid]
    rnd = random.Random(77 + fid)
    quot = [rand_poly(rnd, p, n) for n in (700, 333, 1025, 64)]
    # the reference's term list: the randomizer once, every quotient once plain and once shifted (fast_stark.rs:305-317)
    polys, shifts = [rand_poly(rnd, p, 1100)], [0]
    for q in quot:
        polys += [q, q]
        shifts += [0, 1100 - len(q)]
    weights = rand_poly(rnd, p, len(polys))
    want = mm.lincomb_reference(polys, weights, shifts, p)
    assert want == mm.lincomb(polys, weights, shifts, p)
    arrs = [limbs(fid, q) for q in polys]
    assert ints(mz.poly_lincomb(fid, arrs, weights, shifts)) == want
    # count = 1; a shift that makes the output longer than every input; weights 0 and 1; a cancelling pair
    assert ints(mz.poly_lincomb(fid, arrs[:1], weights[:1], [0])) == mm.lincomb_reference(polys[:1], weights[:1], [0], p)
    assert ints(mz.poly_lincomb(fid, arrs[1:3], [1, 0], [0, 5000])) == mm.trim(polys[1])
    got = ints(mz.poly_lincomb(fid, arrs[1:3], [0, 1], [0, 5000]))
    assert got == [0] * 5000 + mm.trim(polys[1]) and len(got) > max(len(q) for q in polys)
    assert ints(mz.poly_lincomb(fid, arrs[1:3], [3, p - 3], [9, 9])) == []
    assert ints(mz.poly_lincomb(fid, [], [], [])) == []
    # the device form, on the context's stream and on a caller's
    flat = np.concatenate(arrs)
    d_in = torch.from_numpy(flat.view(np.int64).reshape(-1).copy()).cuda()
    cap = 1100 + 13
    side = torch.cuda.Stream()
    for stream in (mz.lib().mzk_ctx_stream(0), side.cuda_stream):
        d_out = torch.full((cap * NL[fid],), -1, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        n = mz.poly_lincomb_dev(fid, d_in.data_ptr(), [len(q) for q in polys], weights, shifts, d_out.data_ptr(), cap, stream or 0)
        torch.cuda.synchronize()
        assert n == len(want) and ints(d_out.cpu().numpy().view(np.uint64).reshape(cap, NL[fid])) == want + [0] * (cap - n)
