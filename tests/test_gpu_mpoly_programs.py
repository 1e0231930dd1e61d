"""mzk_mpoly_compose* at every shape of the term program (mzk_mpoly_plan.h: mp_compile), every size edge of the plan (mp_plan) and with
operands next to the modulus, and mzk_poly_lincomb* at its edges.  Every expectation is computed by tests/mpoly_model.py in Python
integers (compose_terms, degree_bounds, lincomb); every comparison is bit-exact and includes the row lengths; no library result is the
expectation of another.  The shapes are the smallest that reach the code: a program's op depends on an exponent or a gap being 0,
1 .. 3, 4 .. 6 or above, a variable's LDS slots on the largest exponent of the whole call, the grid on N / 64 and the constraint
count."""
import ctypes, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import pytest
import mpoly_model as mm

pytestmark = pytest.mark.gpu
FR, M128 = 0, 1
PRIME = {FR: mm.FR_P, M128: mm.M128_P}
NL = {FR: 4, M128: 2}
FIELDS = pytest.mark.parametrize("fid", [FR, M128])
GUARD = 0x5A5A5A5A5A5A5A5A
GAPS = (0, 1, 2, 3, 4, 5, 6, 7, 9, 64)
LASTS = (0, 1, 3, 4, 6, 7, 100)
REST = (0, 1, 2, 3, 4, 6, 7)
STRIDES = (1, 2, 63, 64, 65, 127, 128, 129, 4096, 4097)


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


def compose(mz, fid, cons, point, **kw):
    return [ints(r) for r in mz.mpoly_compose(fid, cons, [limbs(fid, q) for q in point], **kw)]


def model(fid, cons, point):
    return [mm.compose_terms(t, point, PRIME[fid]) for t in cons]


def check(mz, fid, cons, point):
    """the host form against the model, the plan against degree_bounds; returns the model's rows"""
    want = model(fid, cons, point)
    lens = [len(q) for q in point]
    plan = mm.degree_bounds(cons, lens)
    assert mz.mpoly_compose_plan(fid, cons, lens) == plan
    assert all(len(w) <= b for w, b in zip(want, plan[2]))
    got = compose(mz, fid, cons, point)
    assert [len(r) for r in got] == [len(r) for r in want]
    assert got == want
    return want


def rand_poly(rnd, p, n):
    return [rnd.randrange(p) for _ in range(n)]


def check_dev(mz, fid, cons, point, stride, want):
    """the device form into a buffer filled with a guard pattern: the rows, zeros behind their lengths, the element behind the last row
    untouched, the point unchanged"""
    import torch
    nl, nc = NL[fid], len(cons)
    flat = np.concatenate([limbs(fid, q) for q in point] + [limbs(fid, [7])])       # one element behind the point: never read as a value
    d_in = torch.from_numpy(flat.view(np.int64).reshape(-1).copy()).cuda()
    d_out = torch.full(((nc * stride + 1) * nl,), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    lens = mz.mpoly_compose_dev(fid, cons, d_in.data_ptr(), [len(q) for q in point], d_out.data_ptr(), stride, 0)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    rows = out[:nc * stride * nl].reshape(nc, stride, nl)
    assert lens == [len(w) for w in want]
    for a in range(nc):
        assert ints(rows[a, :lens[a]]) == want[a] and not rows[a, lens[a]:].any(), (stride, a)
    assert (out[nc * stride * nl:] == np.uint64(GUARD)).all()
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64).reshape(-1, nl), flat)


# ---- op classes on the Horner variable -------------------------------------------------------------------------------------------------
def horner_constraints(rnd, p):
    """every (gap, last exponent) pair as a two-term constraint, and ten three-term ones whose second gap walks the same classes"""
    cons = [[(rnd.randrange(1, p), (last + gap,)), (rnd.randrange(1, p), (last,))] for gap in GAPS for last in LASTS]
    for k, gap in enumerate(GAPS):
        last, gap2 = LASTS[k % len(LASTS)], GAPS[(k + 3) % len(GAPS)]
        cons.append([(rnd.randrange(1, p), (last + gap + gap2,)), (rnd.randrange(1, p), (last + gap,)), (rnd.randrange(1, p), (last,))])
    return cons


@FIELDS
def test_every_gap_and_tail_class_on_the_point_x(mz, fid):
    """point X: the coefficient of term (c, e) is read at position e"""
    p = PRIME[fid]
    cons = horner_constraints(random.Random(11 + fid), p)
    assert len(cons) == 80
    want = check(mz, fid, cons, [[0, 1]])
    for terms, row in zip(cons, want):
        flat = [0] * len(row)
        for c, (e,) in terms:
            flat[e] = (flat[e] + c) % p
        assert row == mm.trim(flat)


@FIELDS
def test_every_gap_and_tail_class_on_a_random_line(mz, fid):
    p = PRIME[fid]
    rnd = random.Random(13 + fid)
    check(mz, fid, horner_constraints(rnd, p), [rand_poly(rnd, p, 2)])


@FIELDS
def test_table_depth_one_two_three_alone(mz, fid):
    """the constraints whose largest exponent is 1, 2, 3, each alone in a call: the variable gets that many LDS slots"""
    p = PRIME[fid]
    rnd = random.Random(17 + fid)
    point = [rand_poly(rnd, p, 3)]
    cons = horner_constraints(rnd, p) + [[(rnd.randrange(p), (2,)), (rnd.randrange(p), (1,)), (rnd.randrange(p), (0,))], [(rnd.randrange(p), (2,))]]
    seen = set()
    for terms in cons:
        top = max(k[0] for _, k in terms)
        if 1 <= top <= 3:
            seen.add(top)
            check(mz, fid, [terms], point)
    assert seen == {1, 2, 3}


# ---- the other variables ---------------------------------------------------------------------------------------------------------------
def multivariate_constraint(rnd, p, nv, h):
    """runs over rest monomials with exponents of REST, the Horner variable h with falling exponents 12, 9, 8, 5, 4, 0 inside a run"""
    terms = []
    for r in range(4):
        rest = [REST[(r * 3 + i) % len(REST)] for i in range(nv)]
        for eh in (12, 9, 8, 5, 4, 0)[r % 2::1 + r % 2]:
            k = list(rest)
            k[h] = eh
            terms.append((rnd.randrange(p), tuple(k)))
    rnd.shuffle(terms)
    return terms


@FIELDS
@pytest.mark.parametrize("nv", [2, 3, 4, 5, 6, 7, 8])
def test_horner_variable_first_middle_last(mz, fid, nv):
    """each position alone, and all three in one call: constraints of one call with different Horner variables"""
    p = PRIME[fid]
    rnd = random.Random(100 * nv + fid)
    point = [rand_poly(rnd, p, 2 + (i == 1)) for i in range(nv)]
    cons = [multivariate_constraint(rnd, p, nv, h) for h in sorted({0, nv // 2, nv - 1})]
    want = check(mz, fid, cons, point)
    for terms, row in zip(cons, want):
        assert compose(mz, fid, [terms], point) == [row]


@FIELDS
def test_tie_of_the_largest_exponents_and_full_tables(mz, fid):
    p = PRIME[fid]
    rnd = random.Random(23 + fid)
    c = lambda: rnd.randrange(p)
    point3 = [rand_poly(rnd, p, n) for n in (3, 2, 4)]
    tie = [[(c(), (5, 5, 1)), (c(), (5, 2, 0)), (c(), (3, 5, 1)), (c(), (0, 5, 1)), (c(), (2, 2, 0)), (c(), (5, 5, 5))]]
    check(mz, fid, tie, point3)
    # 8 variables, every one at depth 3: 24 slots, the whole 55 296 bytes of LDS over Fr
    point8 = [rand_poly(rnd, p, 2) for _ in range(8)]
    full = [[(c(), (3,) * 8), (c(), (1, 2, 3, 1, 2, 3, 1, 2)), (c(), (3, 3, 3, 3, 3, 3, 3, 7)), (c(), (0,) * 7 + (3,)), (c(), (0,) * 8)],
            [(c(), (2, 0, 0, 0, 0, 0, 0, 1)), (c(), (3, 0, 0, 0, 0, 0, 0, 1)), (c(), (0, 0, 0, 1, 0, 0, 0, 0))]]
    check(mz, fid, full, point8)


# ---- size edges --------------------------------------------------------------------------------------------------------------------------
def size_edge_calls(rnd, p, smin):
    """three calls whose out_stride_min is smin: a line (above 129: a monomial c X, which keeps the model's powers cheap) to the power
    smin - 1 through POW, a polynomial of smin coefficients to the power 1, a product of two variables; each with a shorter row beside"""
    c = lambda: rnd.randrange(1, p)
    line = rand_poly(rnd, p, 2) if smin <= 129 else [0, c()]
    calls = [([[(c(), (smin - 1,))], [(c(), ((smin - 1) // 2,)), (c(), (0,))]], [line]),
             ([[(c(), (1,))], [(c(), (0,))]], [rand_poly(rnd, p, smin - 1) + [c()]])]
    la, lb = (smin - 2, 3) if smin >= 4 else (smin, 1)
    calls.append(([[(c(), (1, 1)), (c(), (1, 0))], [(c(), (0, 2))]], [rand_poly(rnd, p, la - 1) + [c()], rand_poly(rnd, p, lb - 1) + [c()]]))
    return calls


@FIELDS
@pytest.mark.parametrize("smin", STRIDES)
def test_stride_min_on_and_next_to_a_power_of_two(mz, fid, smin):
    p = PRIME[fid]
    rnd = random.Random(1000 * fid + smin)
    n = 1
    while n < smin:
        n *= 2
    for cons, point in size_edge_calls(rnd, p, smin):
        lens = [len(q) for q in point]
        assert mm.degree_bounds(cons, lens)[:2] == (n, smin)
        want = check(mz, fid, cons, point)
        assert len(want[0]) == smin
        for stride in (smin, smin + 3, n + 5):
            check_dev(mz, fid, cons, point, stride, want)


# ---- operands next to the modulus --------------------------------------------------------------------------------------------------------
@FIELDS
def test_every_coefficient_and_every_point_coefficient_p_minus_one(mz, fid):
    p = PRIME[fid]
    m = p - 1
    chain_to_constant = [(m, (29 - i,)) for i in range(30)]                      # HORNER after HORNER, the flush on a HORNER
    chain_to_x = [(m, (30 - i,)) for i in range(30)]                             # ... the flush on the tail product
    behind_horner = [(m, (3,)), (m, (2,)), (m, (2,)), (m, (2,)), (m, (1,)), (m, (1,))]      # ADDC on a lazy sum, HORNER on its result
    behind_pow = [(m, (9,)), (m, (4,)), (m, (4,)), (m, (0,)), (m, (0,))]         # ADDC behind two products, and behind a flush-less ADDC
    behind_square = [(m, (20,)), (m, (13,)), (m, (13,)), (m, (12,))]              # ADDC behind POW
    cons = [chain_to_constant, chain_to_x, behind_horner, behind_pow, behind_square]
    for point in ([[m, m]], [[m]], [[m, m, m]], [[0, m]], [[1, 1]]):
        check(mz, fid, cons, point)
    # several variables, everything p - 1: MULT chains on lazy sums
    cons2 = [[(m, (2, 3, 1)), (m, (1, 3, 1)), (m, (0, 3, 1)), (m, (6, 0, 0)), (m, (5, 0, 0)), (m, (0, 0, 0))],
             [(m, (0, 7, 4)), (m, (0, 6, 4)), (m, (0, 6, 4)), (m, (1, 1, 1))]]
    check(mz, fid, cons2, [[m, m], [m, m, m], [m]])
    rnd = random.Random(31 + fid)
    check(mz, fid, cons2 + cons2[::-1], [[rnd.randrange(p - 4, p) for _ in range(n)] for n in (3, 2, 2)])


@FIELDS
def test_constants_under_exponents_of_31_and_32_bits(mz, fid):
    p = PRIME[fid]
    m = p - 1
    rnd = random.Random(37 + fid)
    big = ((1 << 31) - 1, 1 << 31, (1 << 32) - 1)
    point = [[0], [1], [m], [rnd.randrange(2, p - 1)]]
    cons = [[(m, (0, e, 0, 0)), (m, (0, 0, e, 0)), (rnd.randrange(p), (0, 0, 0, e)), (m, (e, 0, 0, 0))] for e in big]
    cons += [[(m, (0, big[0], big[1], big[2])), (m, (0, big[2], big[0], big[1]))], [(m, (big[2], 1, 1, 1))], [(1, (0, 0, big[1], 0)), (m, (0, 0, big[0], 0))]]
    want = check(mz, fid, cons, point)
    assert mm.degree_bounds(cons, [1, 1, 1, 1])[:2] == (1, 1)
    assert want[4] == [] and want[5] == [2] and all(len(r) == 1 for r in want[:4])


# ---- invariances, each against the model -------------------------------------------------------------------------------------------------
@FIELDS
def test_invariances(mz, fid):
    p = PRIME[fid]
    rnd = random.Random(41 + fid)
    nv = 3
    point = [rand_poly(rnd, p, n) for n in (4, 2, 3)]
    cons = []
    for a in range(6):
        terms = [(rnd.randrange(p), tuple(rnd.choice((0, 0, 1, 2, 3, 4, 6, 7, 9)) for _ in range(nv))) for _ in range(rnd.randrange(2, 14))]
        cons.append(terms + [(rnd.randrange(p), terms[0][1])])                       # a duplicate row in each
    cons[1] = [(c, (k[0], min(k[1], 1), 0)) for c, k in cons[1]]                     # alone: depth 1 on the second variable, none on the third
    want = check(mz, fid, cons, point)
    # terms permuted
    shuffled = [rnd.sample(terms, len(terms)) for terms in cons]
    assert compose(mz, fid, shuffled, point) == want == model(fid, shuffled, point)
    # every constraint alone: other depths, other slots
    for terms, row in zip(cons, want):
        assert compose(mz, fid, [terms], point) == [row]
    # an extra constraint that raises another variable's depth
    extra = [(rnd.randrange(p), (0, 0, 3)), (rnd.randrange(p), (0, 2, 0))]
    assert compose(mz, fid, [cons[1], extra], point) == [want[1], mm.compose_terms(extra, point, p)]
    assert compose(mz, fid, [extra, cons[1]], point) == [mm.compose_terms(extra, point, p), want[1]]
    # variables permuted together with the point
    for perm in ((2, 0, 1), (1, 2, 0), (0, 2, 1)):
        pc = [[(c, tuple(k[i] for i in perm)) for c, k in terms] for terms in cons]
        pp = [point[i] for i in perm]
        assert model(fid, pc, pp) == want
        assert compose(mz, fid, pc, pp) == want


# ---- ABI offsets, raw ctypes ----------------------------------------------------------------------------------------------------------------
def raw_compose(mz, fid, coefs, exps, toff, nc, nv, point, poff, out, stride, lens):
    P_ = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    A = lambda v: None if v is None else (ctypes.c_size_t * len(v))(*v)
    return mz.lib().mzk_mpoly_compose(fid, P_(coefs), P_(exps), A(toff), ctypes.c_size_t(nc), ctypes.c_size_t(nv), P_(point), A(poff), P_(out),
                                      ctypes.c_size_t(stride), lens)


@FIELDS
def test_offsets_that_do_not_begin_at_zero(mz, fid):
    p, nl = PRIME[fid], NL[fid]
    rnd = random.Random(43 + fid)
    junk = np.full((3, nl), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)                       # not canonical: never read
    cons = [[(rnd.randrange(p), (2, 1, 0)), (rnd.randrange(p), (1, 1, 0)), (rnd.randrange(p), (0, 0, 0))],
            [],
            [(rnd.randrange(p), (0, 3, 0)), (rnd.randrange(p), (0, 0, 5)), (rnd.randrange(p), (7, 0, 0)), (rnd.randrange(p), (0, 3, 0))]]
    point = [rand_poly(rnd, p, 3), rand_poly(rnd, p, 2), []]                           # the third is empty: exponent 0 keeps a term, 5 drops it
    want = model(fid, cons, point)
    assert want[2] == mm.compose_terms([cons[2][0], cons[2][2], cons[2][3]], point, p) and len(want[2]) == 15
    flat_terms = [t for terms in cons for t in terms]
    coefs = np.concatenate([junk, limbs(fid, [c for c, _ in flat_terms])])
    exps = np.concatenate([np.full((3, 3), 0xFFFFFFFF, dtype=np.uint32), np.array([k for _, k in flat_terms], dtype=np.uint32)])
    toff = [3, 6, 6, 10]
    pts = np.concatenate([junk[:2], limbs(fid, point[0] + point[1])])
    poff = [2, 5, 7, 7]
    n, smin, bounds = mm.degree_bounds(cons, [3, 2, 0])
    for stride in (smin, smin + 2):
        out = np.full((3, stride, nl), GUARD, dtype=np.uint64)
        lens = (ctypes.c_size_t * 3)()
        assert raw_compose(mz, fid, coefs, exps, toff, 3, 3, pts, poff, out, stride, lens) == 0
        assert list(lens) == [len(w) for w in want]
        for a in range(3):
            assert ints(out[a, :lens[a]]) == want[a] and not out[a, lens[a]:].any()
    # the plan reads the same offsets
    nt, sm = ctypes.c_size_t(0), ctypes.c_size_t(0)
    bd = (ctypes.c_size_t * 3)()
    A = lambda v: (ctypes.c_size_t * len(v))(*v)
    assert mz.lib().mzk_mpoly_compose_plan(fid, exps.ctypes.data_as(ctypes.c_void_p), A(toff), ctypes.c_size_t(3), ctypes.c_size_t(3), A(poff),
                                           ctypes.byref(nt), ctypes.byref(sm), bd) == 0
    assert (nt.value, sm.value, list(bd)) == (n, smin, bounds)


@FIELDS
def test_a_call_in_which_everything_vanishes(mz, fid):
    p, nl = PRIME[fid], NL[fid]
    cons = [[(5, (1, 0)), (p - 1, (3, 2))], [], [(7, (13, 1))]]
    point = [[], [1, 2, 3]]
    assert model(fid, cons, point) == [[], [], []]
    assert mm.degree_bounds(cons, [0, 3]) == (1, 0, [0, 0, 0])
    assert mz.mpoly_compose_plan(fid, cons, [0, 3]) == (1, 0, [0, 0, 0])
    flat_terms = [t for terms in cons for t in terms]
    coefs, exps = limbs(fid, [c for c, _ in flat_terms]), np.array([k for _, k in flat_terms], dtype=np.uint32)
    pts = limbs(fid, point[1])
    for stride in (0, 5):
        out = np.full((3, max(stride, 1), nl), GUARD, dtype=np.uint64)
        lens = (ctypes.c_size_t * 3)(9, 9, 9)
        assert raw_compose(mz, fid, coefs, exps, [0, 2, 2, 3], 3, 2, pts, [0, 0, 3], out, stride, lens) == 0
        assert list(lens) == [0, 0, 0]
        assert (out == np.uint64(GUARD)).all() if stride == 0 else not out.any()
    assert compose(mz, fid, cons, point, out_stride=5) == [[], [], []]


# ---- many constraints in one grid ----------------------------------------------------------------------------------------------------------
@FIELDS
@pytest.mark.parametrize("nc", [1, 2, 255, 256, 1000])
def test_many_constraints_in_one_call(mz, fid, nc):
    """at 1000 constraints of five terms: 5000 terms in one call"""
    p = PRIME[fid]
    rnd = random.Random(7000 + 10 * nc + fid)
    point = [rand_poly(rnd, p, 3), rand_poly(rnd, p, 2)]
    per = 5 if nc == 1000 else 3
    cons = [[(rnd.randrange(p), (rnd.randrange(6), rnd.randrange(4))) for _ in range(per)] for _ in range(nc)]
    if nc in (255, 256):
        cons[nc // 2] = []                                                           # an empty constraint inside the grid
    assert nc != 1000 or sum(len(t) for t in cons) == 5000
    want = check(mz, fid, cons, point)
    if nc >= 255:
        stride = mm.degree_bounds(cons, [3, 2])[1] + 1
        check_dev(mz, fid, cons, point, stride, want)


# ---- the weighted combination ----------------------------------------------------------------------------------------------------------------
def lincomb_dev(mz, fid, polys, weights, shifts, cap):
    import torch
    nl = NL[fid]
    flat = np.concatenate([limbs(fid, q) for q in polys] + [limbs(fid, [9])])
    d_in = torch.from_numpy(flat.view(np.int64).reshape(-1).copy()).cuda()
    d_out = torch.full(((cap + 1) * nl,), GUARD, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = mz.poly_lincomb_dev(fid, d_in.data_ptr(), [len(q) for q in polys], weights, shifts, d_out.data_ptr(), cap, 0)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64).reshape(cap + 1, nl)
    assert not out[n:cap].any() and (out[cap] == np.uint64(GUARD)).all()
    assert np.array_equal(d_in.cpu().numpy().view(np.uint64).reshape(-1, nl), flat)
    return ints(out[:n]) if n else []


def check_lincomb(mz, fid, polys, weights, shifts, cap):
    want = mm.lincomb(polys, weights, shifts, PRIME[fid])
    assert ints(mz.poly_lincomb(fid, [limbs(fid, q) for q in polys], weights, shifts, out_cap=cap)) == want
    assert lincomb_dev(mz, fid, polys, weights, shifts, cap) == want
    return want


@FIELDS
@pytest.mark.parametrize("cap", [0, 1, 255, 256, 257])
def test_lincomb_at_every_capacity(mz, fid, cap):
    p = PRIME[fid]
    rnd = random.Random(90 + 2 * cap + fid)
    w = lambda: rnd.randrange(1, p)
    assert check_lincomb(mz, fid, [], [], [], cap) == []                                    # count 0: the zero polynomial, out zero-filled
    assert check_lincomb(mz, fid, [[], []], [w(), w()], [0, cap], cap) == []                # zero-length polynomials at both ends of out
    if cap == 0:
        return
    top = rand_poly(rnd, p, cap - 1) + [w()]
    assert len(check_lincomb(mz, fid, [top], [w()], [0], cap)) == cap
    assert check_lincomb(mz, fid, [[w()]], [w()], [cap - 1], cap)[:cap - 1] == [0] * (cap - 1)
    assert check_lincomb(mz, fid, [top, top], [0, p - 1], [0, 0], cap) == [(-v) % p for v in top]
    if cap == 1:
        return
    h = cap // 2
    a, b, c = rand_poly(rnd, p, h - 1) + [w()], rand_poly(rnd, p, cap - h - 1) + [w()], rand_poly(rnd, p, 40)
    # disjoint shifts that tile out; overlapping ones; zero-length polynomials between full ones
    assert check_lincomb(mz, fid, [a, b], [w(), w()], [0, h], cap) and check_lincomb(mz, fid, [b, a], [w(), w()], [0, cap - h], cap)
    check_lincomb(mz, fid, [a, [], b, [], c, top], [w(), w(), p - 1, 0, w(), w()], [3, 7, 1, cap, cap - 40, 0], cap)
    check_lincomb(mz, fid, [c, c, c], [p - 1, p - 1, p - 1], [0, 1, 39], cap)
    # everything cancels; only the leading terms cancel
    k = w()
    assert check_lincomb(mz, fid, [top, [], top], [k, w(), p - k], [0, 5, 0], cap) == []
    low = [(top[0] + 1) % p] + top[1:]
    assert check_lincomb(mz, fid, [top, low], [k, p - k], [0, 0], cap) == [(p - k) % p]
    lead = top[:h] + [(top[h] + 1) % p] + top[h + 1:]
    assert len(check_lincomb(mz, fid, [lead, top], [k, p - k], [0, 0], cap)) == h + 1


@FIELDS
def test_lincomb_offsets_that_do_not_begin_at_zero(mz, fid):
    p, nl = PRIME[fid], NL[fid]
    rnd = random.Random(97 + fid)
    polys = [rand_poly(rnd, p, 5), [], rand_poly(rnd, p, 300)]
    weights, shifts, cap = [p - 1, 3, rnd.randrange(p)], [290, 2, 0], 301
    want = mm.lincomb(polys, weights, shifts, p)
    flat = np.concatenate([np.full((4, nl), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64), limbs(fid, polys[0] + polys[2])])
    off = (ctypes.c_size_t * 4)(4, 9, 9, 309)
    sh = (ctypes.c_size_t * 3)(*shifts)
    out = np.full((cap, nl), GUARD, dtype=np.uint64)
    n = ctypes.c_size_t(77)
    P_ = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert mz.lib().mzk_poly_lincomb(fid, P_(flat), off, ctypes.c_size_t(3), P_(limbs(fid, weights)), sh, P_(out), ctypes.c_size_t(cap), ctypes.byref(n)) == 0
    assert n.value == len(want) and ints(out[:n.value]) == want and not out[n.value:].any()
