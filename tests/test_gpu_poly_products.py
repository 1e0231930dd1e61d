"""mzk_fft_multiply and mzk_fast_multiply (mzk_api.hip over mzk_mul_plan.h: order and sub-root, zero padding, k_pointwise_mul, the
in-place transforms on workspace slots, trimming, the reference's conventions for empty and zero operands) against
tests/poly_product_model.py, the same products on Python integers, and -- up to order 2^11 -- against the CPU oracle's literal
recursions as well.  Every length pair up to 17 x 17, every order boundary 2^5 .. 2^13 (exact fit and one more), every pass count of
the transforms (one pass up to 2^10, two up to 2^16, three from 2^17, the large tiles at 2^20: mzk_ntt_plan.h), trailing zeros,
zero and empty operands between two runs of a fixed product, edge values, stale workspace, and the refusals with the next call
checked after each.  Exact: every comparison is equality of integers."""
import ctypes
import numpy as np
import pytest
import orc
import poly_product_model as model
from orc import FR, M128

pytestmark = pytest.mark.gpu
FIELDS = [FR, M128]
ORACLE_MAX_ORDER = 1 << 11                    # the literal recursions are slow above
BIG_ROOT_ORDER = 1 << 21
# lopsided: one Kronecker product of a long by a short operand is fast.  m = 2^16 + 1 -> n = 2^17 (three passes) and
# m = 2^19 + 8 -> n = 2^20 (the large tiles); for fast_multiply degree 2^16 -> order 2^17 and degree 2^19 + 7 -> order 2^20
BIG_SHAPES = [((1 << 16) - 62, 64), ((1 << 19) + 1, 8)]


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


def lg(n):
    return n.bit_length() - 1


def omega_for(fid, la, lb):
    n = model.next_power_of_two(la + lb - 1)
    return orc.root_of(fid, lg(n)) if n > 1 else 1


def same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


def check_fft(mz, fid, a, b, tag=None):
    la, lb = a.shape[0], b.shape[0]
    w = omega_for(fid, la, lb)
    rc, want = model.fft_multiply(fid, a, b)
    got = mz.fft_multiply(fid, a, b, w)
    assert rc == 0 and same(got, want), ("fft_multiply", fid, la, lb, tag, got.shape, want.shape)
    if model.next_power_of_two(la + lb - 1) <= ORACLE_MAX_ORDER:
        rc, ref = orc.fft_multiply_ref(fid, a, b, w)
        assert rc == 0 and same(ref, want), ("oracle fft_multiply", fid, la, lb, tag)
    return got


def check_fast(mz, fid, a, b, root_order, tag=None):
    w = orc.root_of(fid, lg(root_order))
    rc, want = model.fast_multiply(fid, a, b, root_order)
    got = mz.fast_multiply(fid, a, b, w, root_order)
    assert rc == 0 and same(got, want), ("fast_multiply", fid, a.shape[0], b.shape[0], root_order, tag, got.shape, want.shape)
    if want.shape[0] <= ORACLE_MAX_ORDER:
        rc, ref = orc.fast_multiply_ref(fid, a, b, w, root_order)
        assert rc == 0 and same(ref, want), ("oracle fast_multiply", fid, a.shape[0], b.shape[0], root_order, tag)
    return got


def code_of(mz, call):
    with pytest.raises(mz.MzkError) as e:
        call()
    return e.value.code


def edge_operands(fid, la, lb):
    """(tag, a, b): constant and alternating fills of the largest values; for M128 the values whose 29-bit limbs are all at their
    maximum (test_gpu_ntt.py::test_noncanonical_edge_values)"""
    p = orc.MOD[fid]
    fills = {"p-1": lambda i: p - 1, "0,p-1": lambda i: (p - 1) * (i & 1)}
    if fid == M128:
        fills["2^116-1"] = lambda i: (1 << 116) - 1
        fills["p-2"] = lambda i: p - 2
    out = []
    for tag, f in fills.items():
        a, b = model.to_arr(fid, [f(i) for i in range(la)]), model.to_arr(fid, [f(i) for i in range(lb)])
        out.append((tag, a, b))
        out.append((tag + " x random", a, model.operand(fid, 31, lb)))
    return out


# ---- fft_multiply --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIELDS)
def test_fft_every_length_pair_up_to_17(mz, fid):
    """m = la + lb - 1 crosses 1, 2, 4, 8, 16 and 32"""
    for la in range(1, 18):
        for lb in range(1, 18):
            got = check_fft(mz, fid, model.operand(fid, 11 + la, la), model.operand(fid, 57 + lb, lb))
            assert got.shape[0] == la + lb - 1


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("k", range(5, 14))
def test_fft_order_boundaries(mz, fid, k):
    for m, (la, lb) in model.fft_boundary_shapes(k):
        got = check_fft(mz, fid, model.operand(fid, 100 + k, la), model.operand(fid, 200 + k, lb))
        assert la + lb - 1 == m and got.shape[0] == m


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("shape", BIG_SHAPES)
def test_fft_three_passes_and_large_tiles_exact(mz, fid, shape):
    la, lb = shape
    got = check_fft(mz, fid, model.operand(fid, 7, la), model.operand(fid, 8, lb))
    assert got.shape[0] == la + lb - 1


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_three_passes_equal_lengths_by_evaluation(mz, fid):
    """(2^16, 2^16 + 1): m = 2^17 = n fits exactly.  Too long for an exact model: the product evaluated at four points by Horner's
    rule, its length, and the other entry point on the same operands (order 2^17 from a root of order 2^21)"""
    p = orc.MOD[fid]
    la, lb = 1 << 16, (1 << 16) + 1
    a, b = model.operand(fid, 21, la), model.operand(fid, 22, lb)
    got = mz.fft_multiply(fid, a, b, orc.root_of(fid, 17))
    assert got.shape[0] == 1 << 17
    for x in (2, p - 1, orc.root_of(fid, 20), model.to_ints(model.operand(fid, 23, 1))[0]):
        assert orc.poly_eval(fid, got, x) == orc.poly_eval(fid, a, x) * orc.poly_eval(fid, b, x) % p, x
    fast = mz.fast_multiply(fid, a, b, orc.root_of(fid, lg(BIG_ROOT_ORDER)), BIG_ROOT_ORDER)
    assert same(fast, got)


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_trailing_zeros_and_zero_operand(mz, fid):
    """m and n come from the stored lengths, the result is trimmed (polynomial.rs:244-245, :271-275)"""
    for la, lb in ((20, 14), (33, 32), (1025, 1024)):
        for za, zb in ((1, 0), (3, 0), (0, 1), (0, 3), (1, 1), (3, 3), (1, 3)):
            got = check_fft(mz, fid, model.operand(fid, 3, la, za), model.operand(fid, 4, lb, zb), (za, zb))
            assert got.shape[0] == la - za + lb - zb - 1
    for a, b in ((model.operand(fid, 3, 5, 5), model.operand(fid, 4, 7)), (model.operand(fid, 3, 7), model.operand(fid, 4, 5, 5))):
        assert check_fft(mz, fid, a, b, "zero operand").shape[0] == 0


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_empty_operand_is_the_empty_product(mz, fid):
    """la = 0: m = lb - 1, and for lb = 2^k + 1 the order n = 2^k is one less than the operand's length; the reference's resize cuts
    it and the product is empty whatever omega is.  Nothing may be written past a buffer: the same (300, 213) product is exact
    immediately before and after every such call."""
    fa, fb = model.operand(fid, 41, 300), model.operand(fid, 42, 213)
    fw = omega_for(fid, 300, 213)
    rc, fixed = model.fft_multiply(fid, fa, fb)
    assert rc == 0 and fixed.shape[0] == 512
    for lb in (1, 2, 3, 4, 5, 9, 129, 4097):
        b = model.operand(fid, 50 + lb, lb)
        for x, y in ((b[:0], b), (b, b[:0])):
            assert model.fft_multiply(fid, x, y)[1].shape[0] == 0
            assert same(mz.fft_multiply(fid, fa, fb, fw), fixed), ("before", lb)
            assert mz.fft_multiply(fid, x, y, 1).shape[0] == 0, (x.shape[0], y.shape[0])
            assert same(mz.fft_multiply(fid, fa, fb, fw), fixed), ("after", lb)
    e = fa[:0]
    assert code_of(mz, lambda: mz.fft_multiply(fid, e, e, 1)) == -5 == model.fft_multiply(fid, e, e)[0]      # polynomial.rs:244
    assert same(mz.fft_multiply(fid, fa, fb, fw), fixed)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("shape", [(40, 25), (1024, 1025)])
def test_fft_edge_values(mz, fid, shape):
    for tag, a, b in edge_operands(fid, *shape):
        check_fft(mz, fid, a, b, tag)


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_small_products_after_a_large_one(mz, fid):
    """the padding of the small products lies where the (3000, 3000) call left its transforms"""
    check_fft(mz, fid, model.operand(fid, 61, 3000), model.operand(fid, 62, 3000))
    check_fft(mz, fid, model.operand(fid, 63, 5), model.operand(fid, 64, 4))
    check_fft(mz, fid, model.operand(fid, 65, 33), model.operand(fid, 66, 32))


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_omega_is_checked(mz, fid):
    """The reference's private fft takes any omega (polynomial.rs:278-300); the transforms here check theirs like ntt::ntt
    (ntt.rs:15-22), include/mzk.h says so: twice the order MZK_E_ROOT_ORDER, half the order MZK_E_ROOT_PRIM, not canonical
    MZK_E_RANGE, NULL with n > 1 MZK_E_ARG -- and the next call is right"""
    from myzkp_amd import _lib as L
    a, b = model.operand(fid, 71, 40), model.operand(fid, 72, 25)      # n = 64
    nl = orc.LIMBS[fid]

    def null_omega(x, y):
        out = np.zeros((x.shape[0] + y.shape[0], nl), dtype=np.uint64)
        n = ctypes.c_size_t(99)
        rc = L.lib().mzk_fft_multiply(fid, L._p(x), ctypes.c_size_t(x.shape[0]), L._p(y), ctypes.c_size_t(y.shape[0]), None, L._p(out), ctypes.byref(n))
        return rc, out[:n.value]

    for bad, code in ((orc.root_of(fid, 7), -3), (orc.root_of(fid, 5), -4), (orc.MOD[fid], -6)):
        assert code_of(mz, lambda: mz.fft_multiply(fid, a, b, bad)) == code
        check_fft(mz, fid, a, b, "after %d" % code)
    assert null_omega(a, b)[0] == -1
    check_fft(mz, fid, a, b, "after a null omega")
    # n = 1: fft() of one point is the identity (:279-282), omega is not read; nor is it for an empty operand
    rc, one = null_omega(a[:1], b[:1])
    assert rc == 0 and same(one, model.fft_multiply(fid, a[:1], b[:1])[1])
    rc, none = null_omega(a[:0], b)
    assert rc == 0 and none.shape[0] == 0


# ---- fast_multiply -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIELDS)
def test_fast_below_degree_8_is_the_trimmed_schoolbook_product(mz, fid):
    """ntt.rs:86-88 returns lhs * rhs before it looks at the order: root_order 2 succeeds; trailing zeros do not count"""
    p = orc.MOD[fid]
    for da in range(1, 9):
        for db in range(1, 10 - da):
            for la, lb in ((da, db), (40, 40)):
                a, b = model.operand(fid, 80 + da, la, la - da), model.operand(fid, 90 + db, lb, lb - db)
                want = model.to_arr(fid, model.trim(model.schoolbook(p, model.to_ints(a[:da]), model.to_ints(b[:db]))))
                for root_order in (2, 16, 1024):
                    got = check_fast(mz, fid, a, b, root_order, (da, db))
                    assert same(got, want) and got.shape[0] == da + db - 1


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("k", range(4, 14))
def test_fast_order_boundaries(mz, fid, k):
    """degree 2^k - 1 fits order 2^k exactly, degree 2^k takes 2^(k + 1); the result is the order's coefficients, untrimmed"""
    shapes = model.fast_boundary_shapes(k) + ([(16, s) for s in ((5, 5), (9, 1), (1, 9))] if k == 4 else [])
    for order, (la, lb) in shapes:
        got = check_fast(mz, fid, model.operand(fid, 300 + k, la), model.operand(fid, 400 + k, lb), 1 << 14)
        assert got.shape[0] == order and got[la + lb - 2].any() and not got[la + lb - 1:].any(), (la, lb)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("shape", BIG_SHAPES)
def test_fast_three_passes_and_large_tiles_exact(mz, fid, shape):
    la, lb = shape
    got = check_fast(mz, fid, model.operand(fid, 7, la), model.operand(fid, 8, lb), BIG_ROOT_ORDER)
    assert got.shape[0] == model.next_power_of_two(la + lb - 1) and not got[la + lb - 1:].any()


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_no_halving_wraps_around(mz, fid):
    """root_order 16, degree 22: nothing is halved and the reference returns the cyclic convolution mod X^16 - 1"""
    p = orc.MOD[fid]
    a, b = model.operand(fid, 1, 12), model.operand(fid, 2, 12)
    full = model.schoolbook(p, model.to_ints(a), model.to_ints(b))
    want = [(full[i] + (full[i + 16] if i + 16 < len(full) else 0)) % p for i in range(16)]
    assert model.to_ints(check_fast(mz, fid, a, b, 16)) == want


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_trailing_zeros_and_stored_length(mz, fid):
    """the order comes from the trimmed degree, the copy from the stored length: up to the order exact (ntt.rs:95-102 fills no
    further), one more reaches the reference's ntt as it is and panics; a zero operand of any stored length is the empty product"""
    for k, d in ((5, 10), (11, 600)):
        order = 1 << k
        assert model.fast_order(2 * d - 2, 1 << 14) == order
        for la, lb in ((order, d + 3), (d + 3, order), (order, order)):
            got = check_fast(mz, fid, model.operand(fid, 5, la, la - d), model.operand(fid, 6, lb, lb - d), 1 << 14, (la, lb))
            assert got.shape[0] == order
        for la, lb in ((order + 1, d), (d, order + 1)):
            a, b = model.operand(fid, 5, la, la - d), model.operand(fid, 6, lb, lb - d)
            assert code_of(mz, lambda: mz.fast_multiply(fid, a, b, orc.root_of(fid, 14), 1 << 14)) == -5 == model.fast_multiply(fid, a, b, 1 << 14)[0]
            check_fast(mz, fid, a[:order], b[:order], 1 << 14, "after the refusal")
    b = model.operand(fid, 6, 20)
    for la in (1, 5, 40, 5000):
        z = model.operand(fid, 5, la, la)
        assert check_fast(mz, fid, z, b, 1 << 14).shape[0] == 0 and check_fast(mz, fid, b, z, 1 << 14).shape[0] == 0
    assert check_fast(mz, fid, b[:0], b, 1 << 14).shape[0] == 0 and check_fast(mz, fid, b, b[:0], 1 << 14).shape[0] == 0


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_refusals_leave_the_next_call_right(mz, fid):
    a, b = model.operand(fid, 7, 40), model.operand(fid, 8, 25)
    for bad, code in ((orc.root_of(fid, 15), -3),      # ntt.rs:75 root^order != 1
                      (orc.root_of(fid, 13), -4),      # ntt.rs:76 not primitive
                      (orc.MOD[fid], -6)):             # not canonical
        assert code_of(mz, lambda: mz.fast_multiply(fid, a, b, bad, 1 << 14)) == code
        check_fast(mz, fid, a, b, 1 << 14, "after %d" % code)


def test_fast_order_that_is_no_power_of_two(mz):
    """root_order 48 over Fr with an element of order exactly 48, degree 20: the order stops at 24 and ntt.rs:8-11 panics"""
    r = orc.P_FR
    g = pow(5, (r - 1) // 48, r)
    assert pow(g, 48, r) == 1 and pow(g, 24, r) != 1 and pow(g, 16, r) != 1
    a, b = model.operand(FR, 7, 11), model.operand(FR, 8, 11)
    assert code_of(mz, lambda: mz.fast_multiply(FR, a, b, g, 48)) == -2 == model.fast_multiply(FR, a, b, 48)[0]
    check_fast(mz, FR, a, b, 1 << 14, "after the refusal")


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("shape", [(40, 25), (1024, 1025)])
def test_fast_edge_values(mz, fid, shape):
    for tag, a, b in edge_operands(fid, *shape):
        check_fast(mz, fid, a, b, 1 << 14, tag)


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_small_products_after_a_large_one(mz, fid):
    check_fast(mz, fid, model.operand(fid, 61, 3000), model.operand(fid, 62, 3000), 1 << 14)
    check_fast(mz, fid, model.operand(fid, 63, 5), model.operand(fid, 64, 4), 1 << 14)
    check_fast(mz, fid, model.operand(fid, 65, 33), model.operand(fid, 66, 32), 1 << 14)


def test_every_pass_count_is_reached_by_both_entry_points():
    """one pass up to 2^10, two for 2^11 .. 2^16, three from 2^17, the large tiles at 2^20 (mzk_ntt_plan.h)"""
    def kind(order):
        return "large" if order == 1 << 20 else 1 if order <= 1 << 10 else 2 if order <= 1 << 16 else 3
    fft = {model.next_power_of_two(m) for k in range(5, 14) for m, _ in model.fft_boundary_shapes(k)} | {model.next_power_of_two(la + lb - 1) for la, lb in BIG_SHAPES}
    fast = {o for k in range(4, 14) for o, _ in model.fast_boundary_shapes(k)} | {model.fast_order(la + lb - 2, BIG_ROOT_ORDER) for la, lb in BIG_SHAPES}
    assert {kind(o) for o in fft} == {1, 2, 3, "large"} == {kind(o) for o in fast}
