"""Pin the CPU oracle's two polynomial products (oracle/mzk_oracle.c: orc_fft_multiply_ref, orc_fast_multiply_ref -- the literal
recursions of polynomial.rs:242-300 and ntt.rs:7-116) on tests/poly_product_model.py, the same products on Python integers with no
transform in them: every (la, lb) in 0 .. 20 in both fields, the empty-operand shapes (0, 2^k + 1) among them, and the order
boundaries up to 2^11.  The model's two product rules are checked against each other first.  A stand-alone program runs the oracle
at the empty-operand shapes under AddressSanitizer (tests/hostcheck/oracle_products_main.c).  Exact; CPU only."""
import os, random, subprocess
import numpy as np
import pytest
import orc
import poly_product_model as model
from orc import FR, M128

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIELDS = [FR, M128]


def omega_for(fid, la, lb):
    n = model.next_power_of_two(la + lb - 1)
    return orc.root_of(fid, n.bit_length() - 1) if n > 1 else 1


def same(got, want):
    return got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("fid", FIELDS)
def test_model_kronecker_equals_schoolbook(fid):
    """the two rules share nothing but the operands: lengths around the stride's bits(min(la, lb)) steps, edge values that make
    every coefficient of the integer product as large as it gets"""
    p = orc.MOD[fid]
    rng = random.Random(1000 + fid)
    for la, lb in ((1, 1), (1, 9), (2, 3), (7, 8), (8, 8), (31, 33), (64, 65), (127, 5), (128, 129), (200, 150)):
        a, b = [rng.randrange(p) for _ in range(la)], [rng.randrange(p) for _ in range(lb)]
        assert model.kronecker(p, a, b) == model.schoolbook(p, a, b), (la, lb)
        assert model.kronecker(p, [p - 1] * la, [p - 1] * lb) == model.schoolbook(p, [p - 1] * la, [p - 1] * lb), (la, lb)
    assert model.kronecker(p, [], [1]) == [] == model.schoolbook(p, [1], [])
    assert model.fold(p, [1, 2, 3, 4, 5], 4) == [6, 2, 3, 4] and model.fold(p, [1, 2], 4) == [1, 2, 0, 0] and model.fold(p, [p - 1, 0, 0, 0, 1], 4) == [0, 0, 0, 0]


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_multiply_every_small_pair(fid):
    for la in range(21):
        for lb in range(21):
            a, b = model.operand(fid, 11 + la, la), model.operand(fid, 57 + lb, lb)
            rc_want, want = model.fft_multiply(fid, a, b)
            if la + lb == 0:
                assert rc_want == model.E_LENGTH and orc.fft_multiply_ref(fid, a, b, 1)[0] == -5      # :244 usize underflow
                continue
            rc, got = orc.fft_multiply_ref(fid, a, b, omega_for(fid, la, lb))
            assert rc == 0 and rc_want == 0 and same(got, want), (la, lb)
            if la == 0 or lb == 0:
                assert got.shape[0] == 0


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_multiply_empty_operand_against_two_to_the_k_plus_one(fid):
    """m = lb - 1 = 2^k = n: resize(n) cuts the operand (polynomial.rs:248-251), the product is empty"""
    for lb in (3, 5, 9, 17, 129, 1025, 4097):
        b = model.operand(fid, lb, lb)
        e = b[:0]
        w = omega_for(fid, 0, lb)
        for x, y in ((e, b), (b, e)):
            rc, got = orc.fft_multiply_ref(fid, x, y, w)
            assert rc == 0 and got.shape[0] == 0 and model.fft_multiply(fid, x, y)[1].shape[0] == 0, lb


@pytest.mark.parametrize("fid", FIELDS)
def test_fft_multiply_trailing_zeros_and_zero_operand(fid):
    """m and n come from the stored lengths; the result is trimmed"""
    for la, lb, za, zb in ((20, 14, 1, 0), (20, 14, 3, 0), (20, 14, 0, 3), (20, 14, 1, 3), (20, 14, 3, 3), (5, 7, 5, 0), (7, 5, 0, 5)):
        a, b = model.operand(fid, 3, la, za), model.operand(fid, 4, lb, zb)
        rc, got = orc.fft_multiply_ref(fid, a, b, omega_for(fid, la, lb))
        want = model.fft_multiply(fid, a, b)[1]
        assert rc == 0 and same(got, want), (la, lb, za, zb)
        assert got.shape[0] == (0 if za == la or zb == lb else la - za + lb - zb - 1)


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("k", range(5, 11))
def test_fft_multiply_order_boundaries(fid, k):
    for m, (la, lb) in model.fft_boundary_shapes(k):
        a, b = model.operand(fid, 100 + k, la), model.operand(fid, 200 + k, lb)
        rc, got = orc.fft_multiply_ref(fid, a, b, omega_for(fid, la, lb))
        assert la + lb - 1 == m and rc == 0 and got.shape[0] == m and same(got, model.fft_multiply(fid, a, b)[1]), (la, lb)


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_multiply_every_small_pair(fid):
    """root_order 64: the zero exit, the schoolbook exit below degree 8, orders 16, 32 and 64"""
    w = orc.root_of(fid, 6)
    orders = set()
    for la in range(21):
        for lb in range(21):
            for za, zb in ((0, 0), (min(la, 2), 0), (0, lb)):
                a, b = model.operand(fid, 11 + la, la, za), model.operand(fid, 57 + lb, lb, zb)
                rc_want, want = model.fast_multiply(fid, a, b, 64)
                rc, got = orc.fast_multiply_ref(fid, a, b, w, 64)
                assert rc == rc_want, (la, lb, za, zb)
                if rc == 0:
                    assert same(got, want), (la, lb, za, zb)
                    orders.add(got.shape[0])
    assert {0, 1, 8, 16, 32, 64} <= orders


@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("k", range(4, 11))
def test_fast_multiply_order_boundaries(fid, k):
    w = orc.root_of(fid, 14)
    for order, (la, lb) in model.fast_boundary_shapes(k):
        a, b = model.operand(fid, 300 + k, la), model.operand(fid, 400 + k, lb)
        rc, got = orc.fast_multiply_ref(fid, a, b, w, 1 << 14)
        assert rc == 0 and got.shape[0] == order and same(got, model.fast_multiply(fid, a, b, 1 << 14)[1]), (la, lb)
        assert not got[la + lb - 1:].any()


@pytest.mark.parametrize("fid", FIELDS)
def test_fast_multiply_wrap_around_stored_length_and_refusals(fid):
    a, b = model.operand(fid, 1, 12), model.operand(fid, 2, 12)
    rc, got = orc.fast_multiply_ref(fid, a, b, orc.root_of(fid, 4), 16)           # degree 22 >= 16: nothing is halved, the product wraps
    p = orc.MOD[fid]
    full = model.schoolbook(p, model.to_ints(a), model.to_ints(b))
    want = [(full[i] + (full[i + 16] if i + 16 < len(full) else 0)) % p for i in range(16)]
    assert rc == 0 and model.to_ints(got) == want and same(got, model.fast_multiply(fid, a, b, 16)[1])
    # trimmed degree 18 selects order 32: a stored length of 32 is filled no further, 33 reaches ntt as it is and panics
    w = orc.root_of(fid, 10)
    for la, rc_want in ((32, 0), (33, -5)):
        a, b = model.operand(fid, 5, la, la - 10), model.operand(fid, 6, 20, 10)
        rc, got = orc.fast_multiply_ref(fid, a, b, w, 1024)
        assert (rc, rc_want) == (rc_want, model.fast_multiply(fid, a, b, 1024)[0]), la
        if rc == 0:
            assert got.shape[0] == 32 and same(got, model.fast_multiply(fid, a, b, 1024)[1])
    a, b = model.operand(fid, 7, 11), model.operand(fid, 8, 11)
    assert orc.fast_multiply_ref(fid, a, b, orc.root_of(fid, 11), 1024)[0] == -3      # ntt.rs:75
    assert orc.fast_multiply_ref(fid, a, b, orc.root_of(fid, 9), 1024)[0] == -4       # ntt.rs:76


def test_fast_multiply_order_that_is_no_power_of_two():
    """root_order 48 over Fr, degree 20: order 24, and ntt.rs:8-11 panics"""
    r = orc.P_FR
    g = pow(5, (r - 1) // 48, r)
    assert pow(g, 48, r) == 1 and pow(g, 24, r) != 1 and pow(g, 16, r) != 1
    a, b = model.operand(FR, 7, 11), model.operand(FR, 8, 11)
    assert orc.fast_multiply_ref(FR, a, b, g, 48)[0] == -2 == model.fast_multiply(FR, a, b, 48)[0]


def test_oracle_products_under_address_sanitizer(tmp_path):
    """the empty-operand shapes with every buffer of exactly its documented size: copying all lb = 2^k + 1 coefficients into the
    2^k-element vector is a heap overflow the sanitizer reports"""
    exe = str(tmp_path / "oracle_products")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-fopenmp", "-Wall", "-Wextra", "-Wno-unused-parameter", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "oracle_products_main.c"),
                           os.path.join(ROOT, "oracle", "mzk_oracle.c"), "-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 73, r.stdout
