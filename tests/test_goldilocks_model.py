"""tests/goldilocks_model.py against facts checked here with plain integers, and its own FRI::prove / FRI::verify at the parameters of
the reference's test_fri_efield (zkstark/fri.rs:546-594).  CPU only."""
import random
import numpy as np
import pytest
import fri_prove_model as fpm
import goldilocks_model as gm

P = gm.P
X3 = gm.M64X3


def test_the_generator_has_order_2_32():
    assert P == 18446744069414584321
    assert pow(gm.ROOT_2_32, 1 << 32, P) == 1 and pow(gm.ROOT_2_32, 1 << 31, P) == P - 1
    assert gm.root_of_unity(gm.M64, 10) == pow(gm.ROOT_2_32, 1 << 22, P)
    assert gm.root_of_unity(X3, 10) == (pow(gm.ROOT_2_32, 1 << 22, P), 0, 0)


def _pmulmod(a, b, m):
    """a * b mod the monic polynomial m over F_p (coefficient lists, ascending)"""
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = (r[i + j] + x * y) % P
    d = len(m) - 1
    for k in range(len(r) - 1, d - 1, -1):
        c = r[k]
        if c:
            for j in range(d + 1):
                r[k - d + j] = (r[k - d + j] - c * m[j]) % P
    return (r + [0] * d)[:d]


def _pgcd(a, b):
    def trim(x):
        while x and x[-1] == 0:
            x = x[:-1]
        return x
    a, b = trim(list(a)), trim(list(b))
    while b:
        while len(a) >= len(b):          # a mod b
            c = a[-1] * pow(b[-1], -1, P) % P
            s = len(a) - len(b)
            a = trim([(x - c * b[i - s]) % P if i >= s else x for i, x in enumerate(a)])
        a, b = b, a
    return a


def test_ip3_is_irreducible():
    """a cubic is irreducible over F_p iff it has no root there iff gcd(x^p - x, m) = 1"""
    m = [1, P - 1, 0, 1]                                   # x^3 - x + 1
    xp, base, e = [1, 0, 0], [0, 1, 0], P                  # x^p mod m by square and multiply
    while e:
        if e & 1:
            xp = _pmulmod(xp, base, m)
        base = _pmulmod(base, base, m)
        e >>= 1
    g = _pgcd(m, [(xp[0]) % P, (xp[1] - 1) % P, xp[2]])
    assert len(g) == 1 and g[0] != 0
    assert xp == list(X3.pow((0, 1, 0), P))               # the model's own product agrees with the generic one


def test_extension_inverse():
    rng = random.Random(3)
    for _ in range(10):
        a = tuple(rng.randrange(P) for _ in range(3))
        assert X3.mul(a, X3.pow(a, P ** 3 - 2)) == X3.one == X3.mul(a, X3.inv(a))
    assert X3.mul((0, 1, 0), X3.mul((0, 1, 0), (0, 1, 0))) == (P - 1, 1, 0)


def test_fold_is_even_plus_alpha_odd_on_the_squared_coset():
    rng = random.Random(4)
    n, offset = 64, X3.from_int(7)
    omega = gm.root_of_unity(X3, 6)
    f = [tuple(rng.randrange(P) for _ in range(3)) for _ in range(16)]
    alpha = tuple(rng.randrange(P) for _ in range(3))
    cw = [gm.poly_eval(X3, f, X3.mul(offset, gm.fpow(X3, omega, i))) for i in range(n)]
    assert cw == gm.fast_coset_evaluate(X3, f, offset, omega, n)
    g = [X3.add(e, X3.mul(alpha, o)) for e, o in zip(f[0::2], f[1::2])]
    o2, w2 = X3.mul(offset, offset), X3.mul(omega, omega)
    assert gm.fold(X3, cw, alpha, offset, omega) == [gm.poly_eval(X3, g, X3.mul(o2, gm.fpow(X3, w2, i))) for i in range(n // 2)]


def test_ntt_round_trip_and_definition():
    rng = random.Random(5)
    for F in (gm.M64, X3):
        w = gm.root_of_unity(F, 4)
        v = [F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for _ in range(16)]
        t = gm.ntt(F, w, v)
        assert t == [gm.poly_eval(F, v, gm.fpow(F, w, k)) for k in range(16)]
        assert gm.intt(F, w, t) == v


def test_leaf_lengths():
    assert len(X3.leaf((0, 0, 0))) == 8
    assert len(X3.leaf((5, 0, 0))) == 21
    assert len(X3.leaf((P - 1, P - 1, P - 1))) == 59
    assert len(gm.M64.leaf(P - 1)) == 17
    assert X3.leaf((0, 5, 0)) == fpm.u64le(2) + fpm.leaf(0) + fpm.leaf(5) and len(fpm.leaf(0)) == 9


@pytest.fixture(scope="module")
def efield_case():
    """test_fri_efield: degree 63, expansion 16, 17 tests, n = 1024, offset 7, coefficients from_value(i), the codeword on omega^i"""
    n = 1024
    omega, offset = gm.root_of_unity(X3, 10), X3.from_int(7)
    coef = [X3.from_int(i) for i in range(64)]
    return n, omega, offset, coef, gm.ntt(X3, omega, coef + [X3.zero] * (n - 64))


def test_prove_and_verify_at_the_reference_parameters(efield_case):
    n, omega, offset, coef, cw = efield_case
    assert fpm.num_rounds(n, 16, 17) == 4
    proof = gm.prove(X3, cw, omega, offset, 16, 17)
    assert len(proof["merkle_roots"]) == 4 and len(proof["last_codeword"]) == 128
    points = []
    assert gm.verify(X3, proof, omega, offset, n, 16, 17, points)
    assert len(points) == 34
    for x, y in points:
        assert gm.poly_eval(X3, coef, gm.fpow(X3, omega, x)) == y


def test_verify_rejects_the_corrupted_codeword(efield_case):
    n, omega, offset, coef, cw = efield_case
    bad = [X3.one] * 21 + cw[21:]
    assert not gm.verify(X3, gm.prove(X3, bad, omega, offset, 16, 17), omega, offset, n, 16, 17, [])


# ---- the numpy form of the field ------------------------------------------------------------------------------------------------
EDGES = [0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - (1 << 32), 1 << 63, (1 << 64) - (1 << 32)]


def _check_ops(a, b):
    A, B = np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64)
    assert gm.np_mul(A, B).tolist() == [x * y % P for x, y in zip(a, b)]
    assert gm.np_add(A, B).tolist() == [(x + y) % P for x, y in zip(a, b)]
    assert gm.np_sub(A, B).tolist() == [(x - y) % P for x, y in zip(a, b)]


def test_numpy_field_ops_on_random_pairs():
    rng = random.Random(11)
    n = 20000
    _check_ops([rng.randrange(P) for _ in range(n)], [rng.randrange(P) for _ in range(n)])
    # operands with a half of all ones or all zeros: the carries between the partial products
    halves = [0, 1, (1 << 32) - 1, (1 << 32) - 2]
    pick = lambda: ((rng.choice(halves) << 32) | rng.randrange(1 << 32) if rng.random() < 0.5 else (rng.randrange(1 << 32) << 32) | rng.choice(halves)) % P
    _check_ops([pick() for _ in range(n)], [pick() for _ in range(n)])


def test_numpy_field_ops_on_the_edge_values():
    assert all(e < P for e in EDGES)
    _check_ops([x for x in EDGES for _ in EDGES], [y for _ in EDGES for y in EDGES])
    assert gm.np_mul(P - 1, np.uint64(P - 1)).tolist() == [1]               # scalars come back as one-element arrays


def test_numpy_powers():
    for a in (0, 1, 7, P - 1, gm.ROOT_2_32):
        for n in (1, 2, 3, 8, 1000):
            assert gm.np_powers(a, n).tolist() == [pow(a, i, P) for i in range(n)]


@pytest.mark.parametrize("n", [2, 4, 32, 1024])
def test_numpy_ntt_equals_the_literal_recursion(n):
    rng = random.Random(n)
    lg = n.bit_length() - 1
    for F in (gm.M64, X3):
        w = gm.root_of_unity(F, lg)
        v = [F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for _ in range(n)]
        v[0], v[-1] = F.zero, F.from_words([P - 1] * F.limbs)
        a = np.array([F.words(e) for e in v], dtype=np.uint64)              # (n, limbs)
        w0 = F.words(w)[0]
        assert [F.from_words(r) for r in gm.np_ntt(a, w0).tolist()] == gm.ntt(F, w, v)
        assert [F.from_words(r) for r in gm.np_intt(a, w0).tolist()] == gm.intt(F, w, v)
        if F.limbs == 1:                                                    # the (n,) form
            assert gm.np_ntt(a[:, 0], w0).tolist() == gm.ntt(F, w, v)
    assert gm.np_ntt(np.array([5], dtype=np.uint64), 1).tolist() == [5]
