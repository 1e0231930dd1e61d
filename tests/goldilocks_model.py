"""The reference's second FRI instantiation restated with Python integers: M64 = F_p, p = 2^64 - 2^32 + 1 (zkstark/fri.rs:409), and
ExtendedFieldElement<M64, Ip3> = F_p[x] / (x^3 - x + 1) (fri.rs:410-421, algebra/efield.rs).  Holds the arithmetic, the literal
recursive ntt / intt (ntt.rs:7-64), fast_coset_evaluate (ntt.rs:254-269), the leaf bytes, and FRI::prove / FRI::verify
(fri.rs:99-400) over either field.  bincode, the transcript, Merkle and sample_indices come from fri_prove_model.  No GPU, no library.

A base element is an int in [0, p); an extension element is a tuple (c0, c1, c2) of such ints for c0 + c1 x + c2 x^2."""
import numpy as np
import fri_prove_model as fpm

P = (1 << 64) - (1 << 32) + 1
ROOT_2_32 = 1753635133440165772          # get_nth_root_of_m64, fri.rs:449-473: of order 2^32
FIELD_M64, FIELD_M64X3 = 3, 4


class M64:
    fid, limbs, name = FIELD_M64, 1, "M64"
    zero, one = 0, 1

    @staticmethod
    def from_int(v):
        return v % P

    @staticmethod
    def add(a, b):
        return (a + b) % P

    @staticmethod
    def sub(a, b):
        return (a - b) % P

    @staticmethod
    def neg(a):
        return (-a) % P

    @staticmethod
    def mul(a, b):
        return a * b % P

    @staticmethod
    def inv(a):
        return pow(a, P - 2, P)

    @staticmethod
    def words(a):
        return [a]

    @staticmethod
    def from_words(w):
        return int(w[0])

    @staticmethod
    def leaf(a):
        """bincode(FiniteFieldElement): sign byte (0 for zero, else 1), u64 digit count, u32 LE digits"""
        return fpm.leaf(a)


class M64X3:
    fid, limbs, name = FIELD_M64X3, 3, "M64X3"
    zero, one = (0, 0, 0), (1, 0, 0)

    @staticmethod
    def from_int(v):
        return (v % P, 0, 0)

    @staticmethod
    def add(a, b):
        return tuple((x + y) % P for x, y in zip(a, b))

    @staticmethod
    def sub(a, b):
        return tuple((x - y) % P for x, y in zip(a, b))

    @staticmethod
    def neg(a):
        return tuple((-x) % P for x in a)

    @staticmethod
    def mul(a, b):
        d = [0] * 5
        for i in range(3):
            for j in range(3):
                d[i + j] += a[i] * b[j]
        # x^3 = x - 1, x^4 = x^2 - x
        return ((d[0] - d[3]) % P, (d[1] + d[3] - d[4]) % P, (d[2] + d[4]) % P)

    @staticmethod
    def pow(a, e):
        r = M64X3.one
        while e:
            if e & 1:
                r = M64X3.mul(r, a)
            a = M64X3.mul(a, a)
            e >>= 1
        return r

    @staticmethod
    def inv(a):
        """a^(p^3 - 2); inverse(0) = 0.  A base value is inverted in the base field (the same element: F_p* is a subgroup)."""
        if a[1] == 0 and a[2] == 0:
            return (pow(a[0], P - 2, P), 0, 0)
        return M64X3.pow(a, P ** 3 - 2)

    @staticmethod
    def words(a):
        return list(a)

    @staticmethod
    def from_words(w):
        return (int(w[0]), int(w[1]), int(w[2]))

    @staticmethod
    def leaf(a):
        """bincode(ExtendedFieldElement{poly: Polynomial{coef}}): u64 count of coefficients after trimming trailing zeros, then the
        base leaves"""
        k = 3
        while k and a[k - 1] == 0:
            k -= 1
        return fpm.u64le(k) + b"".join(fpm.leaf(c) for c in a[:k])


FIELDS = {FIELD_M64: M64, FIELD_M64X3: M64X3}


def fpow(F, a, e):
    r = F.one
    while e:
        if e & 1:
            r = F.mul(r, a)
        a = F.mul(a, a)
        e >>= 1
    return r


def root_of_unity(F, log2_n):
    """get_nth_root_of_m64: the generator of order 2^32 squared down to order 2^log2_n (a base value, embedded)"""
    assert log2_n <= 32, "Field does not have nth root of unity where n > 2^32 or not power of two."
    r = ROOT_2_32
    for _ in range(32 - log2_n):
        r = r * r % P
    return F.from_int(r)


# ---- ntt.rs ---------------------------------------------------------------------------------------------------------------------
def ntt(F, root, values):
    """ntt.rs:7-48, the literal recursion (primitive_root.pow(i) as a running product)"""
    n = len(values)
    assert n & (n - 1) == 0, "cannot compute ntt of non-power-of-two sequence"
    if n <= 1:
        return list(values)
    assert fpow(F, root, n) == F.one, "primitive root must be nth root of unity, where n is len(values)"
    assert fpow(F, root, n // 2) != F.one, "primitive root is not primitive nth root of unity, where n is len(values)"
    return _ntt(F, root, list(values))


def _ntt(F, root, values):
    n = len(values)
    if n <= 1:
        return values
    half = n // 2
    r2 = F.mul(root, root)
    odds = _ntt(F, r2, values[1::2])
    evens = _ntt(F, r2, values[0::2])
    out, w = [], F.one
    for i in range(n):
        out.append(F.add(evens[i % half], F.mul(w, odds[i % half])))
        w = F.mul(w, root)
    return out


def intt(F, root, values):
    """ntt.rs:50-64"""
    if len(values) == 1:
        return list(values)
    ninv = F.inv(F.from_int(len(values)))
    return [F.mul(ninv, v) for v in ntt(F, F.inv(root), values)]


def fast_coset_evaluate(F, coef, offset, generator, order):
    """ntt.rs:254-269 with Polynomial::scale (coefficient i times offset^i)"""
    assert len(coef) <= order, "attempt to subtract with overflow (order - polynomial.coef.len())"
    scaled, w = [], F.one
    for c in coef:
        scaled.append(F.mul(c, w))
        w = F.mul(w, offset)
    return ntt(F, generator, scaled + [F.zero] * (order - len(coef)))


def poly_eval(F, coef, x):
    acc = F.zero
    for c in reversed(coef):
        acc = F.add(F.mul(acc, x), c)
    return acc


# ---- FRI (fri.rs) ------------------------------------------------------------------------------------------------------------------
def sample(F, byte_array):
    """F::sample: the wrapping usize accumulator taken mod p, embedded in the base field (efield.rs:180-186)"""
    return F.from_int(fpm.sample(byte_array))


def fold(F, cw, alpha, offset, omega):
    """one split-and-fold (fri.rs:182-193): out[i] = 2^-1 ((1 + q) c[i] + (1 - q) c[h + i]), q = alpha / (offset omega^i).  Elementwise, so
    any even length is accepted (the library folds n / 2 pairs whatever n is)."""
    h = len(cw) // 2
    two_inv = F.inv(F.from_int(2))
    out, x = [], offset
    for i in range(h):
        q = F.mul(alpha, F.inv(x))
        s, d = F.add(cw[i], cw[h + i]), F.sub(cw[i], cw[h + i])
        out.append(F.mul(two_inv, F.add(s, F.mul(q, d))))
        x = F.mul(x, omega)
    return out


def prove(F, codeword, omega, offset, expansion_factor, tests):
    """FRI::prove (fri.rs:99-260); the proof dict has fri_prove_model.prove's shape with elements of F"""
    n = len(codeword)
    rounds = fpm.num_rounds(n, expansion_factor, tests)
    assert rounds >= 2
    stream, roots, codewords, trees, alphas = [], [], [], [], []
    cw = list(codeword)
    for r in range(rounds):
        leaves = [F.leaf(v) for v in cw]
        levels = fpm.merkle_levels(leaves)
        root = levels[-1][0]
        roots.append(root)
        stream.append([root])
        codewords.append(cw)
        trees.append((leaves, levels))
        if r == rounds - 1:
            break
        alpha = sample(F, fpm.fiat_shamir(stream))
        alphas.append(alpha)
        cw = fold(F, cw, alpha, offset, omega)
        omega, offset = F.mul(omega, omega), F.mul(offset, offset)
    stream.append([F.leaf(v) for v in cw])
    top = fpm.sample_indices(fpm.fiat_shamir(stream), n // 2, len(cw), tests)
    layers, indices = [], list(top)
    for i in range(rounds - 1):
        half = len(codewords[i]) // 2
        indices = [idx % half for idx in indices]
        a, b = list(indices), [idx + half for idx in indices]
        (lc, vc), (ln, vn) = trees[i], trees[i + 1]
        layers.append({"a": ([codewords[i][j] for j in a], [fpm.merkle_open(j, lc, vc) for j in a]),
                       "b": ([codewords[i][j] for j in b], [fpm.merkle_open(j, lc, vc) for j in b]),
                       "c": ([codewords[i + 1][j] for j in a], [fpm.merkle_open(j, ln, vn) for j in a])})
    return {"top_level_indices": top, "last_codeword": cw, "merkle_roots": roots, "revealed_layers": layers, "alphas": alphas,
            "codewords": codewords}


def _interpolant_degree(F, omega, offset, values):
    """degree of the interpolant through (offset omega^i, values[i]) -- the last codeword's low-degree check (fri.rs:300-318).  The
    domain is a coset of a 2-power subgroup, so the unique interpolant is intt(values) with coefficient i divided by offset^i."""
    coef = intt(F, omega, values)
    d = len(coef) - 1
    while d >= 0 and coef[d] == F.zero:         # offset^-i != 0: the scaling does not move the degree
        d -= 1
    return d


def verify(F, proof, omega, offset, domain_length, expansion_factor, tests, points=None):
    """FRI::verify (fri.rs:262-400)"""
    rounds = fpm.num_rounds(domain_length, expansion_factor, tests)
    roots = proof["merkle_roots"]
    stream, alphas = [], []
    for root in roots:
        stream.append([root])
        alphas.append(sample(F, fpm.fiat_shamir(stream)))
    last = list(proof["last_codeword"])
    stream.append([F.leaf(v) for v in last])
    if fpm.merkle_levels([F.leaf(v) for v in last])[-1][0] != roots[-1]:
        return False
    degree = len(last) // expansion_factor - 1
    last_omega, last_offset = fpow(F, omega, 1 << (rounds - 1)), fpow(F, offset, 1 << (rounds - 1))
    if _interpolant_degree(F, last_omega, last_offset, last) > degree:
        return False
    top = fpm.sample_indices(fpm.fiat_shamir(stream), domain_length >> 1, domain_length >> (rounds - 1), tests)
    if top != proof["top_level_indices"]:
        return False
    for r in range(rounds - 1):
        c_idx = [i % (domain_length >> (r + 1)) for i in top]
        a_idx, b_idx = c_idx, [i + (domain_length >> (r + 1)) for i in c_idx]
        L = proof["revealed_layers"][r]
        for s in range(tests):
            ay, by, cy = L["a"][0][s], L["b"][0][s], L["c"][0][s]
            if r == 0 and points is not None:
                points += [(a_idx[s], ay), (b_idx[s], by)]
            ax, bx, cx = F.mul(offset, fpow(F, omega, a_idx[s])), F.mul(offset, fpow(F, omega, b_idx[s])), alphas[r]
            if F.mul(F.sub(by, ay), F.sub(cx, ax)) != F.mul(F.sub(cy, ay), F.sub(bx, ax)):
                return False
        for s in range(tests):
            if not fpm.merkle_verify(roots[r], a_idx[s], L["a"][1][s], F.leaf(L["a"][0][s])):
                return False
            if not fpm.merkle_verify(roots[r], b_idx[s], L["b"][1][s], F.leaf(L["b"][0][s])):
                return False
            if not fpm.merkle_verify(roots[r + 1], c_idx[s], L["c"][1][s], F.leaf(L["c"][0][s])):
                return False
        omega, offset = F.mul(omega, omega), F.mul(offset, offset)
    return True


# ---- the same field on numpy uint64 arrays ------------------------------------------------------------------------------------------
# For transforms too large for Python integers.  Canonical values (< p) in and out; the operands broadcast.  Checked against Python
# integers in test_goldilocks_model.py.  A transform of M64X3 data with a base-field root is the M64 transform of each of its three
# coefficient columns, so np_ntt over an (n, 3) array serves the extension as well.
_U = np.uint64
_P, _EPS, _M32, _S32 = _U(P), _U((1 << 32) - 1), _U((1 << 32) - 1), _U(32)


def _operands(a, b):
    """at least one dimension: array arithmetic wraps silently, numpy scalars warn"""
    return np.atleast_1d(np.asarray(a, dtype=_U)), np.atleast_1d(np.asarray(b, dtype=_U))


def np_add(a, b):
    a, b = _operands(a, b)
    s = a + b                                             # wraps; a + b < 2 p
    s = s + (s < a).astype(_U) * _EPS                     # 2^64 = 2^32 - 1: the wrapped sum is below 2 p - 2^64, no second carry
    return s - (s >= _P).astype(_U) * _P


def np_sub(a, b):
    a, b = _operands(a, b)
    return (a - b) - (a < b).astype(_U) * _EPS            # a - b + 2^64 - (2^32 - 1) = a - b + p


def np_mul(a, b):
    """four 32 x 32 partial products -> (hi, lo) of the 128-bit product -> lo + hi_lo (2^32 - 1) - hi_hi, by 2^64 = 2^32 - 1 and 2^96 = -1"""
    a, b = _operands(a, b)
    a0, a1, b0, b1 = a & _M32, a >> _S32, b & _M32, b >> _S32
    ll, lh, hl, hh = a0 * b0, a0 * b1, a1 * b0, a1 * b1
    m1 = lh + (ll >> _S32)                                # < 2^64: (2^32 - 1)^2 + 2^32 - 1
    m2 = hl + (m1 & _M32)
    lo = (m2 << _S32) | (ll & _M32)
    hi = hh + (m1 >> _S32) + (m2 >> _S32)
    hi_lo, hi_hi = hi & _M32, hi >> _S32
    t = lo - hi_hi
    t = t - (lo < hi_hi).astype(_U) * _EPS                # borrowed 2^64: the wrapped value is at least 2^64 - 2^32, no second borrow
    u = hi_lo * _EPS
    r = t + u
    r = r + (r < u).astype(_U) * _EPS                     # carried 2^64: the wrapped sum is below 2^64 - 2^32, no second carry
    return r - (r >= _P).astype(_U) * _P


def np_powers(a, n):
    """a^0 .. a^(n-1) by doubling: the first k powers times a^k are the next k"""
    out = np.ones(max(n, 1), dtype=_U)
    k, ak = 1, int(a) % P
    while k < n:
        m = min(k, n - k)
        out[k:k + m] = np_mul(out[:m], _U(ak))
        ak = ak * ak % P
        k *= 2
    return out[:n]


def np_ntt(x, w):
    """X[k] = sum_j x[j] w^(j k), w of order n = len(x): iterative radix 2 (bit-reversal, then decimation-in-time stages), natural
    order in and out, over an (n,) array or column by column over an (n, c) one"""
    x = np.asarray(x, dtype=_U)
    n = x.shape[0]
    assert n and n & (n - 1) == 0, "cannot compute ntt of non-power-of-two sequence"
    if n == 1:
        return x.copy()
    lg = n.bit_length() - 1
    assert pow(int(w), n, P) == 1 and pow(int(w), n // 2, P) == P - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(lg):
        rev |= ((np.arange(n, dtype=np.int64) >> b) & 1) << (lg - 1 - b)
    y = x[rev].reshape(n, -1)
    c = y.shape[1]
    pw = np_powers(w, n // 2)
    m = 1
    while m < n:                                          # blocks of 2 m: (u, v) -> (u + t v, u - t v), t = w_{2m}^j
        y = y.reshape(n // (2 * m), 2, m, c)
        tv = np_mul(y[:, 1], pw[::n // (2 * m)][None, :, None])
        u = y[:, 0]
        y = np.stack([np_add(u, tv), np_sub(u, tv)], axis=1)
        m *= 2
    return y.reshape(x.shape)


def np_intt(x, w):
    """n^-1 times the transform with w^-1 (ntt.rs:50-64)"""
    n = np.asarray(x).shape[0]
    if n == 1:
        return np.asarray(x, dtype=_U).copy()
    return np_mul(np_ntt(x, pow(int(w), P - 2, P)), _U(pow(n, P - 2, P)))
