"""Reed-Solomon over GF(2^8) in Python integers, line for line after algebra/reedsolomon.rs: the model the device codec
(myzkp_amd/csrc/mzk_rs.hip) is compared with, bit for bit.

Two forms of every result that the reference trims:
  * the TRIMMED form is the reference's own: Polynomial subtraction drops trailing zero coefficients, so `encode` returns fewer than
    n symbols whenever the top message bytes are zero (reedsolomon.rs:76-77), the empty list for the zero message;
  * the FIXED form always has n symbols -- what the device writes.  fixed == trimmed, zero-extended (tests/test_rs_model.py).
Decoding works on fixed-length words; `None` is the reference's None."""

POLY = 0x11D          # x^8 + x^4 + x^3 + x^2 + 1 (Ip0x11D, reedsolomon.rs:352-369)
GEN = 2               # the element x (setup_rs1d, reedsolomon.rs:396-403)


def gf_mul_bits(a, b):
    """the definition: shift and add over GF(2), reduced by POLY"""
    r = 0
    while b:
        if b & 1:
            r ^= a
        b >>= 1
        a <<= 1
        if a & 0x100:
            a ^= POLY
    return r


# x generates the multiplicative group, so products go through logarithms (a large code costs the model 10^5 products per word);
# tests/test_rs_model.py holds gf_mul against gf_mul_bits on all 65536 pairs
EXP = [1] * 510
for _i in range(1, 510):
    EXP[_i] = gf_mul_bits(EXP[_i - 1], GEN)
LOG = [0] * 256
for _i in range(255):
    LOG[EXP[_i]] = _i


def gf_mul(a, b):
    return EXP[LOG[a] + LOG[b]] if a and b else 0


def gf_pow(a, e):
    if e == 0:
        return 1
    return EXP[LOG[a] * e % 255] if a else 0


def gf_inv(a):
    assert a != 0
    return gf_pow(a, 254)


def _trim(p):
    p = list(p)
    while p and p[-1] == 0:
        p.pop()
    return p


def poly_mul(a, b):
    if not a or not b:
        return []
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                r[i + j] ^= gf_mul(x, y)
    return _trim(r)


def poly_add(a, b):
    r = [0] * max(len(a), len(b))
    for i, x in enumerate(a):
        r[i] ^= x
    for i, x in enumerate(b):
        r[i] ^= x
    return _trim(r)


def poly_rem(a, g):
    """a mod g, g monic or not (long division from the top)"""
    a, g = _trim(a), _trim(g)
    assert g
    inv = gf_inv(g[-1])
    while len(a) >= len(g):
        f = gf_mul(a[-1], inv)
        s = len(a) - len(g)
        for i, x in enumerate(g):
            a[s + i] ^= gf_mul(f, x)
        a = _trim(a)
    return a


def poly_eval(p, x):
    r = 0
    for c in reversed(p):
        r = gf_mul(r, x) ^ c
    return r


class ReedSolomon:
    def __init__(self, n, k, g=GEN):                                  # reedsolomon.rs:28-32
        assert n >= k, "n must be at least k"
        self.n, self.k, self.d, self.g = n, k, n - k, g

    def evaluation_points(self, el):                                  # :40-48
        return [gf_pow(self.g, i) for i in range(el)]

    def generator_polynomial(self):                                   # :34-37, from_monomials: prod (x - p)
        g = [1]
        for p in self.evaluation_points(self.d):
            g = poly_mul(g, [p, 1])
        return g

    def encode(self, message):                                        # :54-78, the trimmed form
        assert len(message) <= self.k
        shifted = [0] * self.d + list(message)
        rem = poly_rem(shifted, self.generator_polynomial())
        return poly_add(shifted, rem)

    def encode_fixed(self, message):
        c = self.encode(message)
        return c + [0] * (self.n - len(c))

    def compute_syndromes(self, received):                            # :90-102
        pts = self.evaluation_points(self.n)
        out = []
        for j in range(self.d):
            s = 0
            for i, r in enumerate(received):
                s ^= gf_mul(r, gf_pow(pts[i], j))
            out.append(s)
        return out

    def berlekamp_massey(self, syn):                                  # :106-153
        sigma, bb = [1], [1]
        el, m, b = 0, 1, 1
        for n_iter in range(len(syn)):
            d = syn[n_iter]
            for i in range(1, el + 1):
                if i < len(sigma):
                    d ^= gf_mul(sigma[i], syn[n_iter - i])
            if d == 0:
                m += 1
            else:
                t = list(sigma)
                factor = gf_mul(d, gf_inv(b))
                x_m_b = poly_mul([0] * m + [1], bb)
                sigma = poly_add(sigma, poly_mul(x_m_b, [factor]))
                if 2 * el <= n_iter:
                    el = n_iter + 1 - el
                    bb = t
                    b = d
                    m = 1
                else:
                    m += 1
        return sigma

    def correct_errors(self, received):                               # :206-253
        """(corrected word or None, status): status 0 clean, else the number of corrected symbols, 255 for None"""
        assert len(received) <= self.n
        syn = self.compute_syndromes(received)
        if all(s == 0 for s in syn):
            return list(received), 0
        sigma = self.berlekamp_massey(syn)
        pts = self.evaluation_points(self.n)
        positions = [i for i, p in enumerate(pts) if poly_eval(sigma, gf_inv(p)) == 0]
        if len(positions) != len(sigma) - 1:
            return None, 255
        t = (self.n - self.k) // 2
        omega = poly_mul(sigma, _trim(syn))[:2 * t]
        deriv = [c if i % 2 == 1 else 0 for i, c in enumerate(sigma)][1:]      # from_value(i) = i mod 2
        corrected = list(received)
        for pos in positions:
            xi_inv = gf_inv(pts[pos])
            dv = poly_eval(deriv, xi_inv)
            if dv == 0:
                return None, 255
            corrected[pos] ^= gf_mul(gf_mul(pts[pos], poly_eval(omega, xi_inv)), gf_inv(dv))
        return corrected, len(positions)

    def decode(self, received):                                       # :80-86
        corrected, _ = self.correct_errors(received)
        if corrected is None or len(corrected) < self.d:
            return None
        return corrected[self.d:]

    def decode_status(self, received):
        """(corrected, messages, status) in the device's form: a word the reference gives up on (status 255) comes back unchanged"""
        corrected, status = self.correct_errors(received)
        if corrected is None:
            corrected = list(received)
        return corrected, corrected[self.d:], status


def isqrt_ceil(v):
    s = 0
    while s * s < v:
        s += 1
    return s


class ReedSolomon2D:
    """ReedSolomon2D on fixed-length rows: the reference's result wherever its transposes neither truncate nor panic"""

    def __init__(self, col_n, row_n, message_len, g=GEN):             # reedsolomon.rs:263-272
        self.size = isqrt_ceil(message_len)
        self.col = ReedSolomon(col_n, self.size, g)
        self.row = ReedSolomon(row_n, self.size, g)
        self.message_len = message_len

    def encode(self, data):                                           # :274-295
        size = isqrt_ceil(len(data))
        m = [[0] * size for _ in range(size)]
        for i, v in enumerate(data):
            m[i // size][i % size] = v
        rows = [self.row.encode_fixed(r) for r in m]                              # size x row_n
        cols = [self.col.encode_fixed([rows[i][c] for i in range(size)]) for c in range(self.row.n)]      # row_n x col_n
        return [[cols[c][r] for c in range(self.row.n)] for r in range(self.col.n)]

    def decode_status(self, code):                                    # :297-324
        """(data or None, col_status, row_status)"""
        col_n, row_n = self.col.n, self.row.n
        col_dec, col_status = [], []
        for c in range(row_n):
            _, msg, st = self.col.decode_status([code[r][c] for r in range(col_n)])
            col_dec.append(msg)
            col_status.append(st)
        row_dec, row_status = [], []
        for i in range(self.size):
            _, msg, st = self.row.decode_status([col_dec[c][i] for c in range(row_n)])
            row_dec.append(msg)
            row_status.append(st)
        if 255 in col_status or 255 in row_status:
            return None, col_status, row_status
        flat = [v for r in row_dec for v in r]
        return flat[:self.message_len], col_status, row_status

    def decode(self, code):
        return self.decode_status(code)[0]


def setup_rs1d(n, k):
    return ReedSolomon(n, k)


def setup_rs2d(col_n, row_n, message_len):
    return ReedSolomon2D(col_n, row_n, message_len)


def encode_rs1d(message, rs):
    return rs.encode(message)


def decode_rs1d(code, rs):
    return rs.decode(code)


def encode_rs2d(message, rs):
    return rs.encode(message)


def decode_rs2d(code, rs):
    return rs.decode(code)
