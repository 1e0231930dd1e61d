"""Case tables and integer model of BN254 G2 as the device computes it (myzkp_amd/csrc/mzk_g2.h: Fq2 = Fq[u]/(u^2 + 1) on the 29-bit-limb
Montgomery field code, the XYZZ group law over it), used on both sides of the G2 arithmetic probe: tests/test_hostcheck_g2_probe.py
runs every table WHOLE through the host build of the header with the bounds assertions armed (hc_g2_probe), tests/test_gpu_g2_probe.py
runs the same tables through mzk_selftest_g2_probe on the device.  No case is skipped or filtered on either side.

Everything here is Python integers: no call into the oracle, the library or the host build.
  Fq2 add, sub, dbl, mul, sqr   every limb, composed from the exact steps of tests/arith_model.py (limb-wise sums, K p - b, the unique
                                Montgomery quotient) and the exact weak reduction below
  Fq2 inv                       the residue: a inv(a) == 1, inv(0) == 0
  group operations              the affine sum on y^2 = x^3 + 3 / (9 + u) over Python integers, None = infinity
  every Fq of every output      limbs 0 .. 7 below 2^29 and value below the 2.01 p that mzk_g2.h states ("N2"): 100 v < 201 p
The zero tests of the group law run with KMAX = 3 (f2_is_zero): G2_KMAX.  Plain module: no pytest hooks."""
import random
from arith_model import limbs, value, mont_dense, FQ, FR, Mismatch, MASK, W, first_diff

Q = FQ.p
RORD = FR.p                  # the group order
L = 9
F2W, SLOT2, AFF2 = 18, 72, 36
G2_KMAX = 3                  # f2_is_zero: fe_is_zero_mod<QP, 3> on both coefficients

# op codes: MZK_PROBE_G2_* of include/mzk.h
(F2_ADD, F2_SUB, F2_DBL, F2_MUL, F2_SQR, F2_INV, F2_IS_ZERO, G2_MADD, G2_ADD, G2_DBL, G2_DBL_AFFINE, G2_TO_AFFINE, G2_SCALAR_MUL,
 G2_STORE_LOAD) = range(14)
G2_NAMES = ("f2_add", "f2_sub", "f2_dbl", "f2_mul", "f2_sqr", "f2_inv", "f2_is_zero", "madd", "add", "dbl", "dbl_affine", "to_affine",
            "scalar_mul", "store_load")
F2_OPS = tuple(range(F2_ADD, F2_IS_ZERO + 1))
GROUP_OPS = tuple(range(G2_MADD, G2_STORE_LOAD + 1))


def a_words(op):
    return F2W if op in F2_OPS else AFF2 if op in (G2_DBL_AFFINE, G2_SCALAR_MUL) else SLOT2


def b_words(op):
    return F2W if op in (F2_ADD, F2_SUB, F2_MUL) else AFF2 if op == G2_MADD else SLOT2 if op == G2_ADD else 0


def out_words(op):
    return F2W if op in F2_OPS else SLOT2


# ---- Fq2 = Fq[u] / (u^2 + 1) on integers: (c0, c1) ----------------------------------------------------------------------------------
def f2_add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2_sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2_neg(a):
    return ((-a[0]) % Q, (-a[1]) % Q)


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_scale(a, k):
    return (a[0] * k % Q, a[1] * k % Q)


def f2_inv(a):
    ni = pow((a[0] * a[0] + a[1] * a[1]) % Q, -1, Q)       # -1 is a non-residue (q = 3 mod 4): the norm of a non-zero a is non-zero
    return (a[0] * ni % Q, (-a[1]) * ni % Q)


F2_ZERO, F2_ONE = (0, 0), (1, 0)
B2 = f2_scale(f2_inv((9, 1)), 3)                            # the twist: y^2 = x^3 + 3 / (9 + u)
G2_GEN = ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
           11559732032986387107991004021392285783925812861821192530917403151452391805634),
          (8495653923123431417604973247489272438418190587263600148770280649306958101930,
           4082367875863433681332203403145435568316851327593401208105741076214120093531))


def aff2_neg(P):
    return None if P is None else (P[0], f2_neg(P[1]))


def aff2_add(P1, P2):
    """short Weierstrass over Fq2, a = 0, None = infinity"""
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if f2_add(y1, y2) == F2_ZERO:
            return None
        lam = f2_mul(f2_scale(f2_mul(x1, x1), 3), f2_inv(f2_scale(y1, 2)))
    else:
        lam = f2_mul(f2_sub(y2, y1), f2_inv(f2_sub(x2, x1)))
    x3 = f2_sub(f2_sub(f2_mul(lam, lam), x1), x2)
    return (x3, f2_sub(f2_mul(lam, f2_sub(x1, x3)), y1))


def aff2_mul(P, k):
    acc = None
    while k:
        if k & 1:
            acc = aff2_add(acc, P)
        P = aff2_add(P, P)
        k >>= 1
    return acc


def on_curve2(P):
    return P is None or f2_sub(f2_mul(P[1], P[1]), f2_add(f2_mul(f2_mul(P[0], P[0]), P[0]), B2)) == F2_ZERO


# ---- forms ---------------------------------------------------------------------------------------------------------------------
def mont(v):
    return v * FQ.R % Q


def mont2_limbs(a, j=(0, 0)):
    """an Fq2 value in Montgomery form, coefficient c stored as its canonical value + j[c] p: 18 limbs"""
    out = []
    for v, jj in zip(a, j):
        v = mont(v) + jj * Q
        assert 100 * v < 201 * Q
        out += limbs(v, L)
    return out


def affine2_limbs(P):
    """an affine operand: x then y, 36 limbs, canonical Montgomery"""
    return mont2_limbs(P[0]) + mont2_limbs(P[1])


def slot2_of(P, z, j=(0,) * 8):
    """the raw slot of P in the representation (x z^2, y z^3, z^2, z^3), z in Fq2*, Montgomery form, coordinate-major, c0 then c1, each
    of the 8 Fq coefficients stored as canonical + j p (j in {0, 1}: both inside N2); None -> the all-zero slot"""
    if P is None:
        return [0] * SLOT2
    assert z != F2_ZERO
    z2 = f2_mul(z, z)
    z3 = f2_mul(z2, z)
    out = []
    for c, v in enumerate((f2_mul(P[0], z2), f2_mul(P[1], z3), z2, z3)):
        out += mont2_limbs(v, j[2 * c:2 * c + 2])
    return out


def f2_of(w):
    """the integer pair an 18-limb operand holds (raw values, not reduced)"""
    return (value(w[:L]), value(w[L:2 * L]))


def slot2_coords(s):
    return [f2_of(s[F2W * c:F2W * c + F2W]) for c in range(4)]


def _red(a):
    return (a[0] % Q, a[1] % Q)


def slot2_point(s):
    """the group element a slot holds (None = infinity; raises if ZZ^3 != ZZZ^2)"""
    X, Y, ZZ, ZZZ = [_red(c) for c in slot2_coords(s)]
    if ZZ == F2_ZERO:
        return None
    iR = pow(FQ.R, -1, Q)
    zz, zzz = f2_scale(ZZ, iR), f2_scale(ZZZ, iR)
    if f2_mul(f2_mul(zz, zz), zz) != f2_mul(zzz, zzz):
        raise Mismatch("ZZ^3 != ZZZ^2")
    return (f2_mul(X, f2_inv(ZZ)), f2_mul(Y, f2_inv(ZZZ)))         # the Montgomery factors cancel


def wire_words(P):
    """g2_store_plain: x.c0 | x.c1 | y.c0 | y.c1, 8 canonical plain words each; infinity all-zero"""
    if P is None:
        return [0] * 32
    return [(v >> (32 * i)) & 0xffffffff for v in (P[0][0], P[0][1], P[1][0], P[1][1]) for i in range(8)]


def scalar_words(k):
    return [(k >> (32 * i)) & 0xffffffff for i in range(8)]


# ---- the exact steps ----------------------------------------------------------------------------------------------------------------
KP8 = FQ.kp(8)
QS = 52
QM = (1 << QS) // (FQ.PT + 1)          # tools/gen_constants.py: the quotient estimate of fe_weak_reduce / fe_reduce
assert QM == 0x54a4736b


def m_add(a, b):
    """fe_add: limb-wise"""
    return [x + y for x, y in zip(a, b)]


def m_sub8(a, b):
    """fe_sub<8>: a + (8 p - b) limb-wise on the borrow-friendly limbs of 8 p"""
    assert all(c >= y for c, y in zip(KP8, b))
    return [x + c - y for x, c, y in zip(a, KP8, b)]


def m_neg8(b):
    """fe_neg_lazy<8>"""
    return [c - y for c, y in zip(KP8, b)]


def m_weak(a):
    """fe_weak_reduce, exactly: carry, q = floor(top QM / 2^QS), x - q p (never negative: q <= floor(x / p))"""
    v = value(a)
    q = ((v >> (W * (L - 1))) * QM) >> QS
    assert v - q * Q >= 0
    return limbs(v - q * Q, L)


def m_mul_add2(a, b, c, d):
    return mont_dense(FQ, value(a) * value(b) + value(c) * value(d))


def _c(w):
    return w[:L], w[L:2 * L]


def f2m_add(a, b):
    (a0, a1), (b0, b1) = _c(a), _c(b)
    return m_weak(m_add(a0, b0)) + m_weak(m_add(a1, b1))


def f2m_sub(a, b):
    (a0, a1), (b0, b1) = _c(a), _c(b)
    return m_weak(m_sub8(a0, b0)) + m_weak(m_sub8(a1, b1))


def f2m_mul(a, b):
    (a0, a1), (b0, b1) = _c(a), _c(b)
    return m_mul_add2(a0, b0, m_neg8(a1), b1) + m_mul_add2(a0, b1, a1, b0)


def f2m_expected(op, a, b):
    if op == F2_ADD:
        return f2m_add(a, b)
    if op == F2_SUB:
        return f2m_sub(a, b)
    if op == F2_DBL:
        return f2m_add(a, a)
    if op == F2_MUL:
        return f2m_mul(a, b)
    if op == F2_SQR:
        return f2m_mul(a, a)
    raise ValueError(op)


# ---- judgement ---------------------------------------------------------------------------------------------------------------------
def _hex(w):
    return None if w is None else [hex(int(x)) for x in w]


def _fail(op, case, out, why, limb=None):
    raise Mismatch("G2 %s class=%s: %s%s\n  a: %s\n  b: %s\n  k: %s\n  result: %s" % (
        G2_NAMES[op], case["cls"], why, "" if limb is None else " (first bad limb %d)" % limb, _hex(case["a"]), _hex(case.get("b")),
        _hex(case.get("k")), _hex(out)))


def _n2(op, case, out, nfe):
    """every Fq of an output is N2: limbs 0 .. 7 below 2^29, value below 2.01 p (the header's number)"""
    for c in range(nfe):
        co = out[L * c:L * c + L]
        for i in range(L - 1):
            if co[i] > MASK:
                _fail(op, case, out, "Fq %d: limb not below 2^29" % c, L * c + i)
        if 100 * value(co) >= 201 * Q:
            _fail(op, case, out, "Fq %d not below 2.01 p (%.4f p)" % (c, value(co) / Q), L * c + L - 1)


def check_f2(op, case, out):
    """out: the 18 result limbs of an Fq2 op"""
    out = [int(x) for x in out]
    a, b = case["a"], case.get("b")
    if op == F2_IS_ZERO:
        va = f2_of(a)
        want = 1 if all(v % Q == 0 and v // Q <= G2_KMAX for v in va) else 0
        d = first_diff(out, [want] + [0] * (F2W - 1))
        if d is not None:
            _fail(op, case, out, "expected %d" % want, d)
        return
    _n2(op, case, out, 2)
    if op == F2_INV:
        x = _red(f2_of(a))
        got = _red(f2_of(out))
        if x == F2_ZERO:
            if got != F2_ZERO:
                _fail(op, case, out, "inv(0) != 0", 0 if got[0] else L)
            return
        # raw x = a R  ->  a^-1 R = x^-1 R^2
        want = f2_scale(f2_inv(x), FQ.R * FQ.R % Q)
        if got != want:
            _fail(op, case, out, "a inv(a) != 1", 0 if got[0] != want[0] else L)
        return
    want = f2m_expected(op, a, b)
    d = first_diff(out, want)
    if d is not None:
        _fail(op, case, out, "expected limbs %s" % _hex(want), d)
    # the composed steps are Fq2 arithmetic: one more look at the residue
    va, vb, vo = _red(f2_of(a)), _red(f2_of(b)) if b is not None else None, _red(f2_of(out))
    iR = pow(FQ.R, -1, Q)
    res = {F2_ADD: lambda: f2_add(va, vb), F2_SUB: lambda: f2_sub(va, vb), F2_DBL: lambda: f2_add(va, va),
           F2_MUL: lambda: f2_scale(f2_mul(va, vb), iR), F2_SQR: lambda: f2_scale(f2_mul(va, va), iR)}[op]()
    if vo != res:
        _fail(op, case, out, "wrong residue in Fq2", 0 if vo[0] != res[0] else L)


def g2_expected(op, case):
    A = case["A"]
    if op in (G2_MADD, G2_ADD):
        return aff2_add(A, case["B"])
    if op in (G2_DBL, G2_DBL_AFFINE):
        return aff2_add(A, A)
    if op == G2_SCALAR_MUL:
        return aff2_mul(A, case["K"])
    return A


def check_g2(op, case, out, want="compute"):
    """out: the 72 result words of a group op, against the affine expectation (`want`, by default computed from the case)"""
    out = [int(x) for x in out]
    if want == "compute":
        want = g2_expected(op, case)
    if op == G2_TO_AFFINE:
        d = first_diff(out, wire_words(want) + [0] * (SLOT2 - 32))
        if d is not None:
            _fail(op, case, out, "expected the wire words %s" % _hex(wire_words(want)), d)
        return
    _n2(op, case, out, 8)
    zero = not any(out)
    if want is None:
        if not zero:
            _fail(op, case, out, "expected infinity as the all-zero slot", [i for i, x in enumerate(out) if x][0])
        return
    if zero:
        _fail(op, case, out, "all-zero slot (infinity) for a finite result", 0)
    try:
        got = slot2_point(out)
    except Mismatch as e:
        _fail(op, case, out, str(e), 2 * F2W)
    if got is None:
        _fail(op, case, out, "ZZ == 0 (mod p) in a non-zero slot", 2 * F2W)
    if got != want:
        _fail(op, case, out, "wrong group element: expected %s, got %s" % (want, got), 0 if got[0] != want[0] else F2W)
    if op == G2_STORE_LOAD:
        ref = []
        for c in slot2_coords(case["a"]):
            ref += limbs(c[0] % Q, L) + limbs(c[1] % Q, L)
        d = first_diff(out, ref)
        if d is not None:
            _fail(op, case, out, "a coefficient is not the canonical value of the one stored", d)


# ---- the exceptional branches ------------------------------------------------------------------------------------------------------
# When the operands share x, P = f2_sub(U2, U1) and (same point) R = f2_sub(S2, S1) are, per coefficient,
#     fe_weak_reduce(U2 + 8 p - U1)        with U2 == U1 (mod p).
# BEFORE the reduction the sum is a multiple (8 + u2 - u1) p:
#   add:  U1, U2 are Fq2 products, each coefficient what fe_mul_add2 returns: < (a b + c d) / R + p.  With N2 operands (< 2.01 p) and
#         the lazy 8 p - a.c1 of f2_mul, (a b + c d) / R < (2.01^2 + 8 * 2.01) p^2 / R = 20.2 * 0.0059 p < 0.12 p, so a coefficient is
#         canonical + u p with u in {0, 1}, u = 1 only for a canonical part below 0.12 p.  The canonical parts of U1 and U2 are
#         equal, so the sum is (8 + u2 - u1) p: 7, 8 or 9.
#   madd: U1 is the stored a.X: canonical + j p, j in {0, 1} (N2); U2 = q.x a.ZZ is a product: 8 + u - j: 7, 8 or 9.  R likewise.
# fe_weak_reduce then takes q = floor(top QM / 2^52) multiples of p away, top the carried limb 8.  p / 2^232 = PT + 0.449, so the top limb
# of k p is k PT + floor(0.449 k) and q = floor((k PT + floor(0.449 k)) / (PT + 1)) = k - 1 for every k from 1 to far beyond 9 (k < PT
# / 2): the weak reduction of k p is exactly p.  So each coefficient of P and of R, as f2_is_zero sees it, is 1 p, for every one of
# the three sums before it -- the zero test never meets 0 p with non-zero operands, nor 2 p or 3 p, and KMAX = 3 has room to spare.
# The table therefore searches representations until 7, 8 and 9 have each occurred BEFORE the reduction, in c0 and in c1, of P and
# of R, with cases whose c0 and c1 differ, and asserts that what f2_is_zero then sees is G2_K_EXPECTED.
G2_K_PRE_EXPECTED = {7, 8, 9}
G2_K_EXPECTED = {1}
COVER_KEYS = ("P.c0", "P.c1", "R.c0", "R.c1")


def g2_diff_multiples(op, a_slot, b):
    """{"P.c0": (k before the weak reduction, k after), ...}: the multiples of p that the coefficients of P and R are when the operands
    share x, as the code computes them (exact limb model); None where a difference is not a multiple of p"""
    aX, aY, aZZ, aZZZ = [a_slot[F2W * c:F2W * c + F2W] for c in range(4)]
    if op == G2_ADD:
        bX, bY, bZZ, bZZZ = [b[F2W * c:F2W * c + F2W] for c in range(4)]
        U1, U2, S1, S2 = f2m_mul(aX, bZZ), f2m_mul(bX, aZZ), f2m_mul(aY, bZZZ), f2m_mul(bY, aZZZ)
    else:
        U1, U2, S1, S2 = aX, f2m_mul(b[:F2W], aZZ), aY, f2m_mul(b[F2W:], aZZZ)
    out = {}
    for nm, lo, hi in (("P", U1, U2), ("R", S1, S2)):
        for c in range(2):
            x, y = _c(lo)[c], _c(hi)[c]
            pre, post = value(m_sub8(y, x)), value(m_weak(m_sub8(y, x)))
            assert pre == value(y) + 8 * Q - value(x)
            out["%s.c%d" % (nm, c)] = (pre // Q, post // Q) if pre % Q == 0 else None
    return out


# ---- tables ------------------------------------------------------------------------------------------------------------------------
def _n2max():
    return (201 * Q - 1) // 100          # the largest v with 100 v < 201 p


def _edge_fq():
    """(class, raw value) of an N2 coefficient"""
    p = Q
    return [("0", 0), ("1", 1), ("p-1", p - 1), ("p", p), ("p+1", p + 1), ("2p-1", 2 * p - 1), ("2p", 2 * p), ("2p+1", 2 * p + 1),
            ("2.01p", _n2max()), ("R mod p", FQ.R % p), ("2^232", 1 << (W * (L - 1))), ("limbs all-ones", (1 << (W * (L - 1))) - 1)]


def _rand_fq(rng):
    k = rng.randrange(4)
    if k == 0:
        return rng.randrange(Q)
    if k == 1:
        return Q + rng.randrange(Q)
    return rng.randrange(_n2max() + 1)


def _w2(c0, c1):
    return limbs(c0, L) + limbs(c1, L)


def f2_table(op, seed=1, nrand=600):
    """cases of an Fq2 op: {"cls", "a": 18 limbs, "b": 18 limbs or None}; operands are N2, the contract of mzk_g2.h"""
    rng = random.Random((seed << 8) ^ (0x200 + op))
    p = Q
    cases = []
    binary = op in (F2_ADD, F2_SUB, F2_MUL)

    def add(cls, a, b=None):
        cases.append({"cls": cls, "a": [int(x) for x in a], "b": None if b is None else [int(x) for x in b]})

    E = _edge_fq()
    if op == F2_IS_ZERO:
        # each coefficient k p for every k the IS_ZERO_MOD tables use relative to their KMAX (0 .. KMAX + 2), here KMAX = 3
        nz = (12345, p - 1, 2 * p + 99, 1 << 29, 1 << (W * (L - 1)))
        for k0 in range(G2_KMAX + 3):
            for k1 in range(G2_KMAX + 3):
                add("(%dp, %dp)" % (k0, k1), _w2(k0 * p, k1 * p))
                for e in (1, -1):
                    if k0 or e > 0:
                        add("(%dp%+d, %dp)" % (k0, e, k1), _w2(k0 * p + e, k1 * p))
                    if k1 or e > 0:
                        add("(%dp, %dp%+d)" % (k0, k1, e), _w2(k0 * p, k1 * p + e))
                # same limb 0 as a multiple: past the filter on limb 0, into the full reduction
                add("(%dp+2^29, %dp)" % (k0, k1), _w2(k0 * p + (1 << W), k1 * p))
                add("(%dp, %dp+2^232)" % (k0, k1), _w2(k0 * p, k1 * p + (1 << (W * (L - 1)))))
            for v in nz:
                add("(%dp, nonzero)" % k0, _w2(k0 * p, v))
                add("(nonzero, %dp)" % k0, _w2(v, k0 * p))
        for k in range(nrand):
            c0 = rng.randrange(G2_KMAX + 3) * p if k % 2 else rng.randrange(5 * p)
            c1 = rng.randrange(G2_KMAX + 3) * p if k % 3 else rng.randrange(5 * p)
            add("random", _w2(c0, c1))
        return cases
    if op == F2_INV:
        for k0 in range(3):
            for k1 in range(3):
                add("zero as (%dp, %dp)" % (k0, k1), _w2(k0 * p, k1 * p))
    n = len(E)
    for i, (ca, va) in enumerate(E):
        for j, (cb, vb) in enumerate(E):
            if binary:
                (cc, vc), (cd, vd) = E[(i + 3 * j + 1) % n], E[(2 * i + j + 5) % n]
                add("(%s, %s) . (%s, %s)" % (ca, cb, cc, cd), _w2(va, vb), _w2(vc, vd))
            else:
                add("(%s, %s)" % (ca, cb), _w2(va, vb))
    if binary:
        for ca, va in E:          # every edge against itself and against the widest operand, in both coefficients
            add("(%s, %s) . itself" % (ca, ca), _w2(va, va), _w2(va, va))
            add("(%s, %s) . (2.01p, 2.01p)" % (ca, ca), _w2(va, va), _w2(_n2max(), _n2max()))
            add("(2.01p, 2.01p) . (%s, %s)" % (ca, ca), _w2(_n2max(), _n2max()), _w2(va, va))
    if op in (F2_ADD, F2_SUB, F2_DBL):
        # the quotient estimate of the weak reduction reads the carried top limb alone: q = floor(top QM / 2^52) steps where top passes
        # a multiple of PT + 1.  Sums whose top limb is m (PT + 1) + t, t = -2 .. 3, with random limbs below: the estimate is one lower
        # on one side of each step, and a sum formed on another multiple of p (a + 4 p - b, say) comes out a whole p apart here
        top1 = FQ.PT + 1
        for m in ((7, 8, 9) if op == F2_SUB else (1, 2, 3, 4)):
            for t in range(-2, 4):
                for rep in range(3):
                    vs = [((m * top1 + t) << (W * (L - 1))) + (rng.randrange(1 << (W * (L - 1))) & ~1) for _ in range(2)]
                    if op == F2_SUB:          # a + 8 p - b = v
                        bs = [rng.randrange(max(0, 8 * p - v), min(_n2max(), _n2max() + 8 * p - v) + 1) for v in vs]
                        as_ = [v - 8 * p + b for v, b in zip(vs, bs)]
                    else:                     # a + b = v
                        as_ = [v // 2 for v in vs]
                        bs = [v - a for v, a in zip(vs, as_)]
                    assert all(0 <= x <= _n2max() for x in as_ + bs), (m, t)
                    add("sum with top limb %d (PT+1) %+d" % (m, t), _w2(*as_), _w2(*bs) if binary else None)
    for k in range(nrand):
        a = _w2(_rand_fq(rng), _rand_fq(rng))
        add("random", a, _w2(_rand_fq(rng), _rand_fq(rng)) if binary else None)
    return cases


_POOL = {}


def g2_points(seed, n):
    """n points d G2, d random: the pool the tables draw from (cached: a scalar multiplication on integers is milliseconds)"""
    key = (seed, n)
    if key not in _POOL:
        rng = random.Random(0x6732 ^ seed)
        _POOL[key] = [aff2_mul(G2_GEN, rng.randrange(1, RORD)) for _ in range(n)]
    return list(_POOL[key])


def _rand_z(rng):
    return (rng.randrange(1, Q), rng.randrange(1, Q))


def _z_kinds(rng):
    return [("z=1", F2_ONE), ("z random", _rand_z(rng)), ("z.c0=0", (0, rng.randrange(1, Q))), ("z.c1=0", (rng.randrange(2, Q), 0))]


def _rand_j(rng):
    return tuple(rng.randrange(2) for _ in range(8))


def _jxy(m, tail):
    """j pattern number m (0 .. 15) on the four coefficients of X and Y; ZZ and ZZZ take `tail`"""
    return tuple((m >> i) & 1 for i in range(4)) + tuple(tail)


def g2_table(op, seed=1, nrand=600, search=40000):
    """cases of a group op: {"cls", "a": slot or affine limbs, "b": affine limbs / slot / None, "k": 8 words / None, "A", "B": the
    affine points (None = infinity), "K": the scalar}, and the coverage of the exceptional branches: {"pre" / "post": {"P.c0" ...: set
    of multiples of p before / after the weak reduction}, "mixed": cases whose c0 and c1 were different multiples}"""
    rng = random.Random((seed << 8) ^ (0x300 + op))
    pool = g2_points(seed, 12)
    pts = pool[:7] + [G2_GEN]
    cases, cover = [], {}

    def add(cls, a, b, A, B, K=None):
        cases.append({"cls": cls, "a": a, "b": b, "k": None if K is None else scalar_words(K), "A": A, "B": B, "K": K})

    def walk(n):
        """n further points, one affine addition each"""
        out, P = [], pool[8]
        for i in range(n):
            P = aff2_add(P, pool[i % 8])
            out.append(P)
        return out

    if op == G2_SCALAR_MUL:
        # k canonical here: canonicalising is the kernel's job (k_g2_pair_mul), tested on the kernels
        r = RORD
        special = [0, 1, 2, 3, r - 1, r - 2, 1 << 253, (1 << 253) - 1, (1 << 253) | 1, ((1 << 253) - 1) // 3, 2 * (((1 << 253) - 1) // 3),
                   1 << 252, 1 << 31, 1 << 32, (1 << 32) - 1, 1 << 64, r >> 1]
        assert all(0 <= k < r for k in special)
        for P, nm in ((G2_GEN, "generator"), (pool[0], "point")):
            for k in special:
                add("%s k=%s" % (nm, hex(k)), affine2_limbs(P), None, P, None, k)
        for i in range(64):
            P = (G2_GEN, pool[1], pool[2], pool[3])[i % 4]
            add("random k", affine2_limbs(P), None, P, None, rng.randrange(r))
        return cases, cover
    if op == G2_DBL_AFFINE:
        for P in pts + pool[8:] + walk(nrand):
            add("generator" if P == G2_GEN else "point", affine2_limbs(P), None, P, None)
        return cases, cover
    if op in (G2_DBL, G2_TO_AFFINE, G2_STORE_LOAD):
        add("infinity", slot2_of(None, F2_ONE), None, None, None)
        for i, P in enumerate(pts):
            for zc, z in _z_kinds(rng):
                for m in range(16):
                    add("%s%s jXY=%x" % ("generator " if P == G2_GEN else "", zc, m), slot2_of(P, z, _jxy(m, [(m + i + t) & 1 for t in range(4)])), None, P, None)
        for P in walk(nrand // 2):
            add("random", slot2_of(P, _rand_z(rng), _rand_j(rng)), None, P, None)
        if op == G2_DBL:
            # x2_dbl's U == 0 exit cannot be reached from the prime-order group: one OFF-CURVE slot with Y == 0, in each representation of 0
            for m in range(1, 4):
                s = slot2_of(pts[0], _rand_z(rng))
                s[F2W:2 * F2W] = _w2((m & 1) * Q, (m >> 1) * Q)
                add("off-curve, completeness branch", s, None, None, None)
            s = slot2_of(pts[0], _rand_z(rng))
            s[F2W:2 * F2W] = _w2(0, 0)
            add("off-curve, completeness branch", s, None, None, None)
        return cases, cover

    assert op in (G2_MADD, G2_ADD)
    affine_b = op == G2_MADD

    def bform(B, zb=None, jb=(0,) * 8):
        if affine_b:
            return affine2_limbs(B)
        return slot2_of(B, zb if zb is not None else _rand_z(rng), jb)

    inf = slot2_of(None, F2_ONE)
    for i, A in enumerate(pts):
        others = [("another point", pts[(i + 3) % len(pts)]), ("the same point", A), ("its negative", aff2_neg(A)), ("the generator", G2_GEN)]
        for zc, z in _z_kinds(rng):
            for m in range(16):
                a = slot2_of(A, z, _jxy(m, [(m + i + t) & 1 for t in range(4)]))
                for cb, B in others:
                    add("%s %s jXY=%x" % (cb, zc, m), a, bform(B, None, _rand_j(rng)), A, B)
        if affine_b:
            add("infinity + q", inf, affine2_limbs(A), None, A)
        else:
            z = _rand_z(rng)
            add("a + infinity", slot2_of(A, z, _rand_j(rng)), inf, A, None)
            add("infinity + b", inf, slot2_of(A, z, _rand_j(rng)), None, A)
            add("b with z = 1", slot2_of(pts[(i + 2) % len(pts)], _rand_z(rng)), slot2_of(A, F2_ONE), pts[(i + 2) % len(pts)], A)
    if not affine_b:
        add("infinity + infinity", inf, inf, None, None)
    # the exceptional branches: search representations until every multiple has occurred before the reduction, in every coefficient
    cover = {"pre": {k: set() for k in COVER_KEYS}, "post": {k: set() for k in COVER_KEYS}, "mixed": 0}
    mixed_seen = set()
    tries = 0

    def done():
        return all(cover["pre"][k] == G2_K_PRE_EXPECTED for k in COVER_KEYS) and len(mixed_seen) >= 6

    while not done() and tries < search:
        tries += 1
        A = pts[tries % len(pts)]
        same = bool(tries & 1)
        B = A if same else aff2_neg(A)
        a = slot2_of(A, _rand_z(rng), _rand_j(rng))
        b = bform(B, None, _rand_j(rng))
        ks = g2_diff_multiples(op, a, b)
        assert ks["P.c0"] is not None and ks["P.c1"] is not None
        assert (ks["R.c0"] is not None and ks["R.c1"] is not None) == same
        keys = COVER_KEYS if same else COVER_KEYS[:2]
        new = any(ks[k][0] not in cover["pre"][k] for k in keys)
        pairs = [("P", ks["P.c0"][0], ks["P.c1"][0])] + ([("R", ks["R.c0"][0], ks["R.c1"][0])] if same else [])
        mixed = [pr for pr in pairs if pr[1] != pr[2]]
        if any(pr not in mixed_seen for pr in mixed) and len(mixed_seen) < 12:
            new = True
        if new:
            for k in keys:
                cover["pre"][k].add(ks[k][0])
                cover["post"][k].add(ks[k][1])
            mixed_seen.update(mixed)
            cover["mixed"] += bool(mixed)
            add("exceptional %s %s" % ("doubling" if same else "cancelling", " ".join("%s=%dp" % (k, ks[k][0]) for k in keys)), a, b, A, B)
    for k in range(nrand):
        A, B = rng.choice(pool), rng.choice(pool)
        if k % 16 == 0:
            B = A if k % 32 else aff2_neg(A)
        add("random" if k % 16 else "random, equal or opposite", slot2_of(A, _rand_z(rng), _rand_j(rng)), bform(B, None, _rand_j(rng)), A, B)
    return cases, cover


def assert_cover(op, cover):
    """the coverage conditions of the exceptional branches: every multiple before the reduction, exactly G2_K_EXPECTED after it, none
    above the KMAX the code passes, and cases whose c0 and c1 are different multiples"""
    assert bool(cover) == (op in (G2_MADD, G2_ADD))
    if not cover:
        return
    for k in COVER_KEYS:
        assert cover["pre"][k] == G2_K_PRE_EXPECTED, (G2_NAMES[op], k, cover["pre"][k])
        assert cover["post"][k] == G2_K_EXPECTED, (G2_NAMES[op], k, cover["post"][k])
        assert max(cover["post"][k]) <= G2_KMAX
    assert cover["mixed"] >= 6, (G2_NAMES[op], cover["mixed"])


def pack(cases, key):
    import numpy as np
    if cases[0].get(key) is None:
        return None
    return np.array([c[key] for c in cases], dtype=np.uint32)


# ---- chains: each step's output slot is the next step's input ------------------------------------------------------------------------
def sum_tree(run, slots, points):
    """128 slots folded by x2_add in the order k_g2_sum folds them (slot i += slot i + off, off = 64, 32 .. 1), every level judged;
    run(op, cases) -> outputs.  Returns the final (slot, point)."""
    assert len(slots) == len(points) == 128
    slots, points = [list(s) for s in slots], list(points)
    off = 64
    while off >= 1:
        cases = [{"cls": "tree off=%d lane %d" % (off, i), "a": slots[i], "b": slots[i + off], "k": None, "A": points[i], "B": points[i + off], "K": None}
                 for i in range(off)]
        out = run(G2_ADD, cases)
        for i, (c, o) in enumerate(zip(cases, out)):
            check_g2(G2_ADD, c, o)
            slots[i], points[i] = [int(x) for x in o], g2_expected(G2_ADD, c)
        off >>= 1
    return slots[0], points[0]


def run_chains(run, chains=8, seed=5):
    """the three chains of the probe tests, on any runner: 32 mixed additions with the start point coming back every fifth step,
    alternating with its negative; 17 doublings; the sum tree over random points and over equal points (every level doubles)"""
    rng = random.Random(seed)
    pool = g2_points(1, 12)
    pts = [pool[i % len(pool)] for i in range(chains)]
    state = [(slot2_of(P, _rand_z(rng), _rand_j(rng)), P) for P in pts]
    for s in range(32):
        cases = []
        for k, (a, A) in enumerate(state):
            B = pool[(k + s + 1) % len(pool)]
            if s % 5 == 0:
                B = pts[k] if (s // 5) % 2 == 0 else aff2_neg(pts[k])
            cases.append({"cls": "madd chain %d step %d" % (k, s), "a": a, "b": affine2_limbs(B), "k": None, "A": A, "B": B, "K": None})
        out = run(G2_MADD, cases)
        for c, o in zip(cases, out):
            check_g2(G2_MADD, c, o)
        state = [([int(x) for x in o], g2_expected(G2_MADD, c)) for c, o in zip(cases, out)]
    state = [(slot2_of(P, _rand_z(rng), _rand_j(rng)), P) for P in pts]
    for s in range(17):
        cases = [{"cls": "dbl chain %d step %d" % (k, s), "a": a, "b": None, "k": None, "A": A, "B": None, "K": None} for k, (a, A) in enumerate(state)]
        out = run(G2_DBL, cases)
        for c, o in zip(cases, out):
            check_g2(G2_DBL, c, o)
        state = [([int(x) for x in o], g2_expected(G2_DBL, c)) for c, o in zip(cases, out)]
    P, tp = pool[8], []
    for i in range(128):
        P = aff2_add(P, pool[i % 8])
        tp.append(P)
    _, top = sum_tree(run, [slot2_of(T, _rand_z(rng), _rand_j(rng)) for T in tp], tp)
    acc = None
    for T in tp:
        acc = aff2_add(acc, T)
    assert top == acc
    E = pool[9]
    s, top = sum_tree(run, [slot2_of(E, _rand_z(rng), _rand_j(rng)) for _ in range(128)], [E] * 128)
    assert top == aff2_mul(E, 128)
    # and with one stored record for all 128, as k_g2_sum meets equal records: identical representatives at every level
    s0 = slot2_of(E, _rand_z(rng))
    _, top = sum_tree(run, [s0] * 128, [E] * 128)
    assert top == aff2_mul(E, 128)
