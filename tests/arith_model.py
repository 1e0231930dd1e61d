"""Case table and integer model of the device arithmetic (myzkp_amd/csrc/mzk_field.h, mzk_field_asm.h, mzk_ec.h, mzk_coop.h,
mzk_row.h), used on both sides of the arithmetic probe: tests/test_hostcheck_probe.py runs the WHOLE table through the host build
of the headers with every bounds assertion armed, tests/test_gpu_arith_probe.py runs it through mzk_selftest_field_probe /
mzk_selftest_g1_probe on the device.  No case is skipped or filtered on either side.

Everything here is Python integers: no call into the oracle, the library or the host build.  The operand sets are built from the
callers' own steps (K p - b limb-wise, uncarried sums, doubled limbs, the accumulator representations canonical + j p), and the
expectations are exact wherever the arithmetic is:
  dense Montgomery products    every limb: the normalised limbs of (T + m p) / R, m = -T p^-1 mod R (the quotient is unique)
  sparse products (M128)       every limb, by the two exact divisions of fe_mul_sparse's header comment
  precomputed-quotient product every limb, by tools/shoup_model.py (imported, not restated)
  additive / carry ops         the exact value, and the limbs where the header fixes them
  group law                    the affine sum by the short-Weierstrass formulas over Python integers
The bounds (< a b / R + p, < 2.01 p, < 4 p, < 2.5 p, KMAX) are the ones the headers state.  Plain module: no pytest hooks."""
import os, random, sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import shoup_model  # noqa: E402

W = 29
MASK = (1 << W) - 1
LAZY_MAX = 0x5fffffff          # the widest lazy limb a product accepts against a normalised partner (2^30.58)


class Field:
    def __init__(self, name, fid, p, L):
        self.name, self.fid, self.p, self.L = name, fid, p, L
        self.R = 1 << (W * L)
        self.pinv = pow(p, -1, self.R)
        self.PT = p >> (W * (L - 1))
        # fe_weak_reduce / fe_reduce accept a carried top limb below this (gen_constants.py: TOPMAX)
        self.topmax = min(self.PT ** 2 // 4, (1 << 31) - 1)

    def kp(self, K):
        """K p as borrow-friendly limbs (tools/gen_constants.py: every limb but the top >= 2^29 - 1)"""
        c = limbs(K * self.p, self.L)
        out = [c[i] + ((1 << W) if i < self.L - 1 else 0) - (1 if i > 0 else 0) for i in range(self.L)]
        assert value(out) == K * self.p
        return out


FR = Field("Fr", 0, 21888242871839275222246405745257275088548364400416034343698204186575808495617, 9)
M128 = Field("M128", 1, 270497897142230380135924736767050121217, 5)
FQ = Field("Fq", 2, 21888242871839275222246405745257275088696311157297823662689037894645226208583, 9)
FIELDS = (FR, FQ, M128)

# op codes: MZK_PROBE_* of include/mzk.h
(MUL, SQR, MUL_ADD2, SHOUP_MUL, SMUL, SMUL_C1, SADD, SSUB, SCARRY, SBIAS, SREDUCE, ADD, SUB4, SUB8, NEG_LAZY4, NEG_LAZY8, DBL, CARRY,
 WEAK_REDUCE, REDUCE, COND_SUB_P, NEG_CANON, IS_ZERO_MOD6, IS_ZERO_MOD10, IS_ZERO_MOD12, INV) = range(26)
OP_NAMES = ("mul sqr mul_add2 shoup_mul smul smul_c1 sadd ssub scarry sbias sreduce add sub4 sub8 neg_lazy4 neg_lazy8 dbl carry "
            "weak_reduce reduce cond_sub_p neg_canon is_zero_mod6 is_zero_mod10 is_zero_mod12 inv").split()
FORM_CPP, FORM_ASM, FORM_QUAD, FORM_ROW, FORM_WAVE = range(5)
FORM_NAMES = ("cpp", "asm", "quad", "row", "wave")
ARITY = {MUL_ADD2: 4, SHOUP_MUL: 3, MUL: 2, SMUL: 2, SMUL_C1: 2, SADD: 2, SSUB: 2, ADD: 2, SUB4: 2, SUB8: 2}
SIGNED_OPS = (SMUL, SMUL_C1, SADD, SSUB, SCARRY, SBIAS, SREDUCE)


def arity(op):
    return ARITY.get(op, 1)


def field_ops(f):
    ops = [o for o in range(26) if o not in SIGNED_OPS and o != SHOUP_MUL]
    if f is M128:
        ops += list(SIGNED_OPS)
    if f is FR:
        ops.append(SHOUP_MUL)
    return sorted(ops)


def field_forms(f, op):
    forms = [FORM_CPP]
    if op in (MUL, SQR, MUL_ADD2) or (op == SHOUP_MUL and f is FR) or (op == SMUL and f is M128):
        forms.append(FORM_ASM)
    if op == INV and f is FQ:
        forms.append(FORM_WAVE)
    return forms


# ---- limbs ------------------------------------------------------------------------------------------------------------------
def limbs(v, L):
    """normalised limbs of v >= 0: limbs 0 .. L-2 below 2^29, the top limb takes the rest"""
    assert v >= 0
    return [(v >> (W * i)) & MASK for i in range(L - 1)] + [v >> (W * (L - 1))]


def value(l):
    return sum(int(v) << (W * i) for i, v in enumerate(l))


def s32(v):
    v = int(v) & 0xffffffff
    return v - (1 << 32) if v >> 31 else v


def u32(v):
    return int(v) & 0xffffffff


def svalue(l):
    return sum(s32(v) << (W * i) for i, v in enumerate(l))


def slimbs(v, L):
    """the limbs fe_scarry leaves: limbs 0 .. L-2 in [0, 2^29), the top limb signed (floor division), as u32 words"""
    out = [(v >> (W * i)) & MASK for i in range(L - 1)]
    top = v >> (W * (L - 1))
    assert -(1 << 31) <= top < (1 << 31)
    return out + [u32(top)]


# ---- the models -------------------------------------------------------------------------------------------------------------
def mont_dense(f, T):
    """(T + m p) / R for the unique m = -T p^-1 mod R: what one Montgomery reduction of the double-width T returns, limb for limb"""
    m = (-T * f.pinv) % f.R
    q, r = divmod(T + m * f.p, f.R)
    assert r == 0
    return limbs(q, f.L)


def mont_sparse(f, a, b, signed, C):
    """fe_mul_sparse<P, SIGNED, C>: the two exact divisions of its header comment (floor semantics for negative T)"""
    beta = 1 << W
    T = (svalue(a) if signed else value(a)) * value(b)
    bl = beta ** (f.L - 1)
    m1 = bl - (T % bl)
    U, r = divmod(T + m1 * f.p, bl)
    assert r == 0
    m2 = (1 + C) * beta - (U % beta)
    V, r = divmod(U + m2 * f.p, beta)
    assert r == 0
    return slimbs(V, f.L) if signed else limbs(V, f.L)


def shoup_consts(wv):
    return shoup_model.limbs(wv), shoup_model.limbs(wv * shoup_model.BETA // shoup_model.P)


class Mismatch(AssertionError):
    pass


def _fail(f, op, form, case, out, why, limb=None):
    raise Mismatch("%s %s form=%s class=%s: %s%s\n  operands: %s\n  result:   %s" % (
        f.name, OP_NAMES[op], FORM_NAMES[form], case["cls"], why, "" if limb is None else " (first differing limb %d)" % limb,
        [[hex(x) for x in o] for o in case["ops"]], [hex(int(x)) for x in out]))


def _exact(f, op, form, case, out, want):
    for i, (g, w) in enumerate(zip(out, want)):
        if int(g) != int(w):
            _fail(f, op, form, case, out, "expected limbs %s" % [hex(int(x)) for x in want], i)


def check_field(f, op, form, case, out):
    """out: the L result limbs (u32).  Raises Mismatch naming field, op, form, class, operands and the first differing limb."""
    L, p = f.L, f.p
    o = case["ops"]
    out = [int(x) for x in out]

    def normalised(what=""):
        for i in range(L - 1):
            if out[i] > MASK:
                _fail(f, op, form, case, out, "limb not normalised" + what, i)

    if op in (MUL, SQR, MUL_ADD2):
        if op == MUL and f is M128:
            return _exact(f, op, form, case, out, mont_sparse(f, o[0], o[1], False, 0))
        T = value(o[0]) * value(o[1]) if op == MUL else value(o[0]) ** 2 if op == SQR else value(o[0]) * value(o[1]) + value(o[2]) * value(o[3])
        want = mont_dense(f, T)
        assert value(want) * f.R < T + p * f.R          # the header's bound: < a b / R + p
        return _exact(f, op, form, case, out, want)
    if op == SHOUP_MUL:
        want, worst, _ = shoup_model.shoup_mul(o[0], o[1], o[2])
        assert worst < 1 << 64
        normalised()
        if value(out) % p != value(o[0]) * value(o[1]) % p:
            _fail(f, op, form, case, out, "r != x w (mod p)")
        if value(out) >= 4 * p:
            _fail(f, op, form, case, out, "r >= 4 p")
        return _exact(f, op, form, case, out, want)
    if op in (SMUL, SMUL_C1):
        return _exact(f, op, form, case, out, mont_sparse(f, o[0], o[1], True, 1 if op == SMUL_C1 else 0))
    if op == SADD:
        return _exact(f, op, form, case, out, [u32(s32(a) + s32(b)) for a, b in zip(o[0], o[1])])
    if op == SSUB:
        return _exact(f, op, form, case, out, [u32(s32(a) - s32(b)) for a, b in zip(o[0], o[1])])
    if op == SCARRY:
        return _exact(f, op, form, case, out, slimbs(svalue(o[0]), L))
    if op == SBIAS:
        if svalue(out) != svalue(o[0]) + (1 << 12) * p:
            _fail(f, op, form, case, out, "value != a + 2^12 p")
        want = list(o[0])
        want[0] = u32(s32(want[0]) + (1 << 12) - (1 << W))
        want[1] = u32(s32(want[1]) + 1)
        want[L - 1] = u32(s32(want[L - 1]) + f.PT * (1 << 12))
        return _exact(f, op, form, case, out, want)
    if op == SREDUCE:
        return _exact(f, op, form, case, out, limbs(svalue(o[0]) % p, L))
    if op == ADD:
        return _exact(f, op, form, case, out, [a + b for a, b in zip(o[0], o[1])])
    if op in (SUB4, SUB8):
        K = 4 if op == SUB4 else 8
        if value(out) != value(o[0]) + K * p - value(o[1]):
            _fail(f, op, form, case, out, "value != a + %d p - b" % K)
        return _exact(f, op, form, case, out, [a + c - b for a, c, b in zip(o[0], f.kp(K), o[1])])
    if op in (NEG_LAZY4, NEG_LAZY8):
        K = 4 if op == NEG_LAZY4 else 8
        if value(out) != K * p - value(o[0]):
            _fail(f, op, form, case, out, "value != %d p - b" % K)
        if max(out) >= 0x60000000:
            _fail(f, op, form, case, out, "limb above 2^30.6")
        return _exact(f, op, form, case, out, [c - b for c, b in zip(f.kp(K), o[0])])
    if op == DBL:
        return _exact(f, op, form, case, out, [a << 1 for a in o[0]])
    if op == CARRY:
        return _exact(f, op, form, case, out, limbs(value(o[0]), L))
    if op == WEAK_REDUCE:
        normalised()
        v, r = value(o[0]), value(out)
        if r % p != v % p or r > v:
            _fail(f, op, form, case, out, "residue changed")
        if r * 100 >= 201 * p:
            _fail(f, op, form, case, out, "value >= 2.01 p (%.4f p)" % (r / p))
        return None
    if op == REDUCE:
        return _exact(f, op, form, case, out, limbs(value(o[0]) % p, L))
    if op == COND_SUB_P:
        v = value(o[0])
        return _exact(f, op, form, case, out, limbs(v - p if v >= p else v, L))
    if op == NEG_CANON:
        return _exact(f, op, form, case, out, limbs((-value(o[0])) % p, L))
    if op in (IS_ZERO_MOD6, IS_ZERO_MOD10, IS_ZERO_MOD12):
        kmax = {IS_ZERO_MOD6: 6, IS_ZERO_MOD10: 10, IS_ZERO_MOD12: 12}[op]
        v = value(o[0])
        want = 1 if (v % p == 0 and v // p <= kmax) else 0
        return _exact(f, op, form, case, out, [want] + [0] * (L - 1))
    if op == INV:
        x = value(o[0]) % p
        if x == 0:
            return _exact(f, op, form, case, out, [0] * L)
        normalised()
        if value(out) >= 2 * p:
            _fail(f, op, form, case, out, "inverse not below 2 p")
        want = pow(x, -1, p) * f.R * f.R % p         # raw x = a R  ->  a^-1 R = x^-1 R^2
        return _exact(f, op, form, case, limbs(value(out) % p, L), limbs(want, L))
    raise ValueError(op)


# ---- operand classes ---------------------------------------------------------------------------------------------------------
def _edge_values(f):
    """(class, normalised limbs): zero, one, p - 1, p, p + 1, 2 p - 1, every limb 2^29 - 1, a single non-zero limb per position"""
    p, L = f.p, f.L
    out = [("zero", limbs(0, L)), ("one", limbs(1, L)), ("p-1", limbs(p - 1, L)), ("p", limbs(p, L)), ("p+1", limbs(p + 1, L)),
           ("2p-1", limbs(2 * p - 1, L)), ("all-ones", [MASK] * L)]
    for i in range(L):
        out.append(("single-limb-%d" % i, [MASK - 0x1234 * (i + 1) if j == i else 0 for j in range(L)]))
    return out


def _rand_norm(f, rng):
    return [rng.randrange(MASK + 1) for _ in range(f.L)]


def _rand_below(f, rng, bound):
    return limbs(rng.randrange(bound), f.L)


def _lazy_forms(f, rng):
    """the lazy forms the callers produce, by their own steps, from random carried values"""
    p, L = f.p, f.L
    out = []
    b2, b4 = _rand_below(f, rng, 2 * p), _rand_below(f, rng, 4 * p)
    a = _rand_norm(f, rng)
    a[L - 1] = rng.randrange(2 * f.PT)
    out.append(("4p-b", [c - x for c, x in zip(f.kp(4), b2)]))
    out.append(("8p-b", [c - x for c, x in zip(f.kp(8), b4)]))
    out.append(("a+8p-b", [y + c - x for y, c, x in zip(a, f.kp(8), b4)]))
    out.append(("doubled", [x << 1 for x in _rand_below(f, rng, 5 * p // 2)]))
    out.append(("lazy-random", [rng.randrange(LAZY_MAX + 1) for _ in range(L)]))
    return out


def _sparse_ok(f, a, b, signed, C):
    """the contract of fe_mul_sparse for this pair: columns inside 64 bits and the top limb of the result inside 32"""
    ma = max(abs(s32(x)) if signed else x for x in a)
    if any(x > MASK for x in b[:-1]):
        return False
    if ma * MASK * f.L + f.PT * (2 << 30) + (1 << 36) >= 1 << (63 if signed else 64):
        return False
    try:
        V = mont_sparse(f, a, b, signed, C)
    except AssertionError:
        return False
    return signed or V[-1] < 1 << 32


def _m128_b_values(f, rng):
    """the right-hand operands of the sparse products: twiddles and other carried constants, below 2 p"""
    p = f.p
    return [("b=" + n, limbs(v, f.L)) for n, v in (("zero", 0), ("one", 1), ("R", f.R % p), ("p-1", p - 1), ("p", p), ("2p-1", 2 * p - 1))] + \
           [("b=random", _rand_below(f, rng, p)) for _ in range(3)]


def field_table(f, op, seed=1, nrand=1500):
    """the cases of (field, op): list of {"cls": str, "ops": [limbs, ...]}; deterministic; every case inside the op's contract"""
    rng = random.Random((seed << 16) ^ (f.fid << 8) ^ op)
    p, L = f.p, f.L
    cases = []

    def add(cls, *ops):
        assert len(ops) == arity(op)
        cases.append({"cls": cls, "ops": [[int(x) for x in o] for o in ops]})

    edges = _edge_values(f)
    if op in (MUL, SQR, MUL_ADD2):
        sparse = f is M128 and op == MUL
        rhs = _m128_b_values(f, rng) if f is M128 else edges + [("random", _rand_norm(f, rng)) for _ in range(3)]
        lhs = edges + _lazy_forms(f, rng) + [("top-limb-max", [MASK] * (L - 1) + [LAZY_MAX]), ("all-lazy-max", [LAZY_MAX] * L),
                                              ("below-2^30", [(1 << 30) - 1] * L)]
        carried = edges + [("doubled", [x << 1 for x in _rand_below(f, rng, 5 * p // 2)]), ("below-2^30", [(1 << 30) - 1] * L)]
        if op == MUL:
            for ca, a in lhs:
                for cb, b in rhs:
                    assert not sparse or _sparse_ok(f, a, b, False, 0), (ca, cb)
                    add(ca + " x " + cb, a, b)
            if not sparse:
                add("both-below-2^30", [(1 << 30) - 1] * L, [(1 << 30) - 1] * L)
        elif op == SQR:
            for ca, a in carried:          # squares only ever see carried operands (limbs < 2^30)
                add(ca, a)
            add("Rd<12p", limbs(12 * p - 1, L))
        else:
            for k, (ca, a) in enumerate(lhs):
                cb, b = rhs[k % len(rhs)]
                cc, c = lhs[(3 * k + 1) % len(lhs)]
                cd, d = rhs[(5 * k + 2) % len(rhs)]
                add("%s x %s + %s x %s" % (ca, cb, cc, cd), a, b, c, d)
            if f is not M128:
                # the widest pair mzk_ec.h feeds it (xyzz_madd_signed_with): Rd < 12 p carried against Vd < 9.03 p, 8 p - Y1 lazy against PPP
                for _ in range(40):
                    rd, vd = _rand_below(f, rng, 12 * p), _rand_below(f, rng, 903 * p // 100)
                    y1, ppp = _rand_below(f, rng, 5 * p // 2), _rand_below(f, rng, 108 * p // 100)
                    add("Rd Vd + (8p-Y1) PPP", rd, vd, [c - x for c, x in zip(f.kp(8), y1)], ppp)
                add("Rd Vd + (8p-Y1) PPP at the bounds", limbs(12 * p - 1, L), limbs(903 * p // 100, L), f.kp(8), limbs(108 * p // 100, L))
        for k in range(nrand):
            a = _rand_norm(f, rng) if k % 3 else [rng.randrange(LAZY_MAX + 1) for _ in range(L)]
            b = _rand_below(f, rng, 2 * p) if f is M128 else _rand_norm(f, rng)
            if op == SQR:
                add("random", _rand_norm(f, rng) if k % 3 else [rng.randrange(1 << 30) for _ in range(L)])
            elif op == MUL:
                add("random" if k % 3 else "lazy-random x random", a, b)
            else:
                c = [rng.randrange(LAZY_MAX + 1) for _ in range(L)] if k % 2 else _rand_norm(f, rng)
                d = _rand_below(f, rng, 2 * p) if f is M128 else _rand_norm(f, rng)
                add("random", a, b, c, d)
    elif op == SHOUP_MUL:
        # one constant pair per wave of 64 cases (the kernel reads w, wq of the wave's first lane into scalar registers)
        consts = [0, 1, 2, p - 1, p // 2, (1 << 253) % p] + [rng.randrange(p) for _ in range(18)]
        for wv in consts:
            w, wq = shoup_consts(wv)
            xs = [("x=" + c, x) for c, x in edges] + [("x=lazy-3*2^30", [3 << 30] * (L - 1) + [(1 << 27) - 1]), ("x=just-below-2^261", [MASK] * L)]
            while len(xs) < 64:
                k = len(xs)
                lim = (MASK, 3 << 30, (1 << 30) + (1 << 29))[k % 3]
                xs.append(("x=random" if k % 3 == 0 else "x=lazy-random", [rng.randrange(lim + 1) for _ in range(L - 1)] + [rng.randrange(1 << 27)]))
            assert len(xs) == 64
            for c, x in xs:
                assert value(x) < 1 << 261
                add("w=%s %s" % (hex(wv) if wv > 2 else wv, c), x, w, wq)
    elif op in (SMUL, SMUL_C1):
        C = 1 if op == SMUL_C1 else 0
        M31 = (1 << 31) - 1
        lhs = [("a=" + c, a) for c, a in edges]
        lhs += [("a=+max-i32", [u32(M31)] * (L - 1) + [1 << 12]), ("a=-max-i32", [u32(-M31)] * (L - 1) + [u32(-(1 << 12))]),
                ("a=mixed-max-i32", [u32(M31 if i & 1 else -M31) for i in range(L - 1)] + [u32(-(1 << 12))]),
                ("a=3(2^29-1)", [3 * MASK] * (L - 1) + [1 << 12]), ("a=-3(2^29-1)", [u32(-3 * MASK)] * (L - 1) + [u32(-(1 << 12))]),
                ("a=-1", [u32(-1)] + [0] * (L - 1)), ("a=-p", [u32(-x) for x in limbs(p, L)]),
                ("a=just-below-2^12p", slimbs((1 << 12) * p - 1, L)), ("a=just-above--2^12p", slimbs(-(1 << 12) * p + 1, L))]
        for ca, a in lhs:
            for cb, b in _m128_b_values(f, rng):
                assert _sparse_ok(f, a, b, True, C), (ca, cb)
                add(ca + " x " + cb, a, b)
        add("a=all-ones x b=all-ones", [MASK] * L, [MASK] * L)
        for k in range(nrand):
            kind = k % 4
            lim = (M31, 3 * MASK, MASK, M31)[kind]
            a = [u32(rng.randrange(-lim, lim + 1)) for _ in range(L - 1)] + [u32(rng.randrange(-(1 << 23), 1 << 23))]
            if kind == 2:
                a = [u32(-x) for x in _rand_below(f, rng, 4 * p)]
            b = _rand_below(f, rng, p)
            assert _sparse_ok(f, a, b, True, C)
            add(("full-range", "stage-pair-range", "negated", "full-range")[kind] + " x random", a, b)
    elif op in (SADD, SSUB):
        M31, sg = (1 << 31) - 1, (1 if op == SADD else -1)
        add("max + 0", [u32(M31)] * L, [0] * L)
        add("min + 0", [u32(-M31 - 1)] * L, [0] * L)
        add("max -+ max", [u32(M31)] * L, [u32(-sg * M31)] * L)
        add("to the top of i32", [u32(1 << 30)] * L, [u32(sg * ((1 << 30) - 1))] * L)
        add("to the bottom of i32", [u32(-(1 << 30))] * L, [u32(-sg * (1 << 30))] * L)
        add("stage pair", [3 * MASK // 2 + 1] * L, [u32(sg * (3 * MASK // 2))] * L)
        for c, a in edges:
            add(c + " -+ all-ones", a, [MASK] * (L - 1) + [0])
        for k in range(nrand):
            a = [rng.randrange(-(1 << 30), 1 << 30) for _ in range(L)]
            b = [rng.randrange(-(1 << 30), 1 << 30) for _ in range(L)]
            add("random mixed signs", [u32(x) for x in a], [u32(x) for x in b])
    elif op in (SCARRY, SBIAS, SREDUCE):
        M31 = (1 << 31) - 1
        sp = []
        if op == SCARRY:
            sp += [("+max-i32", [u32(M31)] + [u32(M31 - 8)] * (L - 1)), ("-max-i32", [u32(-M31 - 1)] + [u32(-M31 + 8)] * (L - 1)),
                   ("mixed", [u32((M31 - 8) if i & 1 else -(M31 - 8)) for i in range(L)]), ("-1", [u32(-1)] + [0] * (L - 1)),
                   ("borrow-chain", [u32(-1)] + [0] * (L - 2) + [1]), ("carry-chain", [1 << W] + [MASK] * (L - 2) + [0])]
        if op == SBIAS:
            sp += [("limb0-min", [u32(-(1 << 31) - (1 << 12) + (1 << W))] + [0] * (L - 1)), ("limb1-max", [0, u32(M31 - 1)] + [0] * (L - 2)),
                   ("3(2^29-1)", [3 * MASK] * (L - 1) + [0]), ("-3(2^29-1)", [u32(-3 * MASK)] * (L - 1) + [0])]
        sp += [(c, a) for c, a in edges if op != SREDUCE or value(a) < (1 << 12) * p]
        sp += [("3(2^29-1)", [3 * MASK] * (L - 1) + [0]), ("-3(2^29-1)", [u32(-3 * MASK)] * (L - 1) + [0]),
               ("just-below-2^12p", slimbs((1 << 12) * p - 1, L)), ("just-above--2^12p", slimbs(-(1 << 12) * p + 1, L)),
               ("-1", [u32(-1)] + [0] * (L - 1)), ("-p", [u32(-x) for x in limbs(p, L)])]
        # the borrow path of fe_sreduce (limb 0 < folded quotient): multiples of 3256 * 2^116 = p - 1 and of p, +- small
        for k in (1, 2, 3, 7, 100, 4095, -1, -2, -100, -4095):
            for base, nm in ((p - 1, "(p-1)"), (p, "p")):
                for e in (0, 1, 2, abs(k) - 1, abs(k), abs(k) + 1, -1, -abs(k), 4095, 4096 + abs(k), 4097 + abs(k)):
                    v = k * base + e
                    if abs(v) < (1 << 12) * p:
                        sp.append(("%d%s%+d" % (k, nm, e), slimbs(v, L)))
        # the same values as the uncarried limbs a stage pair leaves: value v, limbs spread by +- 2^29 pairs
        for c, a in list(sp[-40:]):
            b = [s32(x) for x in a]
            for i in range(L - 1):
                d = (1 if i & 1 else -1) * 2
                b[i] += d << W
                b[i + 1] -= d
            sp.append((c + " spread", [u32(x) for x in b]))
        for c, a in sp:
            add(c, a)
        for k in range(nrand):
            lim = 3 * MASK if k % 2 else (1 << 30)
            a = [rng.randrange(-lim, lim + 1) for _ in range(L - 1)] + [rng.randrange(-(1 << 23), 1 << 23)]
            add("random stage-pair range" if k % 2 else "random 2^30 range", [u32(x) for x in a])
        if op == SREDUCE:
            for c in cases:
                assert abs(svalue(c["ops"][0])) < (1 << 12) * p, c["cls"]
    elif op == ADD:
        for ca, a in edges + _lazy_forms(f, rng):
            for cb, b in edges[:7] + [("lazy-random", [rng.randrange(LAZY_MAX + 1) for _ in range(L)])]:
                add(ca + " + " + cb, a, b)
        add("to the top of u32", [0xffffffff] * L, [0] * L)
        add("to the top of u32, halves", [0x80000000] * L, [0x7fffffff] * L)
        for k in range(nrand):
            add("random", [rng.randrange(1 << 31) for _ in range(L)], [rng.randrange(1 << 31) for _ in range(L)])
    elif op in (SUB4, SUB8, NEG_LAZY4, NEG_LAZY8):
        K = 4 if op in (SUB4, NEG_LAZY4) else 8
        kp = f.kp(K)
        subs = [(c, b) for c, b in edges if value(b) < K * p // 2 and all(x <= MASK for x in b[:-1])]
        subs += [("just-below-%dp" % (K // 2), limbs(K * p // 2 - 1, L)), ("2.5p", limbs(5 * p // 2, L) if K == 8 else limbs(2 * p - 2, L))]
        subs += [("random", _rand_below(f, rng, K * p // 2)) for _ in range(nrand if op in (NEG_LAZY4, NEG_LAZY8) else 6)]
        if op in (NEG_LAZY4, NEG_LAZY8):
            for c, b in subs:
                add(c, b)
        else:
            mins = [("zero", [0] * L), ("all-ones", [MASK] * L), ("lazy-max", [LAZY_MAX] * L), ("largest", [0xffffffff - c for c in kp])]
            mins += [(c, a) for c, a in edges[1:6]] + _lazy_forms(f, rng)[:3]
            for ca, a in mins:
                for cb, b in subs:
                    if ca == "largest":
                        a = [0xffffffff - c + x for c, x in zip(kp, b)]
                    add(ca + " - " + cb, a, b)
            for k in range(nrand):
                add("random", [rng.randrange(LAZY_MAX + 1) for _ in range(L)], _rand_below(f, rng, K * p // 2))
    elif op == DBL:
        for c, a in edges + _lazy_forms(f, rng) + [("below-2^31", [0x7fffffff] * L)]:
            add(c, a)
        for k in range(nrand):
            add("random", [rng.randrange(1 << 31) for _ in range(L)])
    elif op == CARRY:
        for c, a in edges + _lazy_forms(f, rng):
            add(c, a)
        add("top of u32", [0xffffffff] + [0xffffffff - 8] * (L - 2) + [0xffffff00])
        add("carry chain", [1 << W] + [MASK] * (L - 2) + [0])
        add("a+8p-b+8p-b", [2 * c + MASK for c in f.kp(8)])
        for k in range(nrand):
            add("random", [rng.randrange(0xfffffff0) for _ in range(L - 1)] + [rng.randrange(1 << 31)])
    elif op in (WEAK_REDUCE, REDUCE, INV):
        top = f.topmax - 1
        sp = [(c, a) for c, a in edges if value(a) >> (W * (L - 1)) < f.topmax]
        sp += [(c, a) for c, a in _lazy_forms(f, rng) if value(a) >> (W * (L - 1)) < f.topmax]
        sp += [("top-limb-max", [MASK] * (L - 1) + [top]), ("top-limb-max, low zero", [0] * (L - 1) + [top]),
               ("top-limb-max uncarried", [0xffffffff] + [0xffffffff - 8] * (L - 2) + [top - 8])]
        for k in (1, 2, 3, 4, 8, 12, 13, 16, 100):
            for e in (-1, 0, 1):
                sp.append(("%dp%+d" % (k, e), limbs(k * p + e, L)))
        sp += [("(a+b)*2+16p-b", [2 * x + y + c for x, y, c in zip(_rand_norm(f, rng), [0] * L, f.kp(16))]) for _ in range(3)]
        if f is M128:
            sp = [(c, a) for c, a in sp if value(a) >> (W * (L - 1)) < f.topmax]
        for c, a in sp:
            add(c, a)
        for k in range(nrand if op != INV else nrand // 3):
            if k % 2:
                add("random canonical", _rand_below(f, rng, p))
            else:
                add("random lazy", [rng.randrange(LAZY_MAX + 1) for _ in range(L - 1)] + [rng.randrange(min(f.topmax - 8, LAZY_MAX))])
    elif op == COND_SUB_P:
        for c, a in edges + [("top-limb-max", [MASK] * (L - 1) + [0x7fffffff]), ("2p", limbs(2 * p, L)), ("p, limb 0 short", limbs(p - 2, L))]:
            add(c, a)
        for i in range(L - 1):          # p with one limb lowered / raised: the borrow has to travel
            lo = limbs(p, L)
            if lo[i] > 0:
                lo[i] -= 1
                add("p minus one in limb %d" % i, lo)
            hi = limbs(p, L)
            if hi[i] < MASK:
                hi[i] += 1
                add("p plus one in limb %d" % i, hi)
        for k in range(nrand):
            add("random", _rand_below(f, rng, 3 * p))
    elif op == NEG_CANON:
        for c, a in edges:
            if value(a) < p:
                add(c, a)
        add("p-2", limbs(p - 2, L))
        add("2", limbs(2, L))
        add("(p-1)/2", limbs((p - 1) // 2, L))
        add("2^k", limbs(1 << (W * (L - 1)), L))
        for k in range(nrand):
            add("random", _rand_below(f, rng, p))
    elif op in (IS_ZERO_MOD6, IS_ZERO_MOD10, IS_ZERO_MOD12):
        kmax = {IS_ZERO_MOD6: 6, IS_ZERO_MOD10: 10, IS_ZERO_MOD12: 12}[op]
        for k in range(kmax + 3):
            add("%dp" % k, limbs(k * p, L))
            add("%dp+1" % k, limbs(k * p + 1, L))
            if k:
                add("%dp-1" % k, limbs(k * p - 1, L))
            add("%dp+2^29" % k, limbs(k * p + (1 << W), L))
            add("%dp+2^%d" % (k, W * (L - 1)), limbs(k * p + (1 << (W * (L - 1))), L))
        for k in range(nrand):
            add("random", _rand_below(f, rng, (kmax + 2) * p))
    else:
        raise ValueError(op)
    return cases


def pack_cases(cases, L):
    """the flat u32 operand array of a case list (numpy), n x arity x L"""
    import numpy as np
    return np.array([[x for o in c["ops"] for x in o] for c in cases], dtype=np.uint32).reshape(len(cases), -1)


# ---- BN254 G1 -----------------------------------------------------------------------------------------------------------------
(G1_MADD_SIGNED, G1_MADD, G1_ADD, G1_DBL, G1_DBL_AFFINE, G1_TO_AFFINE) = range(6)
G1_NAMES = ("madd_signed", "madd", "add", "dbl", "dbl_affine", "to_affine")
G1_GEN = (1, 2)
Q = FQ.p


def g1_forms(op):
    if op in (G1_ADD, G1_DBL):
        return [FORM_CPP, FORM_ASM, FORM_QUAD, FORM_ROW]
    if op == G1_DBL_AFFINE:
        return [FORM_CPP]
    if op == G1_TO_AFFINE:
        return [FORM_CPP, FORM_WAVE]
    return [FORM_CPP, FORM_ASM]


def aff_neg(P):
    return None if P is None else (P[0], (-P[1]) % Q)


def aff_add(P1, P2):
    """short Weierstrass, y^2 = x^3 + 3, None = infinity"""
    if P1 is None:
        return P2
    if P2 is None:
        return P1
    (x1, y1), (x2, y2) = P1, P2
    if x1 == x2:
        if (y1 + y2) % Q == 0:
            return None
        lam = 3 * x1 * x1 * pow(2 * y1, -1, Q) % Q
    else:
        lam = (y2 - y1) * pow(x2 - x1, -1, Q) % Q
    x3 = (lam * lam - x1 - x2) % Q
    return (x3, (lam * (x1 - x3) - y1) % Q)


def aff_mul(P, k):
    acc = None
    while k:
        if k & 1:
            acc = aff_add(acc, P)
        P = aff_add(P, P)
        k >>= 1
    return acc


def on_curve(P):
    return P is None or (P[1] * P[1] - P[0] ** 3 - 3) % Q == 0


def mont(v):
    return v * FQ.R % Q


def affine_limbs(P):
    """an affine operand: 2 x 9 limbs, Montgomery form, canonical"""
    return limbs(mont(P[0]), 9) + limbs(mont(P[1]), 9)


def slot_of(P, z, j=(0, 0, 0, 0)):
    """the raw slot of the point P in the representation (x z^2, y z^3, z^2, z^3), Montgomery form, coordinate c stored as its canonical
    value + j[c] p; None -> the all-zero slot"""
    if P is None:
        return [0] * 36
    vals = (mont(P[0] * z * z % Q), mont(P[1] * z * z * z % Q), mont(z * z % Q), mont(z * z * z % Q))
    out = []
    for v, jj in zip(vals, j):
        v += jj * Q
        assert 2 * v < 5 * Q
        out += limbs(v, 9)
    return out


def slot_coords(s):
    return [value(s[9 * c:9 * c + 9]) for c in range(4)]


def j_choices(P, z):
    """per coordinate, every j for which canonical + j p stays below 2.5 p"""
    vals = (mont(P[0] * z * z % Q), mont(P[1] * z * z * z % Q), mont(z * z % Q), mont(z * z * z % Q))
    return [[j for j in range(3) if 2 * (v + j * Q) < 5 * Q] for v in vals]


def slot_point(s):
    """the group element a slot holds (None = infinity; raises if it is not a consistent XYZZ representation)"""
    X, Y, ZZ, ZZZ = slot_coords(s)
    if ZZ % Q == 0:
        return None
    x, y = X * pow(ZZ, -1, Q) % Q, Y * pow(ZZZ, -1, Q) % Q
    # ZZ^3 == ZZZ^2 out of Montgomery form
    iR = pow(FQ.R, -1, Q)
    if pow(ZZ * iR, 3, Q) != pow(ZZZ * iR, 2, Q):
        raise Mismatch("ZZ^3 != ZZZ^2")
    return (x, y)


def mmul(a, b):
    """the value F::mul returns (FeCpp and FeAsm alike): exact"""
    return value(mont_dense(FQ, a * b))


def diff_multiples(op, a_slot, b, neg=False):
    """(k_P, k_R): the multiples of p that Pd and Rd are when the operands share x (and y up to sign), as the code computes them;
    None where the difference is not a multiple of p.  b: affine limbs (madd forms) or a slot (add)."""
    X1, Y1, ZZ1, ZZZ1 = slot_coords(a_slot)
    if op == G1_ADD:
        X2, Y2, ZZ2, ZZZ2 = slot_coords(b)
        pd = mmul(X2, ZZ1) + 4 * Q - mmul(X1, ZZ2)
        rd = mmul(Y2, ZZZ1) + 4 * Q - mmul(Y1, ZZZ2)
    else:
        qx, qy = value(b[:9]), value(b[9:])
        s2 = mmul(qy, ZZZ1)
        if neg:
            s2 = 4 * Q - s2
        pd = mmul(qx, ZZ1) + 8 * Q - X1
        rd = s2 + 8 * Q - Y1
    return (pd // Q if pd % Q == 0 else None, rd // Q if rd % Q == 0 else None)


# the zero tests the group law passes: (KMAX of Pd, KMAX of Rd) per op
G1_KMAX = {G1_MADD_SIGNED: (10, 12), G1_MADD: (10, 10), G1_ADD: (6, 6)}
# the multiples the differences can take under the storage bound (value < 2.5 p, products canonical or canonical + p), by
# reasoning: a product is canonical + u p, u in {0, 1}, u = 1 only for a canonical part below ~2.5 p^2 / R; a stored coordinate is
# canonical + j p, j in {0, 1, 2}, j = 2 only for a canonical part below p / 2.
#   madd:  Pd = U2 + 8 p - X1 with U2 == X1: 8 + u - j, the canonical parts equal, so every (u, j): 6 .. 9.   Rd likewise.
#   madd_signed, neg: Rd = 12 p - S2 - Y1 with S2 == -Y1: the canonical parts are c and p - c, so 11 - u - j with (u = 1 or
#          j = 2) excluding each other: 9 .. 11.
#   add:   Pd = U2 + 4 p - U1, both products: 4 + u2 - u1: 3 .. 5.  Rd likewise.
G1_K_EXPECTED = {(G1_MADD_SIGNED, "P"): {6, 7, 8, 9}, (G1_MADD_SIGNED, "R+"): {6, 7, 8, 9}, (G1_MADD_SIGNED, "R-"): {9, 10, 11},
                 (G1_MADD, "P"): {6, 7, 8, 9}, (G1_MADD, "R+"): {6, 7, 8, 9}, (G1_ADD, "P"): {3, 4, 5}, (G1_ADD, "R+"): {3, 4, 5}}


def g1_expected(op, case):
    A = case["A"]
    if op in (G1_MADD_SIGNED, G1_MADD):
        return aff_add(A, aff_neg(case["B"]) if case.get("neg") else case["B"])
    if op == G1_ADD:
        return aff_add(A, case["B"])
    if op in (G1_DBL, G1_DBL_AFFINE):
        return aff_add(A, A)
    return A


def _g1_points(rng, n):
    return [aff_mul(G1_GEN, rng.randrange(1, FR.p)) for _ in range(n)]


def _rand_z(rng):
    return rng.randrange(1, Q)


def g1_table(op, seed=1, nrand=600, search=6000):
    """cases of a group op: {"cls", "a": slot or affine limbs, "b": affine limbs / slot / None, "neg": 0 / 1, "A", "B": the affine
    points (None = infinity)}, and the coverage of the exceptional branches: {"P" / "R+" / "R-": set of multiples seen}"""
    rng = random.Random((seed << 8) ^ (0x61 + op))
    pts = _g1_points(rng, 24) + [G1_GEN]
    cases, cover = [], {}

    def add(cls, a, b, neg, A, B):
        cases.append({"cls": cls, "a": a, "b": b, "neg": int(neg), "A": A, "B": B})

    if op == G1_DBL_AFFINE:
        for i, P in enumerate(pts + _g1_points(rng, nrand // 8)):
            add("generator" if P == G1_GEN else "point", affine_limbs(P), None, 0, P, None)
        return cases, cover
    if op in (G1_DBL, G1_TO_AFFINE):
        add("infinity", slot_of(None, 1), None, 0, None, None)
        for i, P in enumerate(pts):
            for z in (1, _rand_z(rng)):
                js = j_choices(P, z)
                for jx in js[0]:
                    for jy in js[1]:
                        add("%sz%s j=%d%d" % ("generator " if P == G1_GEN else "", "=1" if z == 1 else "", jx, jy), slot_of(P, z, (jx, jy, js[2][-1], js[3][-1])), None, 0, P, None)
        for P in _g1_points(rng, nrand // 8):
            for _ in range(8 if op == G1_DBL else 1):
                z = _rand_z(rng)
                js = j_choices(P, z)
                add("random", slot_of(P, z, tuple(rng.choice(c) for c in js)), None, 0, P, None)
        return cases, cover

    affine_b = op != G1_ADD
    signs = (0, 1) if op == G1_MADD_SIGNED else (0,)

    def bform(B, zb=None, jb=(0, 0, 0, 0)):
        if affine_b:
            return affine_limbs(B)
        return slot_of(B, zb if zb is not None else _rand_z(rng), jb)

    # generic classes: another point / the same point / its negative / infinity on either side / the generator / z = 1, every j
    for i, A in enumerate(pts):
        others = [("another point", pts[(i + 5) % len(pts)]), ("the same point", A), ("its negative", aff_neg(A)), ("the generator", G1_GEN)]
        for z in (1, _rand_z(rng)):
            js = j_choices(A, z)
            for jx in js[0]:
                for jy in js[1]:
                    a = slot_of(A, z, (jx, jy, js[2][-1 if (jx + jy) & 1 else 0], js[3][-1 if jx & 1 else 0]))
                    for cb, B in others:
                        for neg in signs:
                            add("%s%s z%s j=%d%d" % (cb, " negated" if neg else "", "=1" if z == 1 else "", jx, jy), a, bform(B), neg, A, B)
        if not affine_b:
            z = _rand_z(rng)
            add("a + infinity", slot_of(A, z), slot_of(None, 1), 0, A, None)
            add("infinity + b", slot_of(None, 1), slot_of(A, z), 0, None, A)
            add("b with z = 1", slot_of(pts[(i + 3) % len(pts)], _rand_z(rng)), slot_of(A, 1), 0, pts[(i + 3) % len(pts)], A)
        else:
            for neg in signs:
                add("infinity + q" + (" negated" if neg else ""), slot_of(None, 1), affine_limbs(A), neg, None, A)
    if not affine_b:
        add("infinity + infinity", slot_of(None, 1), slot_of(None, 1), 0, None, None)
    # the exceptional branches with every multiple the zero tests can meet: search z in the integer model until all occur
    want = {k: set(v) for (o, k), v in G1_K_EXPECTED.items() if o == op}
    cover = {k: set() for k in want}
    tries = 0
    while any(cover[k] != want[k] for k in want) and tries < search:
        tries += 1
        A = pts[tries % len(pts)]
        z = _rand_z(rng)
        # steer the search: the rare multiples need a small canonical part (u = 1), which a random z gives with probability ~ 2^-6
        js = j_choices(A, z)
        zb = _rand_z(rng)
        for same in (True, False):
            for neg in signs:
                # madd_signed adds (neg ? -q : q): q = +-A so that the sum is 2 A (Rd == 0) or infinity
                B = A if same != bool(neg) else aff_neg(A)
                for jx in js[0]:
                    for jy in js[1]:
                        a = slot_of(A, z, (jx, jy, 0, 0))
                        b = bform(B, zb)
                        kP, kR = diff_multiples(op, a, b, bool(neg))
                        assert kP is not None and (kR is not None) == same
                        key = "R-" if neg else "R+"
                        new = kP not in cover["P"] or (same and kR not in cover[key])
                        if new:
                            cover["P"].add(kP)
                            if same:
                                cover[key].add(kR)
                            add("exceptional %s%s kP=%d kR=%s" % ("doubling" if same else "cancelling", " negated" if neg else "", kP, kR), a, b, neg, A, B)
    for k in range(nrand):
        A, B = rng.choice(pts), rng.choice(pts)
        if k % 16 == 0:
            B = A if k % 32 else aff_neg(A)
        z = _rand_z(rng)
        js = j_choices(A, z)
        neg = rng.choice(signs)
        jb = (0, 0, 0, 0)
        zb = _rand_z(rng)
        if not affine_b:
            jb = tuple(rng.choice(c) for c in j_choices(B, zb))
        add("random", slot_of(A, z, tuple(rng.choice(c) for c in js)), bform(B, zb, jb), neg, A, B)
    return cases, cover


def check_g1_slot(op, form, case, out, what=""):
    """a result slot against the affine sum: group element, infinity <=> all-zero, normalised limbs, every coordinate < 2.5 p"""
    out = [int(x) for x in out]
    want = g1_expected(op, case)

    def fail(why):
        raise Mismatch("G1 %s form=%s class=%s%s: %s\n  a: %s\n  b: %s\n  neg: %d\n  result: %s" % (
            G1_NAMES[op], FORM_NAMES[form], case["cls"], what, why, [hex(x) for x in case["a"]],
            None if case["b"] is None else [hex(x) for x in case["b"]], case["neg"], [hex(x) for x in out]))
    if op == G1_TO_AFFINE:
        x = sum(out[i] << (32 * i) for i in range(8))
        y = sum(out[8 + i] << (32 * i) for i in range(8))
        if any(out[16:]):
            fail("words behind the point are not zero")
        if want is None:
            if x or y:
                fail("expected infinity (all-zero)")
        elif (x, y) != want:
            fail("expected the affine point (%x, %x), got (%x, %x)" % (want[0], want[1], x, y))
        return
    zero = not any(out)
    if want is None:
        if not zero:
            fail("expected infinity as the all-zero slot")
        return
    if zero:
        fail("all-zero slot (infinity) for a finite sum")
    for c in range(4):
        co = out[9 * c:9 * c + 9]
        for i in range(8):
            if co[i] > MASK:
                fail("coordinate %d limb %d not below 2^29" % (c, i))
        if 2 * value(co) >= 5 * Q:
            fail("coordinate %d not below 2.5 p (%.3f p)" % (c, value(co) / Q))
    try:
        got = slot_point(out)
    except Mismatch as e:
        fail(str(e))
    if got is None:
        fail("ZZ == 0 (mod p) in a non-zero slot")
    if got != want:
        fail("wrong group element: expected (%x, %x), got (%x, %x)" % (want[0], want[1], got[0], got[1]))


def first_diff(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if int(x) != int(y):
            return i
    return None
