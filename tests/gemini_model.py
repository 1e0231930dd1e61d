"""Pure-Python restatement of the reference's multilinear half: algebra/gemini.rs and algebra/sumcheck.rs (paths relative to
myzkp/src/modules/).  Field elements are Python ints mod P (BN254 Fr = ModEIP197).  The GPU tests and the golden-vector generator
check the library against this model; tests/test_gemini_model.py checks the model against the reference's own tests."""
import hashlib

P = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def neg(x):
    """(FqOrder::zero() - x).sanitize()"""
    return (-x) % P


# ---- gemini.rs ------------------------------------------------------------------------------------------------------
def tensor_product(a, b):
    """gemini.rs:39-49: a * b^T read column by column: out[i * len(a) + k] = a[k] * b[i]."""
    return [a[k] * b[i] % P for i in range(len(b)) for k in range(len(a))]


class SplitFoldError(ValueError):
    pass


def split_and_fold(coef, rhos):
    """gemini.rs:51-100.  f_e keeps the even coefficients, f_o the odd ones shifted down; f_i = f_e + rho * f_o keeps the even
    positions: f_{i+1}[k] = f_i[2k] + rho_i f_i[2k+1].  Returns the el + 1 levels (lists of ints)."""
    n = len(coef)
    if n == 0 or n & (n - 1):
        raise SplitFoldError("CoefsNotPowerOfTwo")
    el = n.bit_length() - 1
    if len(rhos) != el:
        raise SplitFoldError("PointsLenMismatch")
    f = [c % P for c in coef]
    fs = [f]
    for i in range(el):
        f = [(f[2 * k] + rhos[i] * f[2 * k + 1]) % P for k in range(len(f) // 2)]
        fs.append(f)
    return fs


def poly_eval(coef, x):
    """Polynomial::eval (polynomial.rs:120-128)"""
    acc = 0
    for c in reversed(coef):
        acc = (acc * x + c) % P
    return acc


def debug_verify(rhos, mu, polys, beta):
    """gemini.rs:206-232: 2 beta f_{j+1}(beta^2) = beta (f_j(beta) + f_j(-beta)) + rho_j (f_j(beta) - f_j(-beta)), with
    f_el(beta^2) replaced by mu."""
    el = len(rhos)
    es = [poly_eval(f, beta) for f in polys[:el]]
    es_neg = [poly_eval(f, neg(beta)) for f in polys[:el]]
    es_hat = [poly_eval(f, beta * beta % P) for f in polys[1:el]] + [mu % P]
    return gemini_relation(rhos, beta, es, es_neg, es_hat)


def gemini_relation(rhos, beta, es, es_neg, es_hat):
    """the value-level part of verify_gemini (gemini.rs:188-203)"""
    return all(2 * beta * es_hat[j] % P == (beta * (es[j] + es_neg[j]) + rhos[j] * (es[j] - es_neg[j])) % P for j in range(len(rhos)))


def quotient3(coef, us):
    """(f - I) / prod(X - u) of batch_open_kzg (kzg.rs:74-88) as successive synthetic divisions (I = f mod Z, so the quotient of
    the exact division is the quotient of f by Z).  Trailing zeros do not matter to the MSM."""
    q = list(coef)
    for u in us:
        if not q:
            break
        b, out = 0, []
        for c in reversed(q):
            b = (c + u * b) % P
            out.append(b)
        q = list(reversed(out))[1:]
    return q


# ---- sumcheck.rs: a dict-based MPolynomial (key = exponent tuple, as MPolynomial.dictionary) ---------------------------
def mpoly_evaluate(g, point):
    """MPolynomial::evaluate: sum_k c_k prod_i point[i]^k[i] (0^0 = 1)"""
    acc = 0
    for key, c in g.items():
        t = c
        for i, e in enumerate(key):
            t = t * pow(point[i], e, P) % P
        acc = (acc + t) % P
    return acc


def mpoly_partial_evaluate(g, h):
    """MPolynomial::partial_evaluate: variables i in h are replaced by h[i]; the key keeps its length with exponent 0 there."""
    out = {}
    for key, c in g.items():
        t = c
        nk = list(key)
        for i, v in h.items():
            if i < len(key):
                t = t * pow(v, key[i], P) % P
                nk[i] = 0
        nk = tuple(nk)
        out[nk] = (out.get(nk, 0) + t) % P
    return out


def mpoly_add(a, b):
    out = dict(a)
    for k, v in b.items():
        out[k] = (out.get(k, 0) + v) % P
    return out


def num_vars(g):
    return max((len(k) for k in g), default=0)


def bit_combinations(length):
    """BitCombinations (sumcheck.rs:16-55): bit i of the counter is entry i"""
    for n in range(1 << length):
        yield [(n >> i) & 1 for i in range(length)]


def sum_over_boolean_hypercube(g):
    """sumcheck.rs:57-66"""
    el = num_vars(g)
    return sum(mpoly_evaluate(g, c) for c in bit_combinations(el)) % P


def build_gj_from_prefix(g, rs):
    """sumcheck.rs:68-87, literally: sum over the boolean assignments of the variables after j of g with variables < j set to rs."""
    el = num_vars(g)
    j = len(rs)
    assert el >= 1 and el > j, "invalid sizes for sum-check round"
    gj = {}
    for c in bit_combinations(el - 1 - j):
        h = {i: v for i, v in enumerate(rs)}
        for i, v in enumerate(c):
            h[i + 1 + j] = v
        gj = mpoly_add(gj, mpoly_partial_evaluate(g, h))
    return gj


def gj_coefficients(gj, j):
    """(A, B) of g_j(X_j) = A + B X_j: the constant term and X_j's coefficient (every other exponent is 0 after the partial
    evaluation; a multilinear g has no X_j^2)"""
    a = b = 0
    for key, c in gj.items():
        e = key[j]
        assert all(x == 0 for i, x in enumerate(key) if i != j) and e <= 1
        if e == 0:
            a = (a + c) % P
        else:
            b = (b + c) % P
    return a, b


def sumcheck_fold(gj, j, el):
    """sumcheck.rs:89-95: g_j(e_j) + g_j(0)"""
    one = [0] * el
    one[j] = 1
    return (mpoly_evaluate(gj, one) + mpoly_evaluate(gj, [0] * el)) % P


def get_coefs_in_order(g):
    """sumcheck.rs:97-108"""
    el = num_vars(g)
    return [g.get(tuple(c), 0) % P for c in bit_combinations(el)]


def mpoly_from_coefs(coefs):
    el = len(coefs).bit_length() - 1
    return {tuple((t >> i) & 1 for i in range(el)): c % P for t, c in enumerate(coefs) if c % P}


# ---- closed forms (what the device computes) -------------------------------------------------------------------------
def hypercube_sum_closed(coefs):
    """h = sum_t c[t] 2^(el - popcount t): a variable with exponent 0 contributes g(..0..) + g(..1..) = 2 times"""
    el = len(coefs).bit_length() - 1
    return sum(c * (1 << (el - bin(t).count("1"))) for t, c in enumerate(coefs)) % P


def round_message_closed(fj, el, j):
    """A_j, B_j from the fold level f_j (2^(el - j) elements), m = el - 1 - j"""
    m = el - 1 - j
    a = sum(fj[t] * (1 << (m - bin(t >> 1).count("1"))) for t in range(0, len(fj), 2)) % P
    b = sum(fj[t] * (1 << (m - bin(t >> 1).count("1"))) for t in range(1, len(fj), 2)) % P
    return a, b


# ---- transcript stand-in ---------------------------------------------------------------------------------------------
def sample(data):
    """FqOrder::sample (field.rs:272-278): acc = (acc << 8) ^ b in a usize (64 bits: the high bytes fall off), then mod P"""
    acc = 0
    for b in data:
        acc = ((acc << 8) ^ b) & 0xFFFFFFFFFFFFFFFF
    return acc % P


class Transcript:
    """A deterministic stand-in for FiatShamirTransformer (fiat_shamir.rs): SHAKE256 over a canonical serialization of everything
    pushed so far -- el as u64 LE, h as 32 bytes LE, each g_j as A_j || B_j (64 bytes LE) -- 32 bytes squeezed, folded by
    `sample`.  The reference's own bytes (bincode of a HashMap-backed MPolynomial) cannot be reproduced; the ABI leaves the
    transcript to the caller for that reason."""

    def __init__(self):
        self.items = []

    def push(self, b):
        self.items.append(bytes(b))

    def challenge(self):
        blob = b"".join(len(x).to_bytes(8, "little") + x for x in self.items)
        return sample(hashlib.shake_256(blob).digest(32))


def fe_bytes(v):
    return int(v).to_bytes(32, "little")


def sumcheck_rounds(coefs, transcript=None):
    """the transcript half of prove_sumcheck (sumcheck.rs:128-156) over the closed-form round messages: returns (h, gs, rs, beta).
    beta is sampled from the unchanged stream right after r_{el-1}: beta == r_{el-1}."""
    t = transcript or Transcript()
    el = len(coefs).bit_length() - 1
    h = hypercube_sum_closed(coefs)
    t.push(el.to_bytes(8, "little"))
    t.push(fe_bytes(h))
    gs, rs = [], []
    f = [c % P for c in coefs]
    for j in range(el):
        a, b = round_message_closed(f, el, j)
        gs.append((a, b))
        t.push(fe_bytes(a) + fe_bytes(b))
        r = t.challenge()
        rs.append(r)
        f = [(f[2 * k] + r * f[2 * k + 1]) % P for k in range(len(f) // 2)]
    beta = t.challenge()
    return h, gs, rs, beta


class ModelChallenge:
    """the library's callback side of the same transcript: challenge(round, g) as myzkp_amd.Srs.sumcheck_prove calls it"""

    def __init__(self, el, h):
        self.t = Transcript()
        self.t.push(el.to_bytes(8, "little"))
        self.t.push(fe_bytes(h))

    def __call__(self, rnd, g):
        if g is not None:
            self.t.push(fe_bytes(g[0]) + fe_bytes(g[1]))
        return self.t.challenge()


def verify_sumcheck_values(h, gs, rs, beta, ys):
    """the value-level checks of verify_sumcheck (sumcheck.rs:169-215): h = g_0(0) + g_0(1); g_{j-1}(r_{j-1}) = g_j(0) + g_j(1);
    then verify_gemini's relation (gemini.rs:188-203) with rhos = rs and mu = g_{el-1}(r_{el-1}).  ys[i] = (f_i(beta),
    f_i(-beta), f_i(beta^2))."""
    el = len(gs)
    if h % P != (2 * gs[0][0] + gs[0][1]) % P:
        return False
    for j in range(1, el):
        a, b = gs[j - 1]
        if (a + b * rs[j - 1]) % P != (2 * gs[j][0] + gs[j][1]) % P:
            return False
    mu = (gs[el - 1][0] + gs[el - 1][1] * rs[el - 1]) % P
    es = [y[0] for y in ys]
    es_neg = [y[1] for y in ys]
    es_hat = [y[2] for y in ys[1:]] + [mu]
    return gemini_relation(rs, beta, es, es_neg, es_hat)


# the polynomial of sumcheck.rs test_sumcheck_pipeline / test_first_round
PIPELINE_G = {(0, 0, 0): 1, (1, 0, 0): 2, (0, 1, 0): 3, (0, 1, 1): 4, (1, 1, 1): 5}


# ---- trapdoor identities (GPU tests): with powers_1[i] = alpha^i G every KZG point is a known multiple of G --------------
def trapdoor_check(levels, beta, alpha, max_d, commits, ys, ws, deg):
    """C_i = f_i(alpha) G, deg_i = f_i(alpha) alpha^(max_d - d_i) G, w_i = ((f_i(alpha) - I_i(alpha)) / Z_i(alpha)) G with I_i the
    interpolant of (beta, -beta, beta^2) -> ys[i] and Z_i = (X - beta)(X + beta)(X - beta^2); ys[i] = f_i at the three points.
    levels: (len, 4) limb arrays."""
    import orc
    el = len(levels) - 1
    us = [beta, neg(beta), beta * beta % P]
    G = (1, 2)
    for i, f in enumerate(levels):
        fa = orc.poly_eval(orc.FR, f, alpha)
        d = len(f)
        assert commits[i] == orc.ec_mul(0, G, fa), ("commit", i)
        assert deg[i] == orc.ec_mul(0, G, fa * pow(alpha, max_d - d, P) % P), ("deg", i)
        if i == el:
            continue
        assert tuple(ys[i]) == tuple(orc.poly_eval(orc.FR, f, u) for u in us), ("ys", i)
        ia = 0
        for k in range(3):
            t = ys[i][k]
            for m in range(3):
                if m != k:
                    t = t * (alpha - us[m]) % P * pow((us[k] - us[m]) % P, P - 2, P) % P
            ia = (ia + t) % P
        za = (alpha - us[0]) * (alpha - us[1]) % P * (alpha - us[2]) % P
        q = (fa - ia) * pow(za, P - 2, P) % P
        assert ws[i] == (orc.ec_mul(0, G, q) if d > 2 else (0, 0)), ("w", i)
