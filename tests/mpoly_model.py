"""Pure-Python restatement of the polynomial algebra between the transforms of FastStark::prove: Polynomial add / mul / pow with the
reference's trimming (algebra/polynomial.rs), MPolynomial as a dict of exponent tuples with evaluate_symbolic and lift
(algebra/mpolynomials.rs), the Rescue-Prime AIR (zkstark/rescueprime.rs:454-519) and the weighted combination of the quotients
(zkstark/fast_stark.rs:301-326).  Paths relative to myzkp/src/modules/.  Field elements are Python ints mod p; a Polynomial is a list
of ints in ascending degree.  The GPU tests and the golden-vector generator check the library against this model;
tests/test_mpoly_model.py checks the model against the reference's own tests."""

FR_P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
M128_P = 270497897142230380135924736767050121217
M128_GEN = 85408008396924667383611388730472331217     # order 2^119 (zkstark/fri.rs:423-447)


def m128_root(log2n):
    """get_nth_root_of_m128 (fri.rs:423-447)"""
    r = M128_GEN
    for _ in range(119 - log2n):
        r = r * r % M128_P
    return r


# ---- polynomial.rs ---------------------------------------------------------------------------------------------------------------
def trim(c):
    """trim_trailing_zeros"""
    n = len(c)
    while n and c[n - 1] == 0:
        n -= 1
    return list(c[:n])


def padd(a, b, p):
    """add_ref (polynomial.rs:214-228): trims"""
    n = max(len(a), len(b))
    return trim([((a[i] if i < len(a) else 0) + (b[i] if i < len(b) else 0)) % p for i in range(n)])


def pmul(a, b, p):
    """mul_ref (polynomial.rs:302-316): schoolbook, trims.  The reference sizes the result by the DEGREES and indexes it by the lengths, so an
    untrimmed operand panics there; the model trims first (the library accepts untrimmed operands and must give the same polynomial)."""
    a, b = trim(a), trim(b)
    if not a or not b:
        return []
    r = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                r[i + j] = (r[i + j] + x * y) % p
    return trim(r)


def ppow(a, e, p):
    """pow (polynomial.rs:338-372): pow(0) is one even for the zero polynomial; pow(1) is a clone; binary from the top bit"""
    if not trim(a):
        return [1] if e == 0 else []
    if e == 0:
        return [1]
    if e == 1:
        return list(a)
    if len(a) == 1:
        return [pow(a[0], e, p)]                # a constant: the same value without e's bits of polynomial products
    acc = [1]
    for bit in bin(e)[2:]:
        acc = pmul(acc, acc, p)
        if bit == "1":
            acc = pmul(acc, a, p)
    return acc


def peval(c, x, p):
    """eval (polynomial.rs:120-128)"""
    acc = 0
    for v in reversed(c):
        acc = (acc * x + v) % p
    return acc


def pscale(c, f, p):
    """scale (polynomial.rs:167-174)"""
    return [pow(f, i, p) * v % p for i, v in enumerate(c)]


def interpolate(xs, ys, p):
    """Polynomial::interpolate (polynomial.rs:177-199) as the same polynomial by Newton-free Lagrange sums: sum_j y_j prod_{i != j} (X - x_i) /
    (x_j - x_i), trimmed by the final additions"""
    num = [1]
    for x in xs:
        num = pmul(num, [(-x) % p, 1], p)
    res = []
    for j, xj in enumerate(xs):
        den = 1
        for i, xi in enumerate(xs):
            if i != j:
                den = den * (xj - xi) % p
        # num / (X - x_j): synthetic division
        q, carry = [0] * (len(num) - 1), 0
        for k in range(len(num) - 1, 0, -1):
            carry = (num[k] + carry * xj) % p
            q[k - 1] = carry
        w = ys[j] * pow(den, -1, p) % p
        res = padd(res, [v * w % p for v in q], p)
    return res


# ---- mpolynomials.rs: {exponent tuple: coefficient} ---------------------------------------------------------------------------------
def mzero():
    return {}


def mconstant(c, p):
    """constant (mpolynomials.rs:49-57): one variable wide; zero is the empty dictionary"""
    return {(0,): c % p} if c % p else {}


def mvariables(n):
    """variables (mpolynomials.rs:59-73)"""
    return [{tuple(1 if j == i else 0 for j in range(n)): 1} for i in range(n)]


def _width(a, b):
    return max([len(k) for k in a] + [len(k) for k in b] + [0])


def _pad(k, n):
    return tuple(k) + (0,) * (n - len(k))


def madd(a, b, p):
    """Add (mpolynomials.rs:204-243): keys padded to the wider operand; a sum that vanishes is removed"""
    n = _width(a, b)
    d = {_pad(k, n): v for k, v in a.items()}
    for k, v in b.items():
        k = _pad(k, n)
        if k in d:
            d[k] = (d[k] + v) % p
            if d[k] == 0:
                del d[k]
        else:
            d[k] = v
    return d


def mmul(a, b, p):
    """Mul (mpolynomials.rs:254-302)"""
    n = _width(a, b)
    d = {}
    for k0, v0 in a.items():
        for k1, v1 in b.items():
            k = tuple(x + y for x, y in zip(_pad(k0, n), _pad(k1, n)))
            v = v0 * v1 % p
            if k in d:
                d[k] = (d[k] + v) % p
                if d[k] == 0:
                    del d[k]
            else:
                d[k] = v
    return d


def mneg(a, p):
    return {k: (-v) % p for k, v in a.items()}


def msub(a, b, p):
    return madd(a, mneg(b, p), p)


def mis_zero(a):
    return all(v == 0 for v in a.values())


def mpow(a, e, p):
    """pow (mpolynomials.rs:76-101)"""
    if mis_zero(a):
        return {}
    n = len(next(iter(a)))
    acc = {(0,) * n: 1}
    for bit in bin(e)[2:]:
        acc = mmul(acc, acc, p)
        if bit == "1":
            acc = mmul(acc, a, p)
    return acc


def lift(poly, index, p):
    """lift (mpolynomials.rs:143-164): sum_i coef_i x_index^i over index + 1 variables"""
    if not trim(poly):
        return {}
    x = mvariables(index + 1)[index]
    acc = {}
    for i, c in enumerate(poly):
        acc = madd(acc, mmul(mconstant(c, p), mpow(x, i, p), p), p)
    return acc


def evaluate_symbolic(a, point, p):
    """evaluate_symbolic (mpolynomials.rs:125-141), term by term"""
    acc = []
    for k, v in a.items():
        prod = [v]
        for i in range(len(k)):
            prod = pmul(prod, ppow(point[i], k[i], p), p)
        acc = padd(acc, prod, p)
    return acc


def terms_of(a):
    """the flat term list of the library's ABI: [(coefficient, exponents)] in a fixed order"""
    return [(v, k) for k, v in sorted(a.items())]


def compose_terms(terms, point, p):
    """the same sum over a flat term list (duplicate exponent rows add up, zero coefficients allowed)"""
    acc = []
    for c, k in terms:
        prod = [c % p]
        for i in range(len(k)):
            prod = pmul(prod, ppow(point[i], k[i], p), p)
        acc = padd(acc, prod, p)
    return acc


def degree_bounds(constraints, lens):
    """the library's host plan: D_a + 1 per constraint (0 without a non-vanishing term), max over them, N"""
    bounds = []
    for terms in constraints:
        b = 0
        for _, k in terms:
            if any(e and lens[i] == 0 for i, e in enumerate(k)):
                continue
            b = max(b, 1 + sum(e * (lens[i] - 1) for i, e in enumerate(k) if e))
        bounds.append(b)
    smin = max(bounds + [0])
    n = 1
    while n < smin:
        n *= 2
    return (n if constraints else 0), smin, bounds


# ---- rescueprime.rs ------------------------------------------------------------------------------------------------------------------
class RescuePrime:
    def __init__(self, par):
        self.p = M128_P
        self.m, self.n, self.alpha, self.alphainv = par["m"], par["n"], int(par["alpha"]), int(par["alphainv"])
        self.mds = [[int(v) for v in row] for row in par["mds"]]
        self.mdsinv = [[int(v) for v in row] for row in par["mdsinv"]]
        self.rc = [int(v) for v in par["round_constants"]]

    def trace(self, x):
        """trace (rescueprime.rs): the state before round 0 and after every round: n + 1 rows"""
        p, m = self.p, self.m
        state = [x % p] + [0] * (m - 1)
        rows = [list(state)]
        for r in range(self.n):
            for half, e in ((0, self.alpha), (1, self.alphainv)):
                state = [pow(s, e, p) for s in state]
                state = [(sum(self.mds[i][j] * state[j] for j in range(m)) + self.rc[2 * r * m + half * m + i]) % p for i in range(m)]
            rows.append(list(state))
        return rows

    def round_constants_polynomials(self, omicron):
        """rescueprime.rs:454-484"""
        p, m = self.p, self.m
        dom = [pow(omicron, r, p) for r in range(self.n)]
        first = [lift(interpolate(dom, [self.rc[2 * r * m + i] for r in range(self.n)], p), 0, p) for i in range(m)]
        second = [lift(interpolate(dom, [self.rc[2 * r * m + m + i] for r in range(self.n)], p), 0, p) for i in range(m)]
        return first, second

    def transition_constraints(self, omicron):
        """rescueprime.rs:486-519: variables (X, previous state, next state)"""
        p, m = self.p, self.m
        first, second = self.round_constants_polynomials(omicron)
        v = mvariables(1 + 2 * m)
        prev, nxt = v[1:1 + m], v[1 + m:1 + 2 * m]
        air = []
        for i in range(m):
            lhs = mconstant(0, p)
            for k in range(m):
                lhs = madd(lhs, mmul(mconstant(self.mds[i][k], p), mpow(prev[k], self.alpha, p), p), p)
            lhs = madd(lhs, first[i], p)
            rhs = mconstant(0, p)
            for k in range(m):
                rhs = madd(rhs, mmul(mconstant(self.mdsinv[i][k], p), msub(nxt[k], second[k], p), p), p)
            rhs = mpow(rhs, self.alpha, p)
            air.append(msub(lhs, rhs, p))
        return air


# ---- fast_stark.rs:301-326 -----------------------------------------------------------------------------------------------------------
def lincomb_reference(polys, weights, shifts, p):
    """combination = sum_i [w_i] * (x.pow(s_i) * p_i) with the reference's Polynomial arithmetic (a plain term has shift 0)"""
    x = [0, 1]
    comb = []
    for q, w, s in zip(polys, weights, shifts):
        term = pmul(ppow(x, s, p), q, p) if s else list(q)
        comb = padd(comb, pmul([w % p], term, p), p)
    return comb


def lincomb(polys, weights, shifts, p):
    """what the kernel computes: out[j] = sum_i w_i p_i[j - s_i], trimmed"""
    n = max([len(q) + s for q, s in zip(polys, shifts)] + [0])
    out = [0] * n
    for q, w, s in zip(polys, weights, shifts):
        for j, v in enumerate(q):
            out[j + s] = (out[j + s] + w * v) % p
    return trim(out)
