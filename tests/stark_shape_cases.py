"""The AIR shapes tests/test_gpu_stark_shapes.py proves with mzk_stark_prove, and their seeded inputs.  tests/test_stark_shape_cases.py
checks on the CPU, with the model alone, that every case plans, satisfies its constraints and verifies, and that the table reaches
every branch of the prover it is there for.  Needs no GPU and no library.

A parametric AIR over (X, prev_0 .., next_0 ..): register s evolves as next_s = prev_s^deg + prev_((s+1) mod m) [+ X for s = 0];
extra constraint j is X^(j+1) times constraint j mod m (the same trace satisfies it, its degree bound is j + 1 higher).  A boundary
is a list of cells (cycle, register), a negative cycle counting from T; the values are read off the trace.  Every boundary contains
a cell at cycle T - 1 (the verifier derives the trace length from the largest boundary cycle) and no cell twice.  No FRI domain
exceeds 2048 elements: the model's transforms are quadratic."""
import collections, functools, random
import mpoly_model as mm
import stark_model as sm

FR, M128 = 0, 1
MOD = {FR: mm.FR_P, M128: mm.M128_P}
LIMBS = {FR: 4, M128: 2}
COSET = {FR: 5, M128: mm.M128_GEN}                 # the offset of the FRI domain
FR_OMEGA28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904      # order 2^28
MAX_FRI_DOMAIN = 2048

Case = collections.namedtuple("Case", "name field m deg e checks T use_x extra cells kind")


def _c(name, field, m, deg, e, checks, T, use_x, extra, cells, kind="air"):
    return Case(name, field, m, deg, e, checks, T, bool(use_x), extra, tuple(cells), kind)


SAME = ((0, 0), (0, 1), (-1, 0))
TABLE = [
    _c("01-m1-deg1-T2-prefix-small", M128, 1, 1, 4, 1, 2, 1, 0, [(-1, 0)]),
    _c("02-m1-deg1-e2-T4-tree-degree7", M128, 1, 1, 2, 1, 4, 0, 0, [(0, 0), (-1, 0)]),
    _c("03-m1-deg1-T10-prefix-zerofier-shift0", M128, 1, 1, 4, 1, 10, 1, 0, [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (-1, 0)]),
    _c("04-fr-m2-deg1-T9-prefix15", FR, 2, 1, 4, 2, 9, 1, 0, [(0, 0), (0, 1), (-1, 1)]),
    _c("05-m3-deg1-e8-c8-T32", M128, 3, 1, 8, 8, 32, 1, 0, [(0, 0), (-1, 2)]),
    _c("06-m1-deg2-T6", M128, 1, 2, 4, 1, 6, 0, 0, [(0, 0), (-1, 0)]),
    _c("07-fr-m1-deg3-e2-T10-extra1", FR, 1, 3, 2, 2, 10, 1, 1, [(-1, 0)]),
    _c("08-m2-deg2-e1-T10", M128, 2, 2, 1, 2, 10, 0, 0, SAME),
    _c("09-m2-deg2-e2-T23-rl31", M128, 2, 2, 2, 2, 23, 1, 0, SAME),
    _c("10-m2-deg2-e4-T24-rl32", M128, 2, 2, 4, 2, 24, 1, 0, SAME),
    _c("11-m2-deg2-e16-c1-T5", M128, 2, 2, 16, 1, 5, 1, 0, [(0, 1), (-1, 0)]),
    _c("12-m2-deg4-e8-T5-extra2", M128, 2, 4, 8, 1, 5, 1, 2, [(0, 0), (-1, 0)]),
    _c("13-fr-m3-deg2-c3-T20-16constraints", FR, 3, 2, 4, 3, 20, 1, 13, [(0, 0), (7, 0), (-1, 0)]),
    _c("14-m3-deg3-e8-T7-extra1", M128, 3, 3, 8, 1, 7, 0, 1, [(-1, 2)]),
    _c("15-m1-deg7-T10", M128, 1, 7, 4, 2, 10, 1, 0, [(0, 0), (-1, 0)]),
    _c("16-m2-deg2-e32-T12", M128, 2, 2, 32, 2, 12, 0, 0, [(0, 0), (-1, 1)]),
    _c("17-m3-deg2-c16-T64", M128, 3, 2, 4, 16, 64, 1, 0, [(0, 0), (3, 1), (-1, 2)]),
    _c("18-m2-deg2-c32-T100", M128, 2, 2, 4, 32, 100, 1, 0, [(0, 0), (-1, 0)]),
]
# register 1 is the constant 7 in every row, the caller's "random" rows included: a trace polynomial of length 1
DEGENERATE = [
    _c("D1-constant-register", M128, 2, 2, 4, 2, 10, 1, 0, [(0, 0), (-1, 0)], "constant"),
    _c("D2-zero-boundary-quotient", M128, 2, 2, 4, 2, 10, 1, 0, [(0, 1), (-1, 0)], "constant"),
]
# the D1 trace under [c0, next1 - prev1]: the second transition polynomial is the zero polynomial, the coset division refuses it
REFUSED = _c("R1-zero-transition-polynomial", M128, 2, 2, 4, 2, 10, 1, 0, [(0, 0), (-1, 0)], "refused")
# the same handle proves this one afterwards: register 1 random in every row, both transition polynomials non-zero (the AIR is not
# satisfied; the prover is deterministic all the same)
REFUSED_THEN = _c("R1-then-random-register", M128, 2, 2, 4, 2, 10, 1, 0, [(0, 0), (-1, 0)], "refused-random")
# three boundaries for one handle of row 10: 2 + 1, 0 + 1 and 3 + 0 entries per register
REUSE_ROW = "10-m2-deg2-e4-T24-rl32"
REUSE_BOUNDARIES = [((0, 0), (-1, 0), (0, 1)), ((-1, 1),), ((0, 0), (5, 0), (-1, 0))]
CONSTANT = 7

BY_NAME = {c.name: c for c in TABLE + DEGENERATE + [REFUSED, REFUSED_THEN]}
VERIFYING = [c.name for c in TABLE + DEGENERATE]


def root_of(field, log2n):
    """the root of unity of order 2^log2n the library uses (mzk_root_of_unity)"""
    return mm.m128_root(log2n) if field == M128 else pow(FR_OMEGA28, 1 << (28 - log2n), mm.FR_P)


def _unit(nv, i, e=1):
    return tuple(e if j == i else 0 for j in range(nv))


def _sum(p, terms):
    """MPolynomial dict of (exponents, coefficient) pairs; coinciding exponent rows add up, a sum that vanishes is removed"""
    a = {}
    for k, c in terms:
        a[k] = (a.get(k, 0) + c) % p
        if a[k] == 0:
            del a[k]
    return a


def parametric_air(p, m, deg, use_x, extra):
    nv = 1 + 2 * m
    cons = []
    for s in range(m):
        terms = [(_unit(nv, 1 + m + s), 1), (_unit(nv, 1 + s, deg), -1), (_unit(nv, 1 + (s + 1) % m), -1)]
        if use_x and s == 0:
            terms.append((_unit(nv, 0), -1))
        cons.append(_sum(p, terms))
    for j in range(extra):
        cons.append({(k[0] + j + 1,) + k[1:]: c for k, c in cons[j % m].items()})
    return cons


def parametric_trace(p, m, deg, use_x, T, omicron, rnd):
    rows, x = [[rnd.randrange(p) for _ in range(m)]], 1
    for _ in range(T - 1):
        prev = rows[-1]
        rows.append([(pow(prev[s], deg, p) + prev[(s + 1) % m] + (x if use_x and s == 0 else 0)) % p for s in range(m)])
        x = x * omicron % p
    return rows


def degenerate_air(p, refused):
    """c0 = next0 - prev0^2 - prev1 - X;  c1 = X (next1 - prev1) + c0, or next1 - prev1 alone"""
    c0 = [((0, 0, 0, 1, 0), 1), ((0, 2, 0, 0, 0), -1), ((0, 0, 1, 0, 0), -1), ((1, 0, 0, 0, 0), -1)]
    if refused:
        return [_sum(p, c0), _sum(p, [((0, 0, 0, 0, 1), 1), ((0, 0, 1, 0, 0), -1)])]
    return [_sum(p, c0), _sum(p, c0 + [((1, 0, 0, 0, 1), 1), ((1, 0, 1, 0, 0), -1)])]


def degenerate_trace(p, T, nr, omicron, rnd, random_register):
    """register 0 follows next0 = prev0^2 + prev1 + X; register 1 is CONSTANT in all T + nr rows, or random in all of them"""
    r1 = [rnd.randrange(p) if random_register else CONSTANT for _ in range(T + nr)]
    rows, x = [[rnd.randrange(p), r1[0]]], 1
    for i in range(1, T):
        u, v = rows[-1]
        rows.append([(u * u + v + x) % p, r1[i]])
        x = x * omicron % p
    return rows + [[rnd.randrange(p), r1[T + i]] for i in range(nr)]


Built = collections.namedtuple("Built", "case fid p g omicron omega air cons trace boundary false_boundary randomizer plan model")


def cells_to_boundary(cells, T, trace):
    out = [((c + T) if c < 0 else c, r) for c, r in cells]
    assert len(set(out)) == len(out) and all(0 <= c < T for c, _ in out)
    return [(c, r, trace[c][r]) for c, r in out]


@functools.lru_cache(maxsize=None)
def build(name, cells=None):
    """everything a test hands to the model and to the library for the case; cells: another boundary than the case's own"""
    c = BY_NAME[name]
    p = MOD[c.field]
    rnd = random.Random("stark shape " + ("constant register" if c.kind in ("constant", "refused") else name))     # D1, D2 and R1: one trace
    air = parametric_air(p, c.m, c.deg, c.use_x, c.extra) if c.kind == "air" else degenerate_air(p, c.kind.startswith("refused"))
    nr = 4 * c.checks
    olen = 1 << ((c.T + nr) * c.deg).bit_length()                                 # initialize_fast_stark_m128; the plan below must agree
    flen = olen * c.e
    omicron, omega = root_of(c.field, olen.bit_length() - 1), root_of(c.field, flen.bit_length() - 1)
    if c.kind == "air":
        trace = parametric_trace(p, c.m, c.deg, c.use_x, c.T, omicron, rnd) + [[rnd.randrange(p) for _ in range(c.m)] for _ in range(nr)]
    else:
        trace = degenerate_trace(p, c.T, nr, omicron, rnd, c.kind == "refused-random")
    boundary = cells_to_boundary(c.cells if cells is None else cells, c.T, trace)
    false_boundary = boundary[:-1] + [(boundary[-1][0], boundary[-1][1], (boundary[-1][2] + 1) % p)]
    plan = sm.plan(p, c.e, c.checks, c.m, c.T, c.deg, air, boundary)
    assert (plan["omicron_domain_length"], plan["fri_domain_length"], plan["num_randomizers"]) == (olen, flen, nr)
    randomizer = [rnd.randrange(p) for _ in range(plan["randomizer_length"])]
    model = sm.FastStark(p, COSET[c.field], omega, omicron, c.e, c.checks, c.m, c.T, c.deg)
    return Built(c, c.field, p, COSET[c.field], omicron, omega, air, [mm.terms_of(a) for a in air], trace, boundary, false_boundary, randomizer,
                 plan, model)


@functools.lru_cache(maxsize=None)
def model_proof(name, cells=None):
    """FastStark.prove of the case by the model, computed once and never changed by its users ("_debug" holds the intermediates)"""
    b = build(name, cells)
    return b.model.prove(b.trace, b.boundary, b.air, b.randomizer)


def next_pow2(n):
    return 1 if n <= 1 else 1 << (n - 1).bit_length()


PREFIX_MAX_MISSING = 64        # mzk_poly.hip: a prefix of a power-of-two subgroup with at most this many points missing needs no subproduct tree


def routing(name):
    """which branches of the prover the case takes, from its plan and the routing rules of mzk_poly.hip / mzk_api.hip"""
    b = build(name)
    d, c = b.plan, b.case
    rl, olen = d["randomized_trace_length"], d["omicron_domain_length"]
    # the domain omicron^0 .. omicron^(n-1) is a prefix of the subgroup omicron generates only if that subgroup has next_pow2(n) elements
    prefix = lambda n: n >= 2 and next_pow2(n) == olen and olen - n <= PREFIX_MAX_MISSING
    tdeg = [len(q) - 1 for q in model_proof(name)["_debug"]["transition_polynomials"]]
    return {"field": c.field, "m": c.m, "deg": c.deg, "e": c.e, "n_constraints": d["n_constraints"], "rl": rl,
            "register_without_entry": 0 in d["boundary_counts"], "register_with_several_entries": max(d["boundary_counts"]) > 1,
            "boundary_shift_zero": 0 in d["boundary_shifts"], "unequal_transition_shifts": len(set(d["transition_shifts"])) > 1,
            "prefix_interpolation": prefix(rl), "prefix_missing": olen - rl if prefix(rl) else None, "prefix_zerofier": prefix(c.T - 1),
            "transition_degrees": tdeg, "small_division": any(0 <= t < 8 for t in tdeg), "fri_domain": d["fri_domain_length"],
            "fri_rounds": d["fri_num_rounds"], "fri_last_length": d["fri_last_length"], "num_indices": d["num_indices"], "checks": c.checks}
