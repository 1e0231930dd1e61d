"""The case table of mzk_mpoly_hypercube_evals, shared by the model's own test (CPU) and the library's (GPU): per case a name, el and
a list of factors, each a list of terms (coefficient, exponent tuple).  Built once per el and never modified.

el: 0, 1, 2 and 9 are one partial tile, 10 exactly one tile, 11, 12 and 13 are 2, 4 and 8 tiles with 1 to 3 high bits; the scatter form's
butterfly has one pass up to el = 10 and two above."""
import functools, random
import hypercube_model as hm

P = hm.P
ELS = (0, 1, 2, 9, 10, 11, 12, 13)
G = hm.TILE_LOG


def exps_of_mask(m, el, rng=None):
    """an exponent row with support m: exponent 1, or 1..4 with rng"""
    return tuple((rng.randrange(1, 5) if rng else 1) if (m >> (el - 1 - i)) & 1 else 0 for i in range(el))


def sparse(rng, el, count, mask_and=None, mask_or=0):
    """count terms with random coefficients on random supports, restricted to the bits of mask_and"""
    full = (1 << el) - 1
    keep = full if mask_and is None else mask_and
    return [(rng.randrange(P), exps_of_mask((rng.randrange(1 << el) & keep) | mask_or, el, rng)) for _ in range(count)]


def shape_factors(el, rng):
    """one factor per term shape of the issue's list, in this order"""
    full = (1 << el) - 1
    low = full & ((1 << G) - 1)
    high = full & ~low
    c = lambda: rng.randrange(1, P)
    out = [("no_terms", []),
           ("constant", [(c(), (0,) * el)]),
           ("full_mask", [(c(), (1,) * el)]),
           ("dup_equal_rows", [(c(), exps_of_mask(full >> 1, el)), (c(), exps_of_mask(full >> 1, el)), (c(), (0,) * el)]),
           ("zero_coefficient", [(0, exps_of_mask(full, el)), (c(), exps_of_mask(1, el)), (0, (0,) * el)]),
           ("low_bits_only", sparse(rng, el, 37, low)),
           ("mixed", sparse(rng, el, 61)),
           ("chain_pm1", [(P - 1, exps_of_mask((1 << j) - 1, el)) for j in range(el + 1)] + [(P - 1, exps_of_mask(low >> 1, el, rng)) for _ in range(64)])]
    if el >= 1:
        v = el // 2
        lifted = lambda d: tuple(d if i == v else 0 for i in range(el))
        out.append(("lifted_univariate", [(c(), lifted(d)) for d in range(0, 8)]))
        # x0^2 and x0^5 are different keys of a HashMap and the same support
        out.append(("dup_same_support", [(c(), (2,) + (0,) * (el - 1)), (c(), (5,) + (0,) * (el - 1)), (c(), (1,) + (0,) * (el - 1))]))
        out.append(("short_keys", [(c(), (1,)), (c(), ()), (c(), (0, 3)[:el])]))
    if high:
        out.append(("high_bits_only", sparse(rng, el, 29, high)))
        # groups by high mask: 0 fits every tile, the lowest high bit fits every other tile, the full high mask fits the last tile alone
        out.append(("groups_some_tiles_and_last", sparse(rng, el, 9, low) + sparse(rng, el, 9, low, 1 << G) + sparse(rng, el, 9, low, high)))
    return out


@functools.lru_cache(maxsize=None)
def cases(el):
    """[(name, factors)] for one el"""
    rng = random.Random(77000 + el)
    shapes = shape_factors(el, rng)
    out = [("shapes", [terms for _, terms in shapes])]
    # each single variable alone, one factor each: pins the MSB-first order (x_0 <-> bit el-1)
    if el >= 1:
        out.append(("each_variable", [[(1 + i, tuple(1 if j == i else 0 for j in range(el)))] for i in range(el)]))
    for k in (1, 2, 3, 8):
        out.append(("k%d_unequal_counts" % k, [sparse(rng, el, 1 + 13 * f * f + (el if f % 2 else 0)) for f in range(k)]))
    out.append(("empty_between_full", [sparse(rng, el, 40), [], sparse(rng, el, 23)]))
    if el <= 11:
        n = 1 << el
        order = list(range(n))
        rng.shuffle(order)
        dense = [(rng.randrange(P), exps_of_mask(m, el)) for m in order]
        # every coefficient p - 1, every mask, and 64 more rows on the empty mask: the last entry is a sum of 2^el + 64 values of p - 1
        dense_pm1 = [(P - 1, exps_of_mask(m, el)) for m in range(n)] + [(P - 1, (0,) * el)] * 64
        out.append(("dense", [dense, dense_pm1]))
    return tuple(out)


def all_cases():
    return [(el, name) for el in ELS for name, _ in cases(el)]


def get(el, name):
    return dict(cases(el))[name]


@functools.lru_cache(maxsize=None)
def expected(el, name):
    """the model's tables, one list of 2^el ints per factor: computed once, shared, never modified"""
    return tuple(tuple(hm.evals(terms, el)) for terms in get(el, name))
