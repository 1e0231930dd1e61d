"""tests/hypercube_model.py against itself and against tests/sumcheck_product_model.py: the table by masks and subset sums equals the
literal MPolynomial.evaluate (pow, 0^0 = 1) on every case of tests/hypercube_cases.py, equals evals_over_boolean_hypercube on dense
multilinear inputs, and the case table has the shapes the GPU test relies on.  CPU only.

evaluate_direct costs (terms x el) per point.  A case whose terms x points stay below 2^17 is compared at every point; a larger one
at the corners, every single-variable point, every point with one variable off, and 48 seeded random points."""
import random
import pytest
import hypercube_cases as hc
import hypercube_model as hm
import sumcheck_product_model as sm

P = hm.P


def points_of(el, n_terms):
    n = 1 << el
    if n * max(n_terms, 1) <= 1 << 17:
        return list(range(n))
    rng = random.Random(el * 1000 + n_terms)
    pts = {0, n - 1} | {1 << i for i in range(el)} | {(n - 1) ^ (1 << i) for i in range(el)} | {rng.randrange(n) for _ in range(48)}
    return sorted(pts)


@pytest.mark.parametrize("el,name", hc.all_cases())
def test_evals_equals_the_literal_evaluation(el, name):
    for terms, table in zip(hc.get(el, name), hc.expected(el, name)):
        assert len(table) == 1 << el and all(0 <= v < P for v in table)
        pts = points_of(el, len(terms))
        assert [table[b] for b in pts] == hm.evals_direct(terms, el, pts)


@pytest.mark.parametrize("el", [0, 1, 2, 5, 9])
def test_dense_multilinear_equals_the_butterfly(el):
    rng = random.Random(el)
    coef = [rng.randrange(P) for _ in range(1 << el)]
    terms = [(c, hc.exps_of_mask(m, el)) for m, c in enumerate(coef)]
    rng.shuffle(terms)
    assert hm.evals(terms, el) == sm.evals_over_boolean_hypercube(coef, el)
    for b in (0, (1 << el) - 1, (1 << el) // 3):
        assert hm.evaluate_direct(terms, el, b) == sm.eval_monomials_direct(coef, el, b)


def test_reference_demo_shape():
    """main.rs builds its factors over every 0/1 key of el = 8 variables; el = 6 here"""
    el = 6
    rng = random.Random(6)
    factors = [[(rng.randrange(256), tuple((m >> (el - 1 - i)) & 1 for i in range(el))) for m in range(1 << el)] for _ in range(3)]
    for terms in factors:
        assert hm.evals(terms, el) == hm.evals_direct(terms, el)
    tables = [hm.evals(t, el) for t in factors]
    proof = sm.prove(tables, 3)
    assert sm.verify(tables, 3, (), proof["sum"], proof["transcript"])


def test_msb_first_order_and_zero_power():
    el = 4
    for i in range(el):
        table = hm.evals([(7, tuple(1 if j == i else 0 for j in range(el)))], el)
        assert table == [7 if (b >> (el - 1 - i)) & 1 else 0 for b in range(1 << el)]
    assert hm.evals([(5, (0, 0, 0, 0))], el) == [5] * 16                      # 0^0 = 1 at every point
    assert hm.evals([(3, (2,)), (4, (5,))], 1) == [0, 7] == hm.evals_direct([(3, (2,)), (4, (5,))], 1)
    assert hm.evals([], 3) == [0] * 8


def test_case_table_covers_the_issue():
    assert hc.ELS == (0, 1, 2, 9, 10, 11, 12, 13)
    for el in hc.ELS:
        names = [n for n, _ in hc.cases(el)]
        assert {"shapes", "k1_unequal_counts", "k2_unequal_counts", "k3_unequal_counts", "k8_unequal_counts", "empty_between_full"} <= set(names)
        assert ("dense" in names) == (el <= 11)
        shapes = dict(hc.shape_factors(el, random.Random(0)))
        assert ("high_bits_only" in shapes) == (el > 10) == ("groups_some_tiles_and_last" in shapes)
        k8 = hc.get(el, "k8_unequal_counts")
        assert len(k8) == 8 and len({len(t) for t in k8}) == 8
        assert hc.get(el, "empty_between_full")[1] == []
    # the reduction case: the last entry of the all-(p-1) dense factor is a sum of 2^el + 64 values of p - 1
    for el in (0, 9, 11):
        assert hc.expected(el, "dense")[1][-1] == ((1 << el) + 64) * (P - 1) % P
    # groups: high mask 0 fits every tile, the lowest high bit every other tile, the full high mask the last tile alone
    el = 13
    pl = hm.plan([[e for _, e in dict(hc.shape_factors(el, random.Random(77000 + el)))["groups_some_tiles_and_last"]]], el)
    his = [h for h, _ in pl["factors"][0]["groups"]]
    assert his == [0, 1, 7]


def test_plan_model_on_a_hand_example():
    el = 12
    exps = [[hc.exps_of_mask(m, el) for m in (0x801, 0x001, 0x801, 0xC00, 0x001, 0x002)], [], [hc.exps_of_mask(0xFFF, el)]]
    pl = hm.plan(exps, el)
    f0 = pl["factors"][0]
    assert f0["masks"] == [0x001, 0x002, 0x801, 0xC00] and f0["segments"] == [[1, 4], [5], [0, 2], [3]] and f0["groups"] == [(0, 2), (2, 1), (3, 1)]
    assert pl["factors"][1] == {"masks": [], "segments": [], "groups": []}
    assert pl["factors"][2]["segments"] == [[6]]
    assert pl["form"] == hm.TILE and (pl["grid_x"], pl["grid_y"], pl["launches"], pl["memsets"]) == (4, 3, 1, 0)
    sc = hm.plan(exps, el, hm.SCATTER)
    assert (sc["grid_x"], sc["grid_y"], sc["launches"], sc["memsets"], sc["mle_passes"]) == (1, 3, 1 + 3 * 2, 1, 2)
    assert sc["upload_bytes"] == 4 * (12 + 8 * 5) and pl["upload_bytes"] == 4 * (20 + 8 * 5)
