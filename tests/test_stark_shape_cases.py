"""tests/stark_shape_cases.py is sound and not vacuous, shown with the model alone (tests/stark_model.py): every case plans, keeps its
transition degree bounds below the omicron domain (beyond it the reference's own coset division aliases), its trace satisfies every
constraint with Python integers, the model proves and verifies it and rejects the same trace under a false boundary; the refused
case trips the reference's assertion; and the table reaches every class of shape and every branch of the prover it is there for,
computed from the plans and the routing rules, so that pruning it cannot lose one silently.  A failure of
tests/test_gpu_stark_shapes.py is then not the table's fault.  CPU only; the comparison with mzk_stark_plan of the built library is
host-only arithmetic."""
import os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pytest
import mpoly_model as mm
import stark_model as sm
import stark_shape_cases as C


def test_table_is_the_issue_s_and_within_the_limits():
    names = [c.name for c in C.TABLE + C.DEGENERATE + [C.REFUSED, C.REFUSED_THEN]]
    assert len(names) == len(set(names)) == len(C.BY_NAME) and len(C.TABLE) >= 18
    rows = {(c.field, c.m, c.deg, c.e, c.checks, c.T, c.use_x, c.extra, c.cells) for c in C.TABLE}
    M, F = C.M128, C.FR
    same = ((0, 0), (0, 1), (-1, 0))
    for row in [(M, 1, 1, 4, 1, 2, True, 0, ((-1, 0),)), (M, 1, 1, 2, 1, 4, False, 0, ((0, 0), (-1, 0))),
                (M, 1, 1, 4, 1, 10, True, 0, ((0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (-1, 0))), (F, 2, 1, 4, 2, 9, True, 0, ((0, 0), (0, 1), (-1, 1))),
                (M, 3, 1, 8, 8, 32, True, 0, ((0, 0), (-1, 2))), (M, 1, 2, 4, 1, 6, False, 0, ((0, 0), (-1, 0))), (F, 1, 3, 2, 2, 10, True, 1, ((-1, 0),)),
                (M, 2, 2, 1, 2, 10, False, 0, same), (M, 2, 2, 2, 2, 23, True, 0, same), (M, 2, 2, 4, 2, 24, True, 0, same),
                (M, 2, 2, 16, 1, 5, True, 0, ((0, 1), (-1, 0))), (M, 2, 4, 8, 1, 5, True, 2, ((0, 0), (-1, 0))),
                (F, 3, 2, 4, 3, 20, True, 13, ((0, 0), (7, 0), (-1, 0))), (M, 3, 3, 8, 1, 7, False, 1, ((-1, 2),)), (M, 1, 7, 4, 2, 10, True, 0, ((0, 0), (-1, 0))),
                (M, 2, 2, 32, 2, 12, False, 0, ((0, 0), (-1, 1))), (M, 3, 2, 4, 16, 64, True, 0, ((0, 0), (3, 1), (-1, 2))),
                (M, 2, 2, 4, 32, 100, True, 0, ((0, 0), (-1, 0)))]:
        assert row in rows, row
    for c in C.DEGENERATE + [C.REFUSED, C.REFUSED_THEN]:
        assert (c.field, c.m, c.deg, c.e, c.checks, c.T) == (M, 2, 2, 4, 2, 10)
    assert [c.cells for c in C.DEGENERATE] == [((0, 0), (-1, 0)), ((0, 1), (-1, 0))]
    for name in C.BY_NAME:
        b = C.build(name)
        assert b.plan["fri_domain_length"] <= C.MAX_FRI_DOMAIN, name
        assert b.case.T - 1 in [c for c, _, _ in b.boundary], name
        assert len(b.trace) == b.plan["randomized_trace_length"] and all(len(row) == b.case.m for row in b.trace)
        assert all(0 <= v < b.p for row in b.trace for v in row) and all(0 <= v < b.p for v in b.randomizer)


def test_the_parametric_air_is_the_stated_recurrence():
    p = mm.M128_P
    assert C.parametric_air(p, 1, 1, False, 0) == [{(0, 0, 1): 1, (0, 1, 0): p - 2}]              # the two prev_0 terms coincide
    assert C.parametric_air(p, 2, 3, True, 1) == [{(0, 0, 0, 1, 0): 1, (0, 3, 0, 0, 0): p - 1, (0, 0, 1, 0, 0): p - 1, (1, 0, 0, 0, 0): p - 1},
                                                  {(0, 0, 0, 0, 1): 1, (0, 0, 3, 0, 0): p - 1, (0, 1, 0, 0, 0): p - 1},
                                                  {(1, 0, 0, 1, 0): 1, (1, 3, 0, 0, 0): p - 1, (1, 0, 1, 0, 0): p - 1, (2, 0, 0, 0, 0): p - 1}]
    air = C.parametric_air(p, 3, 2, True, 13)
    assert len(air) == sm.MAX_CONSTRAINTS and [min(k[0] for k in a) for a in air[3:]] == list(range(1, 14))
    c0, c1 = C.degenerate_air(p, False)
    assert c1 == {(0, 0, 0, 1, 0): 1, (0, 2, 0, 0, 0): p - 1, (0, 0, 1, 0, 0): p - 1, (1, 0, 0, 0, 0): p - 1, (1, 0, 0, 0, 1): 1, (1, 0, 1, 0, 0): p - 1}
    assert C.degenerate_air(p, True) == [c0, {(0, 0, 0, 0, 1): 1, (0, 0, 1, 0, 0): p - 1}]


def _constraint_at(a, point, p):
    acc = 0
    for k, c in a.items():
        t = c
        for v, e in zip(point, k):
            t = t * pow(v, e, p) % p
        acc = (acc + t) % p
    return acc


@pytest.mark.parametrize("name", C.VERIFYING)
def test_case_plans_satisfies_its_air_and_verifies_in_the_model(name):
    b = C.build(name)
    d, p, T = b.plan, b.p, b.case.T
    assert d == sm.plan(p, b.case.e, b.case.checks, b.case.m, T, b.case.deg, b.cons, b.boundary)
    assert all(t < d["omicron_domain_length"] for t in d["transition_degree_bounds"])
    assert pow(b.omicron, d["omicron_domain_length"], p) == 1 and pow(b.omicron, d["omicron_domain_length"] // 2, p) == p - 1
    assert pow(b.omega, d["fri_domain_length"], p) == 1 and pow(b.omega, d["fri_domain_length"] // 2, p) == p - 1
    for cycle in range(T - 1):
        point = [pow(b.omicron, cycle, p)] + b.trace[cycle] + b.trace[cycle + 1]
        assert [_constraint_at(a, point, p) for a in b.air] == [0] * len(b.air), cycle
    assert all((c, r, b.trace[c][r]) == (c, r, v) for c, r, v in b.boundary)
    pr = C.model_proof(name)
    dbg = pr["_debug"]
    tz_root = dbg["transition_zerofier_root"]
    assert dbg["boundary_exact"] and dbg["max_degree"] == d["max_degree"]
    assert [len(q) - 1 for q in dbg["transition_quotients"]] == d["transition_quotient_degree_bounds"]
    assert b.model.verify(pr, b.air, b.boundary, tz_root) is True
    bad = b.model.prove(b.trace, b.false_boundary, b.air, b.randomizer)
    assert not bad["_debug"]["boundary_exact"]
    assert b.model.verify(bad, b.air, b.false_boundary, tz_root) == "combination"


def test_degenerate_traces_have_the_stated_lengths():
    for name, tp_lens, bq_lens in (("D1-constant-register", [18, 1], [16, 1]), ("D2-zero-boundary-quotient", [18, 1], [17, 0])):
        b = C.build(name)
        assert all(row[1] == C.CONSTANT for row in b.trace) and len(b.trace) == 18
        dbg = C.model_proof(name)["_debug"]
        assert [len(q) for q in dbg["trace_polynomials"]] == tp_lens and [len(q) for q in dbg["boundary_quotients"]] == bq_lens
        assert all(dbg["transition_polynomials"]), "a transition polynomial composes to zero"


def test_refused_case_trips_the_reference_s_assertion():
    b = C.build(C.REFUSED.name)
    assert b.trace == C.build("D1-constant-register").trace and b.air[0] == C.build("D1-constant-register").air[0]
    assert sm.plan(b.p, 4, 2, 2, 10, 2, b.air, b.boundary) == b.plan
    assert mm.evaluate_symbolic(b.air[1], [[0, 1], [3, 5], [7], [1, 2], [7]], b.p) == []      # next1 - prev1 of a constant register
    with pytest.raises(AssertionError):
        b.model.prove(b.trace, b.boundary, b.air, b.randomizer)
    # the trace the same handle proves afterwards: same AIR, same plan, both transition polynomials non-zero, a deterministic proof
    t = C.build(C.REFUSED_THEN.name)
    assert (t.air, t.plan, t.case.cells) == (b.air, b.plan, b.case.cells) and len({row[1] for row in t.trace}) == len(t.trace)
    dbg = C.model_proof(C.REFUSED_THEN.name)["_debug"]
    assert all(dbg["transition_polynomials"]) and [len(q) - 1 for q in dbg["transition_quotients"]] == t.plan["transition_quotient_degree_bounds"]


def test_reuse_boundaries_change_the_root_counts_and_verify():
    counts = []
    for cells in C.REUSE_BOUNDARIES:
        b = C.build(C.REUSE_ROW, cells)
        counts.append(b.plan["boundary_counts"])
        pr = C.model_proof(C.REUSE_ROW, cells)
        assert b.model.verify(pr, b.air, b.boundary, pr["_debug"]["transition_zerofier_root"]) is True
    assert counts == [[2, 1], [0, 1], [3, 0]]


def test_the_table_reaches_every_class():
    R = {c.name: C.routing(c.name) for c in C.TABLE}
    have = lambda key: {r[key] for r in R.values()}
    assert have("m") == {1, 2, 3}
    assert have("deg") == {1, 2, 3, 4, 7}
    assert have("e") == {1, 2, 4, 8, 16, 32}
    assert have("field") == {C.FR, C.M128}
    assert sm.MAX_CONSTRAINTS in have("n_constraints")
    assert any(r["register_without_entry"] for r in R.values())
    assert any(r["register_with_several_entries"] for r in R.values())
    assert any(r["register_with_several_entries"] and r["boundary_shift_zero"] for r in R.values())
    assert any(r["unequal_transition_shifts"] for r in R.values())
    # the constraint limit, every extra constraint with a shift of its own (the m constraints of the recurrence share two)
    assert any(r["n_constraints"] == sm.MAX_CONSTRAINTS and len(set(C.build(n).plan["transition_shifts"])) >= sm.MAX_CONSTRAINTS - 2 for n, r in R.items())
    # prefix interpolation (k_prefix_weights, k_prefix_missing), in both fields; every other case goes through the subproduct tree
    assert {r["field"] for r in R.values() if r["prefix_interpolation"]} == {C.FR, C.M128}
    assert any(r["prefix_interpolation"] and r["prefix_missing"] > 2 for r in R.values())
    assert any(not r["prefix_interpolation"] for r in R.values())
    assert all(r["deg"] == 1 for r in R.values() if r["prefix_interpolation"])      # only then is the omicron domain next_pow2(rl)
    assert any(r["deg"] == 1 and not r["prefix_interpolation"] for r in R.values())                # rl a power of two: the domain doubles
    assert any(r["prefix_zerofier"] for r in R.values()) and any(not r["prefix_zerofier"] for r in R.values())
    # the coset division's host branch for rows of degree < 8, its last degree, and the transform branch
    degrees = {t for r in R.values() for t in r["transition_degrees"]}
    assert any(t < 7 for t in degrees) and 7 in degrees and 8 <= max(degrees)
    assert {r["deg"] for r in R.values() if r["small_division"]} == {1}
    # the randomized trace length on either side of the point where the omicron domain doubles
    pair = [r for r in R.values() if (r["m"], r["deg"]) == (2, 2) and r["rl"] in (31, 32)]
    assert sorted((r["rl"], C.build(n).plan["omicron_domain_length"]) for n, r in R.items() if r in pair) == [(31, 64), (32, 128)]
    # FRI: one colinearity check, a check count that is a large share of the last codeword, domains of 32 to 2048
    assert 1 in have("checks") and any(8 * r["checks"] >= r["fri_last_length"] for r in R.values())
    assert min(have("fri_domain")) == 32 and max(have("fri_domain")) == C.MAX_FRI_DOMAIN and {32, 64, 128} & have("fri_domain") == {32, 64, 128}
    assert any(r["fri_domain"] == C.build(n).plan["omicron_domain_length"] for n, r in R.items())               # expansion 1
    assert max(have("num_indices")) == 128 and {3, 4, 5, 6} <= have("fri_rounds")
    # the degenerate traces: a short trace polynomial and an empty boundary quotient
    lens = [[len(q) for q in C.model_proof(c.name)["_debug"]["boundary_quotients"]] for c in C.DEGENERATE]
    assert any(1 in l for l in lens) and any(0 in l for l in lens)


@pytest.mark.parametrize("name", sorted(C.BY_NAME))
def test_library_plan_matches_the_model(name):
    """mzk_stark_plan of the built library (host only) for every case, the reuse boundaries included"""
    mz = pytest.importorskip("myzkp_amd")
    try:
        mz.lib()
    except ImportError:
        pytest.skip("libmzk is not built")
    for cells in [None] + (list(C.REUSE_BOUNDARIES) if name == C.REUSE_ROW else []):
        b = C.build(name, cells)
        c = b.case
        assert mz.stark_plan(b.fid, c.e, c.checks, c.m, c.T, c.deg, b.cons, b.boundary) == b.plan
        assert mz.stark_proof_layout(b.fid, b.plan) == sm.proof_layout(C.LIMBS[b.fid], b.plan)
        assert mz.root_of_unity(b.fid, b.plan["omicron_domain_length"].bit_length() - 1) == b.omicron
        assert mz.root_of_unity(b.fid, b.plan["fri_domain_length"].bit_length() - 1) == b.omega
