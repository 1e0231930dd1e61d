"""CPU checks of tests/gemini_model.py against the reference's own tests (algebra/gemini.rs, algebra/sumcheck.rs), of the closed
forms the device computes against the literal definitions, and of the new entry points' presence in include/mzk.h and the library."""
import json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pytest
import gemini_model as gm

P = gm.P
NEW_SYMBOLS = ["mzk_gemini_split_fold", "mzk_gemini_split_fold_dev", "mzk_gemini_commit_srs", "mzk_gemini_commit_srs_dev", "mzk_gemini_open_srs",
               "mzk_gemini_open_srs_dev", "mzk_sumcheck_sum", "mzk_sumcheck_prove_srs"]


def test_tensor_product_kats():
    """gemini.rs test_tensor_product_1 / _2"""
    assert gm.tensor_product([2, 3], [4, 5, 6]) == [8, 12, 10, 15, 12, 18]
    assert gm.tensor_product(gm.tensor_product([1, 2], [1, 3]), [1, 4]) == [1, 2, 3, 6, 4, 8, 12, 24]


def test_gemini_kat_mu_and_debug_verify():
    """gemini.rs test_gemini / test_debug_verifier: mu = <coef, tensor(1, rho_i)>; the debug relation holds at beta = 1234, and
    fails for mu + 1"""
    coef = list(range(1, 9))
    rhos = [2, 3, 4]
    c = gm.tensor_product(gm.tensor_product([1, rhos[0]], [1, rhos[1]]), [1, rhos[2]])
    mu = sum(a * b for a, b in zip(coef, c)) % P
    fs = gm.split_and_fold(coef, rhos)
    assert [len(f) for f in fs] == [8, 4, 2, 1] and fs[-1] == [mu]
    assert gm.debug_verify(rhos, mu, fs, 1234)
    assert not gm.debug_verify(rhos, mu + 1, fs, 1234)


def test_split_and_fold_errors():
    with pytest.raises(gm.SplitFoldError, match="CoefsNotPowerOfTwo"):
        gm.split_and_fold([1, 2, 3], [1])
    with pytest.raises(gm.SplitFoldError, match="CoefsNotPowerOfTwo"):
        gm.split_and_fold([], [])
    with pytest.raises(gm.SplitFoldError, match="PointsLenMismatch"):
        gm.split_and_fold([1, 2, 3, 4], [1])


def test_first_round_kat():
    """sumcheck.rs test_first_round: h = 41 and h = sumcheck_fold(g_0, 0)"""
    g = gm.PIPELINE_G
    h = gm.sum_over_boolean_hypercube(g)
    assert h == 41
    g0 = gm.build_gj_from_prefix(g, [])
    assert gm.sumcheck_fold(g0, 0, 3) == h
    coefs = gm.get_coefs_in_order(g)
    assert coefs == [1, 2, 3, 0, 0, 0, 4, 5]
    assert gm.hypercube_sum_closed(coefs) == 41


def test_bit_combinations():
    """sumcheck.rs test_bitcombinations (from 0): 8 combinations of 3 bits, bit i of the counter at entry i"""
    vs = list(gm.bit_combinations(3))
    assert len(vs) == 8 and vs[1] == [1, 0, 0] and vs[6] == [0, 1, 1]


@pytest.mark.parametrize("el", [1, 2, 3, 4, 5, 6, 8])
def test_closed_forms_match_the_literal_definitions(el):
    """A_j / B_j from the fold level equal build_gj_from_prefix's polynomial, and the closed-form h the hypercube sum"""
    rnd = random.Random(1000 + el)
    coefs = [rnd.randrange(P) if rnd.random() < 0.8 else 0 for _ in range(1 << el)]
    g = gm.mpoly_from_coefs(coefs)
    # pad the keys to el variables so that num_vars is el even when the top variable's coefficients are all zero
    g[tuple([1] * el)] = g.get(tuple([1] * el), 0)
    assert gm.get_coefs_in_order(g) == [c % P for c in coefs]
    assert gm.sum_over_boolean_hypercube(g) == gm.hypercube_sum_closed(coefs)
    rs = [rnd.randrange(P) for _ in range(el)]
    fs = gm.split_and_fold(coefs, rs)
    for j in range(el):
        gj = gm.build_gj_from_prefix(g, rs[:j])
        assert gm.gj_coefficients(gj, j) == gm.round_message_closed(fs[j], el, j), j


def test_model_prover_passes_the_value_level_verifier():
    coefs = gm.get_coefs_in_order(gm.PIPELINE_G)
    h, gs, rs, beta = gm.sumcheck_rounds(coefs)
    assert beta == rs[-1]                        # sampled from the unchanged stream
    fs = gm.split_and_fold(coefs, rs)
    us = [beta, gm.neg(beta), beta * beta % P]
    ys = [tuple(gm.poly_eval(f, u) for u in us) for f in fs[:-1]]
    assert gm.verify_sumcheck_values(h, gs, rs, beta, ys)
    assert not gm.verify_sumcheck_values(h + 1, gs, rs, beta, ys)
    bad = list(ys)
    bad[1] = (bad[1][0], bad[1][1], (bad[1][2] + 1) % P)
    assert not gm.verify_sumcheck_values(h, gs, rs, beta, bad)
    # the callback form replays the same transcript
    cb = gm.ModelChallenge(3, h)
    assert [cb(j, gs[j]) for j in range(3)] == rs and cb(3, None) == beta


def test_quotient3_is_the_exact_division():
    rnd = random.Random(7)
    f = [rnd.randrange(P) for _ in range(16)]
    us = [5, P - 5, 25]
    q = gm.quotient3(f, us)
    # f = q Z + I with deg I < 3: f - q Z vanishes at the three points
    z = [1]
    for u in us:
        z = [((z[i - 1] if i else 0) - u * (z[i] if i < len(z) else 0)) % P for i in range(len(z) + 1)]
    qz = [0] * (len(q) + len(z) - 1)
    for i, a in enumerate(q):
        for k, b in enumerate(z):
            qz[i + k] = (qz[i + k] + a * b) % P
    r = [(f[i] - (qz[i] if i < len(qz) else 0)) % P for i in range(len(f))]
    assert all(c == 0 for c in r[3:])
    assert gm.quotient3([1, 2], us) == []


def test_golden_vectors_follow_the_model():
    d = json.load(open(os.path.join(HERE, "golden", "gemini_vectors.json")))
    g = d["gemini"]
    assert g["levels"] == gm.split_and_fold(g["coef"], g["rhos"]) and g["levels"][-1] == [g["mu"]] == [382]
    s = d["sumcheck"]
    h, gs, rs, beta = gm.sumcheck_rounds(s["coefs"])
    assert (h, [list(x) for x in gs], rs, beta) == (s["h"], s["gs"], s["rs"], s["beta"])
    assert gm.verify_sumcheck_values(s["h"], s["gs"], s["rs"], s["beta"], s["ys"])


def test_new_symbols_declared_and_exported():
    import myzkp_amd
    for s in NEW_SYMBOLS:
        assert s in myzkp_amd.DECLARED_SYMBOLS, s
    exported = myzkp_amd.exported_symbols()
    assert [s for s in NEW_SYMBOLS if s not in exported] == []
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "mzk.h")).read()
    assert "typedef int (*mzk_sumcheck_challenge_fn)(void* user, int round, const uint64_t g[8], uint64_t r_out[4]);" in hdr
