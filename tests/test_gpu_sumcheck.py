"""The sum-check prover on the GPU (mzk_sumcheck_prove_srs, mzk_sumcheck_sum): prove_sumcheck (algebra/sumcheck.rs:128-167) for a
multilinear g with the transcript in a Python callback -- round messages, challenges, beta and every Gemini point bit-exact against
the model (tests/gemini_model.py), the golden vectors and the trapdoor identities; the value-level verifier passes."""
import json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import pytest
import orc
import gemini_model as gm

pytestmark = pytest.mark.gpu
P = gm.P


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as mz
    mz.init(0)
    return mz


def arr(v):
    return orc.to_limbs(list(v), 4)


def rand_coefs(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(P) for _ in range(n)]


@pytest.mark.parametrize("el", [0, 1, 3, 9, 12, 18])
def test_hypercube_sum(mz, el):
    coefs = rand_coefs(500 + el, 1 << el)
    assert mz.sumcheck_sum(arr(coefs)) == gm.hypercube_sum_closed(coefs)


def test_reference_polynomial_sum_is_41(mz):
    assert mz.sumcheck_sum(arr(gm.get_coefs_in_order(gm.PIPELINE_G))) == 41


def test_pipeline_polynomial_matches_golden(mz):
    d = json.load(open(os.path.join(HERE, "golden", "gemini_vectors.json")))
    g = d["sumcheck"]
    srs = mz.Srs(orc.kzg_setup_ref(d["alpha"], d["max_d"]))
    out = srs.sumcheck_prove(arr(g["coefs"]), gm.ModelChallenge(3, g["h"]))
    assert [list(x) for x in out["gs"]] == g["gs"] and out["rs"] == g["rs"] and out["beta"] == g["beta"] == g["rs"][-1]
    assert [list(p) for p in out["commits"]] == g["commits"]
    assert [list(y) for y in out["ys"]] == g["ys"]
    assert [list(p) for p in out["ws"]] == g["ws"] and [list(p) for p in out["deg"]] == g["deg"]
    assert gm.verify_sumcheck_values(g["h"], out["gs"], out["rs"], out["beta"], out["ys"])
    srs.close()


@pytest.mark.parametrize("el", [10, 16])
def test_prove_matches_model(mz, el):
    n = 1 << el
    alpha, max_d = 0x2468 + el, n + 1
    srs = mz.Srs(mz.kzg_setup_g1(alpha, max_d))
    coefs = rand_coefs(600 + el, n)
    h, gs, rs, beta = gm.sumcheck_rounds(coefs)
    seen = []

    def challenge(rnd, g):
        seen.append(rnd)
        return cb(rnd, g)
    cb = gm.ModelChallenge(el, h)
    out = srs.sumcheck_prove(arr(coefs), challenge)
    assert seen == list(range(el + 1))
    assert out["gs"] == gs and out["rs"] == rs and out["beta"] == beta
    assert gm.verify_sumcheck_values(h, out["gs"], out["rs"], out["beta"], out["ys"])
    levels = [arr(f) for f in gm.split_and_fold(coefs, rs)]
    gm.trapdoor_check(levels, beta, alpha, max_d, out["commits"], out["ys"], out["ws"], out["deg"])
    # the one call equals the composed entry points on the same levels
    assert out["commits"] == srs.gemini_commit(levels)
    assert (out["ys"], out["ws"], out["deg"]) == srs.gemini_open(levels, beta)
    srs.close()


def test_round_messages_at_2_20_match_a_model_fold(mz):
    el = 20
    n = 1 << el
    srs = mz.Srs(mz.kzg_setup_g1(0x31337, n + 1))
    coefs = rand_coefs(700, n)
    rnd = random.Random(701)
    rs = [rnd.randrange(P) for _ in range(el)]
    got = []

    def challenge(j, g):
        if g is not None:
            got.append(g)
        return rs[j] if j < el else 1234
    out = srs.sumcheck_prove(arr(coefs), challenge)
    f = [c % P for c in coefs]
    for j in range(el):
        assert got[j] == gm.round_message_closed(f, el, j), j
        f = [(f[2 * k] + rs[j] * f[2 * k + 1]) % P for k in range(len(f) // 2)]
    assert out["rs"] == rs and out["beta"] == 1234
    mu = f[0]
    assert gm.verify_sumcheck_values(gm.hypercube_sum_closed(coefs), out["gs"], rs, 1234, out["ys"])
    assert (out["gs"][-1][0] + out["gs"][-1][1] * rs[-1]) % P == mu
    srs.close()


def test_error_paths(mz):
    from myzkp_amd import MzkError
    srs = mz.Srs(mz.kzg_setup_g1(0x55, 8))
    coefs = arr(gm.get_coefs_in_order(gm.PIPELINE_G))
    with pytest.raises(MzkError) as e:                      # el = 0: build_gj_from_prefix's assert
        srs.sumcheck_prove(arr([7]), lambda j, g: 1)
    assert e.value.code == -5
    with pytest.raises(MzkError) as e:
        srs.sumcheck_prove(arr(range(6)), lambda j, g: 1)
    assert e.value.code == -2
    with pytest.raises(MzkError) as e:                      # 2^3 coefficients need 9 powers
        mz.Srs(mz.kzg_setup_g1(0x55, 7)).sumcheck_prove(coefs, lambda j, g: 1)
    assert e.value.code == -5

    class Boom(Exception):
        pass

    def raising(j, g):
        if j == 1:
            raise Boom("transcript failed")
        return 5
    with pytest.raises(Boom):
        srs.sumcheck_prove(coefs, raising)
    with pytest.raises(MzkError) as e:                      # r not canonical
        srs.sumcheck_prove(coefs, lambda j, g: P)
    assert e.value.code == -6
    with pytest.raises(MzkError) as e:                      # beta not canonical
        srs.sumcheck_prove(coefs, lambda j, g: P + 3 if g is None else 5)
    assert e.value.code == -6
    # nothing left enqueued: the next call is right
    h, gs, rs, beta = gm.sumcheck_rounds(gm.get_coefs_in_order(gm.PIPELINE_G))
    out = srs.sumcheck_prove(coefs, gm.ModelChallenge(3, h))
    assert out["gs"] == gs and out["rs"] == rs and out["beta"] == beta
    assert gm.verify_sumcheck_values(h, out["gs"], out["rs"], out["beta"], out["ys"])
    srs.close()
