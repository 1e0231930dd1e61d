"""tests/rescue_cases.py checked on its own: the table's model against mpoly_model.RescuePrime (the model mzk_stark_prove's tests take
their traces from) and against the two known answers of the reference's test_rescue_prime; the exponents and the zero cases are what
their names say.  CPU only."""
import mpoly_model as mm
import rescue_cases as rc


def as_par(c):
    return {"m": c["m"], "n": c["n"], "alpha": c["alpha"], "alphainv": c["alphainv"], "mds": c["mds"], "mdsinv": [[0] * c["m"] for _ in range(c["m"])], "round_constants": c["rc"]}


def test_the_table_model_equals_mpoly_model_on_every_m128_case():
    seen = 0
    for c in rc.CASES:
        if c["field"] != "m128":
            continue
        ref = mm.RescuePrime(as_par(c))
        for x in c["inputs"]:
            assert rc.model_trace(c, x) == ref.trace(x), c["name"]
            seen += 1
    assert seen > 100 and mm.M128_P == rc.M128_P


def test_known_answers_of_the_reference():
    g = rc.golden()
    c = rc.BY_NAME["reference"]
    assert len(g["kats"]) == 2 and (c["m"], c["n"], c["alpha"]) == (2, 27, 3) and c["alphainv"] == 0x87aaaaaaaaaaaaaaaaaaaaaaaaaaaaab
    for k in g["kats"]:
        assert int(k["input"]) in c["inputs"]
        assert rc.model_hash(c, int(k["input"])) == int(k["hash"])
        t = rc.model_trace(c, int(k["input"]))
        assert len(t) == 28 and t[0] == [int(k["input"]), 0] and t[-1][0] == int(k["hash"])


def test_chain_links_feed_each_other():
    c = rc.BY_NAME["reference-chain"]
    links = rc.model_chain(c, rc.CHAIN_INPUT, rc.CHAIN_LINKS)
    assert len(links) == 10 and links[0][0][0] == [rc.CHAIN_INPUT, 0]
    for (t0, o0), (t1, _) in zip(links, links[1:]):
        assert t1[0] == [o0, 0] and t0[-1][0] == o0


def test_the_table_covers_what_it_says():
    names = set(rc.BY_NAME)
    assert {"m128-m%d-n%d" % (m, n) for m in (1, 2, 3, 4) for n in (1, 2, 27, 64)} <= names
    assert {"fr-m%d-n%d" % (m, n) for m in (1, 2, 4) for n in (1, 3)} <= names
    assert {(c["alpha"], c["alphainv"]) for c in rc.CASES if c["name"].startswith("m128-exp-")} == {(a, i) for a in rc.ALPHAS for i in rc.ALPHAINVS_M128}
    assert {c["alphainv"] for c in rc.CASES if c["name"].startswith("fr-exp-")} == set(rc.ALPHAINVS_FR)
    for f, a in (("m128", 3), ("fr", 5)):
        p = rc.PRIME[f]
        assert pow(pow(12345, a, p), rc.inv_exp(a, f), p) == 12345
    for c in rc.CASES:
        p = rc.PRIME[c["field"]]
        assert 1 <= c["m"] <= 4 and 1 <= c["n"] <= 64 and 0 <= c["alpha"] < 1 << 64 and 0 <= c["alphainv"] < 1 << 256, c["name"]
        assert all(0 <= v < p for row in c["mds"] for v in row) and all(0 <= v < p for v in c["rc"]) and all(0 <= v < p for v in c["inputs"]), c["name"]


def test_the_zero_cases_pass_through_zero():
    p = rc.M128_P
    c = rc.BY_NAME["zero-all"]
    assert all(v == 0 for row in rc.model_trace(c, 0) for v in row)
    c = rc.BY_NAME["zero-backward"]
    x = c["inputs"][0]
    assert (c["mds"][0][0] * pow(x, c["alpha"], p) + c["rc"][0]) % p == 0 and rc.model_hash(c, x) == c["rc"][1]
    c = rc.BY_NAME["zero-one-element"]
    x = c["inputs"][0]
    half = [(c["mds"][i][0] * pow(x, 3, p) + c["rc"][i]) % p for i in range(2)]
    assert half[0] != 0 and half[1] == 0


def test_x_to_the_zero_is_one_also_for_zero():
    c = rc.BY_NAME["m128-exp-a0-i0"]
    assert (c["alpha"], c["alphainv"]) == (0, 0)
    m, p = c["m"], rc.M128_P
    t = rc.model_trace(c, 0)
    want = [(sum(c["mds"][i]) + c["rc"][m + i]) % p for i in range(m)]        # after round 0: mds * [1, 1] + the second constants
    assert t[1] == want
