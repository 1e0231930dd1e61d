"""The case table of the Rescue-Prime tests (zkstark/rescueprime.rs; myzkp_amd/csrc/mzk_rescue*.h, mzk_rescue.hip): parameter sets with
seeded constants, inputs, and what each case is there for.  One table for tests/test_rescue_cases.py (the table against
mpoly_model.RescuePrime and the reference's known answers), tests/test_hostcheck_rescue.py (the per-lane code built for the host) and
tests/test_gpu_rescue.py (the kernel).  model_trace is the hash in Python integers over any prime: the model of the Fr cases, and --
checked against mpoly_model.RescuePrime in test_rescue_cases.py -- of the M128 ones."""
import json, os, random

HERE = os.path.dirname(os.path.abspath(__file__))
M128_P = 270497897142230380135924736767050121217                     # 1 + 407 * 2^119 (fri.rs:408)
FR_P = 21888242871839275222246405745257275088548364400416034343698204186575808495617
PRIME = {"m128": M128_P, "fr": FR_P}
FIELD_ID = {"fr": 0, "m128": 1}
LIMBS = {"m128": 2, "fr": 4}
CHAIN_INPUT, CHAIN_LINKS = 123456789, 10                               # test_fast_stark's chain


def golden():
    with open(os.path.join(HERE, "golden", "rescue_prime_m128.json")) as f:
        return json.load(f)


def model_trace(c, x):
    """rescueprime.rs:521-591: the state before round 0 and after every round, n + 1 rows of m"""
    p, m, mds, rc = PRIME[c["field"]], c["m"], c["mds"], c["rc"]
    state = [x % p] + [0] * (m - 1)
    rows = [list(state)]
    for r in range(c["n"]):
        for half, e in ((0, c["alpha"]), (1, c["alphainv"])):
            state = [pow(s, e, p) for s in state]
            state = [(sum(mds[i][j] * state[j] for j in range(m)) + rc[2 * r * m + half * m + i]) % p for i in range(m)]
        rows.append(list(state))
    return rows


def model_hash(c, x):
    return model_trace(c, x)[-1][0]


def model_chain(c, x, links):
    """[(trace, output)] of every link; link l + 1 absorbs the output of link l"""
    out = []
    for _ in range(links):
        t = model_trace(c, x)
        x = t[-1][0]
        out.append((t, x))
    return out


def inv_exp(a, field):
    return pow(a, -1, PRIME[field] - 1)


def case(name, field, m, n, alpha, alphainv, mds, rc, inputs, links, why):
    assert len(mds) == m and all(len(r) == m for r in mds) and len(rc) == 2 * n * m
    return {"name": name, "field": field, "m": m, "n": n, "alpha": alpha, "alphainv": alphainv, "mds": mds, "rc": rc, "inputs": inputs, "links": links, "why": why}


def seeded(name, field, m, n, alpha, alphainv, seed, n_inputs=3, links=1, why=""):
    rng = random.Random(seed)
    p = PRIME[field]
    mds = [[rng.randrange(p) for _ in range(m)] for _ in range(m)]
    rc = [rng.randrange(p) for _ in range(2 * n * m)]
    return case(name, field, m, n, alpha, alphainv, mds, rc, [rng.randrange(p) for _ in range(n_inputs)], links, why)


def reference_case(inputs, links, name, why):
    g = golden()
    return case(name, "m128", g["m"], g["n"], int(g["alpha"]), int(g["alphainv"]), [[int(v) for v in row] for row in g["mds"]], [int(v) for v in g["round_constants"]],
                inputs, links, why)


ALPHAS = (0, 1, 2, 3, 5, 7)
ALPHAINVS_M128 = (0, 1, 2, 1 << 127, (1 << 128) - 1, M128_P - 2, inv_exp(3, "m128"))
ALPHAINVS_FR = (FR_P - 2, 1 << 253, inv_exp(5, "fr"))


def build():
    g = golden()
    p = M128_P
    cases = [
        reference_case([int(k["input"]) for k in g["kats"]] + [0, 1, p - 1, p - 2], 1, "reference", "the reference's parameters: its two known answers and the edge inputs"),
        reference_case([CHAIN_INPUT], CHAIN_LINKS, "reference-chain", "the ten links of test_fast_stark"),
    ]
    for m in (1, 2, 3, 4):
        for n in (1, 2, 27, 64):
            cases.append(seeded("m128-m%d-n%d" % (m, n), "m128", m, n, 3, inv_exp(3, "m128"), 1000 + 100 * m + n, links=2 if n <= 2 else 1,
                                why="every (m, n_rounds) cell: the state loops at every width, the first, a middle and the last admitted round count"))
    for m in (1, 2, 4):
        for n in (1, 3):
            cases.append(seeded("fr-m%d-n%d" % (m, n), "fr", m, n, 5, inv_exp(5, "fr"), 2000 + 100 * m + n, links=2, why="the nine-limb field at every state form"))
    for a in ALPHAS:
        for k, ai in enumerate(ALPHAINVS_M128):
            cases.append(seeded("m128-exp-a%d-i%d" % (a, k), "m128", 2, 2, a, ai, 3000 + 10 * a + k, n_inputs=2,
                                why="exponent shapes: 0 (x^0 = 1, 0^0 included), 1, a lone squaring, each odd slot first, a lone top bit, all ones, p - 2, a true inverse"))
    for k, ai in enumerate(ALPHAINVS_FR):
        cases.append(seeded("fr-exp-i%d" % k, "fr", 2, 2, 5, ai, 3500 + k, n_inputs=2, why="the longest exponents of the 254-bit field"))
    # states that pass through zero
    cases.append(case("zero-all", "m128", 1, 2, 3, inv_exp(3, "m128"), [[0]], [0, 0, 0, 0], [0], 2, "all constants zero, input 0: every product has a zero operand"))
    x, mds0 = 0x1234567, 0x89abcdef
    cases.append(case("zero-backward", "m128", 1, 1, 3, inv_exp(3, "m128"), [[mds0]], [(-mds0 * pow(x, 3, p)) % p, 5], [x, 0, 1], 1,
                      "the first round constant is -mds * x^alpha: the backward S-box of input x receives 0"))
    c = seeded("zero-one-element", "m128", 2, 2, 3, inv_exp(3, "m128"), 3900, n_inputs=1, links=2, why="a zero in one element of the state only, behind the first half-round")
    c["rc"][1] = (-c["mds"][1][0] * pow(c["inputs"][0], 3, p)) % p
    cases.append(c)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


CASES = build()
BY_NAME = {c["name"]: c for c in CASES}


def dump(cases):
    """the table as text for tests/hostcheck/rescue_shim.cpp: one case per block, every number in hex"""
    out = ["%d" % len(cases)]
    for c in cases:
        out.append("%s %d %d %d %x %x %d %d" % (c["name"], FIELD_ID[c["field"]], c["m"], c["n"], c["alpha"], c["alphainv"], len(c["inputs"]), c["links"]))
        out.append(" ".join("%x" % v for row in c["mds"] for v in row))
        out.append(" ".join("%x" % v for v in c["rc"]))
        out.append(" ".join("%x" % v for v in c["inputs"]))
    return "\n".join(out) + "\n"
