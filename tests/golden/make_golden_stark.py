"""Writes tests/golden/stark_vectors.json from tests/stark_model.py: FastStark proofs of the Rescue-Prime hash chain of the reference's
test_fast_stark (expansion 4, 2 colinearity checks), with the random rows of the trace and the randomizer polynomial -- which the
reference draws from the OS -- drawn from a seeded generator and written into the file.  One proof in full, the others as the
SHA3-256 of stark_model.proof_digest's rendering plus the roots.

    python tests/golden/make_golden_stark.py
"""
import json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mpoly_model as mm
import stark_model as sm

LINKS, SEED = 2, 20261016


def setup():
    with open(os.path.join(HERE, "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    p = mm.M128_P
    st = sm.FastStark(p, mm.M128_GEN, mm.m128_root(9), mm.m128_root(7), 4, 2, rp.m, rp.n + 1, 2)
    return rp, st, rp.transition_constraints(st.omicron)


def render(v):
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).hex()
    if isinstance(v, dict):
        return {k: render(x) for k, x in v.items() if k != "_debug"}
    if isinstance(v, (list, tuple)):
        return [render(x) for x in v]
    return str(int(v))


def cases():
    rp, st, air = setup()
    p = st.p
    rnd = random.Random(SEED)
    out, res = 123456789, []
    for link in range(LINKS):
        tr = rp.trace(out)
        inp, out = out, tr[-1][0]
        for label, claimed in (("true", out), ("false", (out + 1) % p)):
            rows = [[rnd.randrange(p) for _ in range(rp.m)] for _ in range(st.nr)]
            randomizer = [rnd.randrange(p) for _ in range(128)]
            boundary = [(0, 1, 0), (rp.n, 0, claimed)]
            pr = st.prove([list(r) for r in tr] + rows, boundary, air, randomizer)
            case = {"name": "link %d, %s output" % (link, label), "input": str(inp), "claimed_output": str(claimed), "random_rows": render(rows),
                    "randomizer": render(randomizer), "bqc_roots": render(pr["bqc_roots"]), "rdc_root": render(pr["rdc_root"]),
                    "indices": pr["_debug"]["indices"], "boundary_exact": pr["_debug"]["boundary_exact"], "digest": sm.proof_digest(pr)}
            if link == 0 and label == "true":
                case["proof"] = render(pr)
            res.append(case)
    return {"expansion_factor": 4, "num_colinearity_checks": 2, "seed": SEED, "transition_zerofier_root": render(st.preprocess()[2]), "cases": res}


if __name__ == "__main__":
    path = os.path.join(HERE, "stark_vectors.json")
    with open(path, "w") as f:
        json.dump(cases(), f, indent=0, separators=(",", ":"))
        f.write("\n")
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
