"""Writes tests/golden/fri_prove_vectors.json: FRI::prove (zkstark/fri.rs:99-143) with the reference's real proof stream,
computed by tests/fri_prove_model.py (Python integers, hashlib SHAKE256 / SHA3-256 / Blake2b-256).

    python tests/golden/make_golden_fri_prove.py

Cases: the reference's test_fri_field (fri.rs:495-545: M128, degree 63, expansion factor 4, 17 colinearity tests, offset the M128
generator, omega = get_nth_root_of_m128), one Fr case, and one M128 case whose initial codeword holds elements the reference left
negative (Sign::Minus leaves in round 0).  Proof fields are hex strings; values with Sign::Minus are negative integers."""
import hashlib, json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import fri_prove_model as fm

GEN = 85408008396924667383611388730472331217              # fri.rs:506-508, order 2^119
FR_OMEGA28 = 19103219067921713944291392827692070036145651957329286315305642004821462161904     # order 2^28


def m128_root(lg):
    return pow(GEN, 1 << (119 - lg), fm.P_M128)


def fr_root(lg):
    return pow(FR_OMEGA28, 1 << (28 - lg), fm.P_FR)


def case(name, field, p, codeword, omega, offset, expansion, tests):
    proof, stream = fm.prove(p, codeword, omega, offset, expansion, tests)
    layers = [{k: {"values": [str(v) for v in L[k][0]], "paths": [[e.hex() for e in path] for path in L[k][1]]} for k in "abc"}
              for L in proof["revealed_layers"]]
    return {"name": name, "field": field, "n": len(codeword), "omega": str(omega), "offset": str(offset), "expansion_factor": expansion,
            "num_colinearity_tests": tests, "codeword": [str(v) for v in codeword],
            "top_level_indices": proof["top_level_indices"], "merkle_roots": [r.hex() for r in proof["merkle_roots"]],
            "last_codeword": [str(v) for v in proof["last_codeword"]], "revealed_layers": layers,
            "stream_sha256": hashlib.sha256(stream).hexdigest(), "stream_len": len(stream)}


def main():
    P = fm.P_M128
    out = []
    n = 256                                                                       # test_fri_field: degree 63, expansion 4
    om = m128_root(8)
    coef = list(range(64))
    cw = [sum(c * pow(om, i * k, P) for k, c in enumerate(coef)) % P for i in range(n)]
    out.append(case("test_fri_field_m128", 1, P, cw, om, GEN, 4, 17))
    rng = random.Random(20260)
    n = 64
    cw = [rng.randrange(fm.P_FR) for _ in range(n)]
    out.append(case("fr_random_64", 0, fm.P_FR, cw, fr_root(6), 7, 4, 4))
    n = 64
    cw = [rng.randrange(P) for _ in range(n)]
    cw = [-v if i % 3 == 1 else v for i, v in enumerate(cw)] + []              # magnitudes < p with Sign::Minus
    cw[5] = 0
    out.append(case("m128_signed_64", 1, P, cw, m128_root(6), GEN, 2, 3))
    with open(os.path.join(HERE, "fri_prove_vectors.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
