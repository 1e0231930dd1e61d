"""Writes tests/golden/fri_prove_gl_vectors.json: FRI::prove over the Goldilocks field and its cubic extension as
tests/goldilocks_model.py computes it (Python integers, hashlib).

    python tests/golden/make_golden_fri_prove_gl.py

Cases: the reference's test_fri_efield (fri.rs:546-594: M64X3, coefficients 0 .. 63, n = 1024, offset 7, expansion factor 16, 17
colinearity tests), 64 random M64 elements, and the M64X3 edge vector of tests/fri_prove_gl_cases.py through a periodic codeword
(every leaf length 8 .. 59 in every tree).  Recorded: roots, top-level indices, SHA-256 of the serialized proof stream."""
import hashlib, json, os, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import goldilocks_model as gm
import fri_prove_gl_cases as cases


def case(name, F, codeword, omega, offset, expansion, tests):
    proof = gm.prove(F, codeword, omega, offset, expansion, tests)
    stream = cases.stream_of(F, proof)
    return {"name": name, "field": F.fid, "n": len(codeword), "omega": str(F.words(omega)[0]), "offset": str(F.words(offset)[0]),
            "expansion_factor": expansion, "num_colinearity_tests": tests, "codeword": [[str(w) for w in F.words(e)] for e in codeword],
            "top_level_indices": proof["top_level_indices"], "merkle_roots": [r.hex() for r in proof["merkle_roots"]],
            "stream_sha256": hashlib.sha256(stream).hexdigest(), "stream_len": len(stream)}


def main():
    out = []
    F = gm.M64X3
    omega = gm.root_of_unity(F, 10)
    coef = [F.from_int(i) for i in range(64)]
    out.append(case("test_fri_efield", F, gm.ntt(F, omega, coef + [F.zero] * (1024 - 64)), omega, F.from_int(7), 16, 17))
    F = gm.M64
    out.append(case("m64_random_64", F, cases.rand_elems(F, 20261, 64), gm.root_of_unity(F, 6), F.from_int(7), 4, 4))
    F = gm.M64X3
    out.append(case("m64x3_edge_64", F, cases.periodic(cases.edge_vector(F, 16), 64), gm.root_of_unity(F, 6), F.from_int(7), 2, 3))
    with open(os.path.join(HERE, "fri_prove_gl_vectors.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
