"""Writes tests/golden/mpoly_vectors.json: small inputs and expected coefficients of evaluate_symbolic (algebra/mpolynomials.rs:125-141)
and of the weighted combination (zkstark/fast_stark.rs:301-326) over Fr and M128, computed by the pure-Python model tests/mpoly_model.py
(term by term, schoolbook products).  Deterministic: python tests/golden/make_golden_mpoly.py"""
import json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import mpoly_model as mm

FIELDS = {"fr": (0, mm.FR_P), "m128": (1, mm.M128_P)}


def S(v):
    return [str(x) for x in v]


def compose_case(name, fname, constraints, point):
    fid, p = FIELDS[fname]
    return {"name": name, "field": fid, "constraints": [[[str(c), list(k)] for c, k in terms] for terms in constraints], "point": [S(q) for q in point],
            "expected": [S(mm.compose_terms(terms, point, p)) for terms in constraints]}


def lincomb_case(name, fname, polys, weights, shifts):
    fid, p = FIELDS[fname]
    want = mm.lincomb_reference(polys, weights, shifts, p)
    assert want == mm.lincomb(polys, weights, shifts, p)
    return {"name": name, "field": fid, "polys": [S(q) for q in polys], "weights": S(weights), "shifts": list(shifts), "expected": S(want)}


def main():
    rnd = random.Random(20260)
    compose, lin = [], []
    for fname, (fid, p) in FIELDS.items():
        rp = lambda n: [rnd.randrange(p) for _ in range(n)]
        # the reference's own known answers (mpolynomials.rs:614-688)
        compose.append(compose_case("2x+3y at (t+1, t^2)", fname, [[(2, (1, 0)), (3, (0, 1))]], [[1, 1], [0, 0, 1]]))
        compose.append(compose_case("constant 5", fname, [[(5, (0, 0))]], [[1, 1], [0, 0, 1]]))
        # random sparse constraints over three variables
        cons = [[(rnd.randrange(p), tuple(rnd.randrange(4) for _ in range(3))) for _ in range(12)] for _ in range(3)]
        compose.append(compose_case("random sparse, 3 variables", fname, cons, [rp(5), rp(7), rp(3)]))
        # a lifted univariate times monomials: the Horner shape, with gaps in the exponents
        cons = [[(rnd.randrange(p), (e, a, b)) for (a, b) in ((0, 0), (2, 1), (0, 3)) for e in (0, 1, 2, 3, 5, 9, 20)]]
        compose.append(compose_case("lifted univariate with gaps", fname, cons, [rp(4), rp(6), rp(2)]))
        # cancellations
        q = rp(9)
        compose.append(compose_case("x1 - x2 at (p, p)", fname, [[(1, (1, 0)), (p - 1, (0, 1))]], [q, q]))
        compose.append(compose_case("leading terms cancel", fname, [[(1, (1, 0)), (p - 1, (0, 1))]], [q, q[:5] + [(q[5] + 1) % p] + q[6:]]))
        lin_polys = [rp(9), rp(12), rp(5)]
        lin.append(lincomb_case("plain and shifted", fname, [lin_polys[0], lin_polys[0], lin_polys[1], lin_polys[1], lin_polys[2]], rp(5), [0, 7, 0, 4, 0]))
        lin.append(lincomb_case("cancelling pair", fname, [lin_polys[0], lin_polys[0]], [3, p - 3], [2, 2]))
    out = os.path.join(HERE, "mpoly_vectors.json")
    with open(out, "w") as f:
        json.dump({"compose": compose, "lincomb": lin}, f, indent=0)
        f.write("\n")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
