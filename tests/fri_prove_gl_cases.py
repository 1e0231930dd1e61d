"""Inputs shared by the tests of mzk_fri_prove_gl and by tests/golden/make_golden_fri_prove_gl.py: the edge vectors that cover every
leaf length of the two Goldilocks fields, the periodic codeword that carries such a vector through every FRI round unchanged, and the
proof stream of a model proof.  No GPU, no library."""
import random
import fri_prove_model as fpm
import goldilocks_model as gm

P = gm.P
EDGE = {
    # leaf lengths 9, 13 and 17
    gm.FIELD_M64: [0, 1, (1 << 32) - 1, 1 << 32, P - 1, 0xFFFFFFFF00000000, 7, 0],
    # leaf lengths 8, 21, 30, 39, 59, 47, 21, 34, 8, 25
    gm.FIELD_M64X3: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (P - 1, P - 1, P - 1), (5, 0, 1 << 32), ((1 << 32) - 1, 0, 0), (0, 1 << 40, 0),
                     (0, 0, 0), (P - 1, 0, 0)],
}


def rand_elems(F, seed, n):
    rng = random.Random(seed)
    return [F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for _ in range(n)]


def edge_vector(F, m, seed=1):
    """m elements: the field's edge list cycled over the first half (all of it where m allows), then random elements"""
    base = EDGE[F.fid]
    k = max(m // 2, min(m, len(base)))
    return [base[i % len(base)] for i in range(k)] + rand_elems(F, 77 * m + seed, m - k)


def periodic(v, n):
    """cw[i] = v[i mod m]: every fold has a = b and returns a (out = 2^-1 (a + b) + q (a - b)), so each round's codeword is again
    periodic in v and the last one -- of length m, when the shape is chosen so -- is v itself"""
    return [v[i % len(v)] for i in range(n)]


def stream_of(F, proof):
    """the serialized proof stream behind a model proof: one object per root, then the last codeword's leaves"""
    return fpm.serialize_stream([[r] for r in proof["merkle_roots"]] + [[F.leaf(e) for e in proof["last_codeword"]]])
