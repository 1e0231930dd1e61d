"""Inputs shared by the CPU and GPU tests of mzk_fri_prove over M128 and Fr: the edge values that cover every leaf length of a field of
nw 32-bit words, and the periodic codeword that carries a vector of them through every FRI round unchanged.  No GPU, no library."""
import random


def edge_values(p, nw):
    """0, 1, p - 1, and 2^(32 j) - 1 and 2^(32 j) for every j below nw: every trimmed word count 0 .. nw, on both sides of each word
    boundary (all below p: p has more than 32 (nw - 1) bits)"""
    assert p >> (32 * (nw - 1)) > 1
    out = [0, 1, p - 1]                                   # j = 0 gives 0 and 1 again
    for j in range(1, nw):
        out += [(1 << (32 * j)) - 1, 1 << (32 * j)]
    return out


def edge_vector(p, nw, m, seed=1):
    """m elements: the edge values cycled over the first half (all of them where m allows, as many as fit otherwise), so that the
    revealed siblings meet them too, then random elements"""
    base = edge_values(p, nw)
    k = max(m // 2, min(m, len(base)))
    rng = random.Random(77 * m + seed)
    return [base[i % len(base)] for i in range(k)] + [rng.randrange(p) for _ in range(m - k)]


def periodic(v, n):
    """cw[i] = v[i mod m]: every fold has a = b and returns a (out = 2^-1 (a + b) + q (a - b)), so each round's codeword is again
    periodic in v and the last one -- of length m, when the shape is chosen so -- is v itself"""
    return [v[i % len(v)] for i in range(n)]


def words(v, nw):
    """the magnitude |v| as nw little-endian 32-bit words"""
    return [(abs(v) >> (32 * i)) & 0xFFFFFFFF for i in range(nw)]
