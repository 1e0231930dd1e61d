"""The shapes tests/test_gpu_das.py runs, and its seeded inputs.  tests/test_das_cases.py checks on the CPU that the tables reach every
path of the kernels.  No shape exceeds 255 x 255 x 3 squares or 17 x 17 x 65."""
import numpy as np

SQUARE_SIDES = list(range(2, 34)) + [63, 64, 65, 127, 128, 129, 254, 255]
RECTS = [(2, 255), (255, 2), (3, 5), (5, 3), (17, 64), (64, 17)]
SQUARE_COUNTS = (1, 2, 3)
MANY_SQUARES = 65             # at sides <= 17: workgroups then straddle squares
MANY_MAX_SIDE = 17
OPEN_ALL_SIDES = list(range(2, 18)) + [31, 32, 33]      # every position, both directions
OPEN_SAMPLED = (255, 255, 3, 512)                       # rows, cols, squares, seeded positions
TIE_SHAPES = [(5, 3, 1), (16, 16, 1), (33, 31, 2)]      # against mzk_merkle_commit_bytes
PIPELINE = [(8, 16, 64), (127, 255, 127 * 127)]         # chunk side, codeword side, message_len: rs2d encode -> grid build


def commit_cases():
    """(rows, cols, squares) of every commit test"""
    out = []
    for n in SQUARE_SIDES:
        out += [(n, n, q) for q in SQUARE_COUNTS]
        if n <= MANY_MAX_SIDE:
            out.append((n, n, MANY_SQUARES))
    for r, c in RECTS:
        out += [(r, c, q) for q in SQUARE_COUNTS]
        if max(r, c) <= MANY_MAX_SIDE:
            out.append((r, c, MANY_SQUARES))
    return out


def max_count(rows, cols):
    return MANY_SQUARES if max(rows, cols) <= MANY_MAX_SIDE else max(SQUARE_COUNTS)


def squares(rows, cols, count, seed):
    """count x rows x cols seeded bytes: the first `count` of the max_count(rows, cols) squares of this shape and seed, so that a model
    computed once per shape serves every count.  No square equals its transpose: a row / column mix-up must not pass."""
    assert 1 <= count <= max_count(rows, cols)
    rng = np.random.default_rng([seed, rows, cols])
    m = rng.integers(0, 256, size=(max_count(rows, cols), rows, cols), dtype=np.uint8)
    if rows == cols:
        for q in range(len(m)):
            if m[q, 0, 1] == m[q, 1, 0]:
                m[q, 1, 0] ^= 0x5A
    return m[:count].copy()


def positions_all(rows, cols, count):
    """every (square, row, col, is_row)"""
    return np.array([(q, r, c, d) for q in range(count) for d in (1, 0) for r in range(rows) for c in range(cols)], dtype=np.uint64)


def positions_sampled(rows, cols, count, n, seed):
    rng = np.random.default_rng([seed, rows, cols, count, n])
    return np.stack([rng.integers(0, count, n), rng.integers(0, rows, n), rng.integers(0, cols, n), rng.integers(0, 2, n)], axis=1).astype(np.uint64)
