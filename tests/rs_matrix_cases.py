"""Case tables shared by the tests of the Reed-Solomon codec at every decode group width (test_rs_matrix_cases.py without a GPU,
test_gpu_rs_matrix.py with one): the codes, the received words with their errors placed after the lane ownership of k_rs_decode (lane l
of a group of W owns positions and coefficients l, l + W, ...), a set of words that miscorrect, the 2D shapes with their error patterns,
and what tests/rs_model.py answers for each of them -- computed once, shared and never modified.  Every builder takes a fixed seed.  No
GPU, no library."""
import functools, random
import rs_model as M

# ---- 1D codes ------------------------------------------------------------------------------------------------------------------
# by decode group width W; n % 4 takes every value, and n < W, W < n < 2 W and n > 2 W all occur
CODES_BY_W = {
    8: ((9, 1), (10, 8)),                                        # d = 8, 2
    16: ((13, 4), (19, 4), (24, 8)),                             # d = 9, 15, 16
    32: ((26, 9), (37, 6), (40, 8)),                             # d = 17, 31, 32
    64: ((40, 7), (70, 6), (70, 5), (135, 6), (255, 1)),         # d = 33, 64, 65 (two coefficients per lane), 129 (three), 254
}
CODES = tuple(c for w in sorted(CODES_BY_W) for c in CODES_BY_W[w])
DEV_CODES = CODES_BY_W[16] + CODES_BY_W[64]                      # once more through the device-pointer form
MISCORRECTION_CODE, MISCORRECTION_WORDS = (10, 8), 60


def width(d):
    """dec_w of rs_plan (mzk_rs_plan.h): the smallest power of two from 8 to 64 that is at least d"""
    w = 8
    while w < d and w < 64:
        w <<= 1
    return w


def error_counts(n, k):
    d, t = n - k, (n - k) // 2
    if d <= 32:
        return tuple(range(t + 3))
    return tuple(sorted({0, 1, 2, t // 2, t - 1, t, t + 1, t + 2}))


def edge_positions(n, k):
    d, w = n - k, width(n - k)
    return [p for p in dict.fromkeys([0, d - 1, d, n - 1, w - 1, w, w + 1]) if 0 <= p < n]


def placements(n, k, e, rnd):
    """[(name, positions)] for e errors, every way that fits: a. the edge list first (then others, when e is beyond it), b. all in the
    stride of one lane, from its first position on (with e = the length of the stride the whole stride is hit), c. a burst across W,
    d. anywhere"""
    w = width(n - k)
    edge = edge_positions(n, k)
    others = [p for p in range(n) if p not in edge]
    rnd.shuffle(others)
    out = [("edge", (edge + others)[:e])]
    if n > w:
        lanes = [c for c in range(w) if len(range(c, n, w)) >= e]
        if lanes:
            c = lanes[e % len(lanes)]
            out.append(("lane", list(range(c, n, w))[:e]))
    if e <= n:
        start = max(0, min(w - e // 2, n - e))
        out.append(("burst", list(range(start, start + e))))
        out.append(("random", rnd.sample(range(n), e)))
    return out


def _hit(rnd, cw, positions, mode):
    """error values cycle 1, 0xFF, random non-zero"""
    r = list(cw)
    for p in positions:
        r[p] ^= (1, 0xFF, rnd.randrange(1, 256))[mode % 3]
    return r


@functools.lru_cache(maxsize=None)
def words(n, k):
    """the batch of code (n, k): a tuple of (sent codeword, received word, error count, placement name).  The order interleaves the
    error counts, so that neighbouring groups of a wave are clean, correcting and failing side by side; the batch length is no multiple
    of the 256 / W codewords of a workgroup."""
    rnd = random.Random(7919 * n + k)
    rs = M.ReedSolomon(n, k)
    by_count, mode = [], 0
    for e in error_counts(n, k):
        row = []
        for name, pos in placements(n, k, e, rnd):
            cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
            row.append((tuple(cw), tuple(_hit(rnd, cw, pos, mode)), e, name))
            mode += 1
        by_count.append(row)
    out = []
    for i in range(max(len(r) for r in by_count)):
        out += [r[i] for r in by_count if i < len(r)]
    if len(out) % (256 // width(n - k)) == 0:
        cw = tuple(rs.encode_fixed([rnd.randrange(256) for _ in range(k)]))
        out.append((cw, cw, 0, "clean"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def expected(n, k):
    """the model on words(n, k): (corrected, messages, status, syndromes), one entry per word"""
    rs = M.ReedSolomon(n, k)
    return tuple(rs.decode_status(list(w[1])) + (rs.compute_syndromes(list(w[1])),) for w in words(n, k))


@functools.lru_cache(maxsize=None)
def miscorrection_words():
    """(sent, received, error count): t + 1 or t + 2 random errors at d = 2, where a word beyond t often lies within t of another
    codeword and is then `corrected` to that one"""
    n, k = MISCORRECTION_CODE
    rnd = random.Random(1008)
    rs = M.ReedSolomon(n, k)
    t = (n - k) // 2
    out = []
    for i in range(MISCORRECTION_WORDS):
        cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
        e = t + 1 + (i & 1)
        out.append((tuple(cw), tuple(_hit(rnd, cw, rnd.sample(range(n), e), 2)), e))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def miscorrection_expected():
    rs = M.ReedSolomon(*MISCORRECTION_CODE)
    return tuple(rs.decode_status(list(w[1])) for w in miscorrection_words())


# ---- wave encoder: the message comes in 64 bytes at a time -------------------------------------------------------------------------
WAVE_D, WAVE_BATCH = 40, 5                                       # batch 5: one wave of the second workgroup is idle
WAVE_K = (63, 64, 65, 127, 128, 129)
WAVE_K_STRIDED = (64, 129)

# ---- lane encoder: 1, 2, 4, 8 parity registers with pad 0 and k % 4 == 0, so that only the placement decides the read path --------------
LANE_CODES = ((12, 8), (16, 8), (24, 8), (40, 8))
LANE_BATCH = 70
# (name, offset of the messages, offset of the codewords, codeword stride - n): only the first is eligible for the word path
LANE_PLACEMENTS = (("aligned", 0, 0, 0), ("message+1", 1, 0, 0), ("output+2", 0, 2, 0), ("stride n+1", 0, 0, 1))


@functools.lru_cache(maxsize=None)
def encode_case(n, k, batch):
    """(messages, model codewords) as tuples of tuples"""
    rnd = random.Random(104729 * n + 131 * k + batch)
    rs = M.ReedSolomon(n, k)
    msgs = tuple(tuple(rnd.randrange(256) for _ in range(k)) for _ in range(batch))
    return msgs, tuple(tuple(rs.encode_fixed(list(m))) for m in msgs)


# ---- 2D ------------------------------------------------------------------------------------------------------------------------
SHAPES = (
    (20, 12, 64),        # size 8; column d = 12, W = 16; the row pass is eligible for the word path
    (21, 13, 60),        # everything odd: byte paths, a zero-padded matrix
    (75, 11, 100),       # column d = 65: wave encoder and W = 64 decode, both strided, two coefficients per lane; row d = 1
    (10, 50, 100),       # column d = 0: the copy form and a clean decode whatever the column holds; row d = 40
    (48, 48, 256),       # d = 32 both ways: 8 registers, pad 0
    (12, 70, 36),        # row_n > 64: 70 column statuses; row W = 64
)


def patterns(shape):
    """A: column c gets c % (t_col + 1) errors; B: c % (t_col + 2); C: the last column beyond repair.  A column code with d = 0 has
    no syndromes and answers 0 for every word, so (10,50,100) has no pattern C: there the word beyond repair is a row (pattern R)."""
    return ("A", "B", "C") if shape[0] > M.isqrt_ceil(shape[2]) else ("A", "B", "R")


CASES_2D = tuple((s, p) for s in SHAPES for p in patterns(s))


@functools.lru_cache(maxsize=None)
def clean_2d(shape):
    """(data, model code)"""
    col_n, row_n, ml = shape
    rnd = random.Random(col_n * 10007 + row_n * 101 + ml)
    data = tuple(rnd.randrange(256) for _ in range(ml))
    code = M.ReedSolomon2D(col_n, row_n, ml).encode(list(data))
    return data, tuple(tuple(r) for r in code)


@functools.lru_cache(maxsize=None)
def case_2d(shape, pattern):
    """(data, clean code, received code, (result or None, column statuses, row statuses) of the model)"""
    col_n, row_n, ml = shape
    rs = M.ReedSolomon2D(col_n, row_n, ml)
    data, code = clean_2d(shape)
    rnd = random.Random(col_n * 7 + row_n * 1009 + ml * 31 + ord(pattern))
    hit = [list(r) for r in code]
    t_col, t_row = (col_n - rs.size) // 2, (row_n - rs.size) // 2
    if pattern in "AB":
        for c in range(row_n):
            for r in rnd.sample(range(col_n), c % (t_col + (1 if pattern == "A" else 2))):
                hit[r][c] ^= rnd.randrange(1, 256)
    elif pattern == "C":
        c = row_n - 1
        while True:
            col = [code[r][c] for r in range(col_n)]
            for r in rnd.sample(range(col_n), min(col_n, t_col + 1 + rnd.randrange(2))):
                col[r] ^= rnd.randrange(1, 256)
            if rs.col.decode_status(col)[2] == 255:
                break
        for r in range(col_n):
            hit[r][c] = col[r]
    else:                                                        # R: the last message row; the column code (d = 0) passes it on as it is
        assert pattern == "R" and t_col == 0 and col_n == rs.size
        r = col_n - 1
        while True:
            row = list(code[r])
            for c in rnd.sample(range(row_n), t_row + 1 + rnd.randrange(2)):
                row[c] ^= rnd.randrange(1, 256)
            if rs.row.decode_status(row)[2] == 255:
                break
        hit[r] = row
    return data, code, tuple(tuple(r) for r in hit), rs.decode_status(hit)
