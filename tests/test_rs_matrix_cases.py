"""The case tables of tests/rs_matrix_cases.py and the model alone, without a GPU: what keeps test_gpu_rs_matrix.py from passing
vacuously.  Every width occurs, every code sees every outcome, the words that must be corrected are, the miscorrection set does
miscorrect, and each 2D pattern does what its name says.  The tables checked here are the ones the GPU file runs: neither file filters
or skips a case."""
import pytest
import rs_matrix_cases as C
import rs_model as M


def test_every_group_width_and_its_boundaries_occur():
    assert {C.width(n - k) for n, k in C.CODES} == {8, 16, 32, 64} == set(C.CODES_BY_W)
    for w, codes in C.CODES_BY_W.items():
        assert all(C.width(n - k) == w for n, k in codes)
    ds = {n - k for n, k in C.CODES}
    assert {8, 9, 16, 17, 32, 33, 64, 65, 129} <= ds                      # d = W, W + 1; two and three coefficients per lane
    assert {n % 4 for n, k in C.CODES} == {0, 1, 2, 3}
    rel = set()
    for n, k in C.CODES:
        w = C.width(n - k)
        rel.add("below" if n < w else "between" if w < n < 2 * w else "beyond" if n > 2 * w else "at")
    assert {"below", "between", "beyond"} <= rel
    assert all(any((n - k) % 2 for n, k in C.CODES_BY_W[w]) for w in (16, 32, 64))      # odd d: t2 != d at every width above 8


@pytest.mark.parametrize("n, k", C.CODES)
def test_every_outcome_occurs_and_up_to_t_errors_are_corrected(n, k):
    words, want = C.words(n, k), C.expected(n, k)
    t, w = (n - k) // 2, C.width(n - k)
    counts = C.error_counts(n, k)
    assert len(words) == len(want) and len(words) % (256 // w) != 0
    assert {e for _, _, e, _ in words} == set(counts)
    if n - k <= 32:
        assert counts == tuple(range(t + 3))
    status = {st for _, _, st, _ in want}
    # every count up to t is a status: all of 0 .. t at d <= 32, the eight listed counts beyond (a status below t is the number of
    # errors, and the table has only those)
    assert {e for e in counts if e <= t} <= status
    if t >= 1:
        assert 255 in status
    for (sent, recv, e, name), (corr, msg, st, syn) in zip(words, want):
        assert sum(a != b for a, b in zip(sent, recv)) == e, (e, name)
        assert (not any(syn)) == (e == 0)
        if e <= t:
            assert st == e and tuple(corr) == sent and tuple(msg) == sent[n - k:], (e, name)
    # the order interleaves: no two neighbours of the first round share an error count
    first = [e for _, _, e, _ in words[:len(counts)]]
    assert first == list(counts)


@pytest.mark.parametrize("n, k", C.CODES)
def test_errors_follow_lane_ownership(n, k):
    w, t = C.width(n - k), (n - k) // 2
    words = C.words(n, k)
    names = {name for _, _, e, name in words}
    assert {"edge", "burst", "random"} <= names and (("lane" in names) == (n > w))
    where = lambda s, r: [i for i, (a, b) in enumerate(zip(s, r)) if a != b]
    if n > w:
        lane = [(e, where(s, r)) for s, r, e, name in words if name == "lane" and e >= 2]
        assert lane and all(len({p % w for p in pos}) == 1 for e, pos in lane)              # two or more errors, one lane
    if n > w + 1 and t >= 3:
        assert any({w - 1, w, w + 1} <= set(where(s, r)) for s, r, e, name in words if e <= t)
    # value 1, value 0xFF and other values all occur
    diffs = {a ^ b for s, r, _, _ in words for a, b in zip(s, r) if a != b}
    assert {1, 0xFF} <= diffs and len(diffs) > 2


def test_a_whole_stride_is_hit_within_t_at_some_code_of_every_width_above_8():
    for w in (16, 32, 64):
        found = False
        for n, k in C.CODES_BY_W[w]:
            for s, r, e, name in C.words(n, k):
                pos = [i for i, (a, b) in enumerate(zip(s, r)) if a != b]
                found |= name == "lane" and 2 <= e <= (n - k) // 2 and pos == list(range(pos[0], n, w))
        assert found, w


def test_the_miscorrection_set_miscorrects():
    n, k = C.MISCORRECTION_CODE
    t = (n - k) // 2
    words, want = C.miscorrection_words(), C.miscorrection_expected()
    assert len(words) == len(want) == C.MISCORRECTION_WORDS == 60
    assert all(e in (t + 1, t + 2) and sum(a != b for a, b in zip(s, r)) == e for s, r, e in words)
    wrong = [i for i, ((s, r, e), (corr, msg, st)) in enumerate(zip(words, want)) if 1 <= st <= t and tuple(corr) != s]
    none = [i for i, (_, _, st) in enumerate(want) if st == 255]
    assert len(wrong) >= 3 and len(none) >= 3
    rs = M.ReedSolomon(n, k)
    for i in wrong:                                                         # accepted because it IS a codeword, only not the sent one
        assert not any(rs.compute_syndromes(want[i][0]))


@pytest.mark.parametrize("shape", C.SHAPES)
def test_2d_patterns_do_what_their_names_say(shape):
    col_n, row_n, ml = shape
    size = M.isqrt_ceil(ml)
    t_col = (col_n - size) // 2
    data, code = C.clean_2d(shape)
    assert M.ReedSolomon2D(*shape).decode_status([list(r) for r in code]) == (list(data), [0] * row_n, [0] * size)
    assert [p for s, p in C.CASES_2D if s == shape] == list(C.patterns(shape))
    # A: every column correctable, the data comes back
    _, _, hit, (res, cs, rs_) = C.case_2d(shape, "A")
    assert res == list(data) and 255 not in cs and 255 not in rs_
    assert cs == [c % (t_col + 1) for c in range(row_n)]
    # B: the columns beyond t are there
    _, _, hit, (res, cs, rs_) = C.case_2d(shape, "B")
    per_col = [sum(hit[r][c] != code[r][c] for r in range(col_n)) for c in range(row_n)]
    assert per_col == [c % (t_col + 2) for c in range(row_n)]
    if shape == (10, 50, 100):
        assert cs == [0] * row_n and any(rs_) and 255 not in rs_ and res == list(data)
    if "C" in C.patterns(shape):
        _, _, hit, (res, cs, rs_) = C.case_2d(shape, "C")
        assert res is None and [c for c, st in enumerate(cs) if st == 255] == [row_n - 1]
        assert all(hit[r][c] == code[r][c] for r in range(col_n) for c in range(row_n - 1))
    else:
        # no syndromes, no failure: the column code of this shape cannot answer 255, the row code can
        assert col_n == size
        col = M.ReedSolomon(col_n, size)
        assert all(col.decode_status([(7 * i + j) & 0xFF for i in range(col_n)])[2] == 0 for j in range(16))
        _, _, hit, (res, cs, rs_) = C.case_2d(shape, "R")
        assert res is None and cs == [0] * row_n and [i for i, st in enumerate(rs_) if st == 255] == [size - 1]


def test_2d_shapes_reach_what_they_are_there_for():
    reach = {s: (s[0] - M.isqrt_ceil(s[2]), s[1] - M.isqrt_ceil(s[2])) for s in C.SHAPES}          # (column d, row d)
    assert reach == {(20, 12, 64): (12, 4), (21, 13, 60): (13, 5), (75, 11, 100): (65, 1), (10, 50, 100): (0, 40), (48, 48, 256): (32, 32),
                     (12, 70, 36): (6, 64)}
    assert C.case_2d((12, 70, 36), "C")[3][1][69] == 255


def test_encoder_tables():
    assert all(n - k in (4, 8, 16, 32) and k % 4 == 0 for n, k in C.LANE_CODES)                      # pad 0: 1, 2, 4, 8 registers
    assert C.WAVE_D > 32 and set(C.WAVE_K_STRIDED) <= set(C.WAVE_K) and C.WAVE_BATCH % 4 == 1 and C.WAVE_BATCH > 4
    assert all(kk + C.WAVE_D <= 255 for kk in C.WAVE_K)
    msgs, code = C.encode_case(16, 8, 3)
    assert all(c[8:] == m for m, c in zip(msgs, code))
