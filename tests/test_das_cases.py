"""tests/das_cases.py is not vacuous: its shapes reach every item pattern, every message form and every path form of the kernels of
mzk_das.hip, stay within the size limits of the GPU file, and its inputs cannot hide a row / column mix-up.  CPU only.

Two forms cannot occur in any tree of merkle.rs and are asserted ABSENT for every leaf count, so that no table can be blamed for
missing them: a tree whose items are all two leaves wide (there are M = 2^floor(log2 n) items and n < 2 M leaves), and a 33-byte
message with the digest first (mid = len / 2 puts the smaller half left, so the one-leaf item of a three-leaf slice is the left one)."""
import numpy as np
import das_cases as C
import das_model as M


def _leaf_counts():
    """leaf counts of every tree the commit cases hash: rows have `cols` leaves, columns `rows`"""
    return sorted({n for r, c, _ in C.commit_cases() for n in (r, c)})


def _level1_messages(n):
    sizes = M.item_sizes(n)
    return {(sizes[i], sizes[i + 1]) for i in range(0, len(sizes), 2)}


def test_shapes_are_the_issue_s_and_within_the_limits():
    cases = C.commit_cases()
    assert len(cases) == len(set(cases))
    for n in list(range(2, 34)) + [63, 64, 65, 127, 128, 129, 254, 255]:
        assert {(n, n, q) for q in (1, 2, 3)} <= set(cases)
        assert ((n, n, 65) in cases) == (n <= 17)
    for rc in [(2, 255), (255, 2), (3, 5), (5, 3), (17, 64), (64, 17)]:
        assert {rc + (q,) for q in (1, 2, 3)} <= set(cases)
    for r, c, q in cases + [C.OPEN_SAMPLED[:3]] + [(n, n, 3) for n in C.OPEN_ALL_SIDES] + C.TIE_SHAPES:
        assert 2 <= r <= 255 and 2 <= c <= 255
        assert q <= 3 or (q == 65 and max(r, c) <= 17)
    assert C.OPEN_ALL_SIDES == list(range(2, 18)) + [31, 32, 33] and C.OPEN_SAMPLED == (255, 255, 3, 512)
    assert len(C.TIE_SHAPES) == 3


def test_every_item_pattern_occurs():
    pats = {n: set(M.item_sizes(n)) for n in _leaf_counts()}
    assert {1} in pats.values(), "no tree whose items are all one leaf (a power of two)"
    assert {1, 2} in pats.values(), "no tree with both kinds of item"
    assert all(set(M.item_sizes(n)) != {2} for n in range(2, 511)), "a tree of two-leaf items only exists after all: add it to the tables"
    # among the mixed ones: a single two-leaf item, a single one-leaf item
    assert any(M.item_sizes(n).count(2) == 1 for n in _leaf_counts()) and any(M.item_sizes(n).count(1) == 1 for n in _leaf_counts())


def test_every_message_form_occurs():
    forms = set().union(*(_level1_messages(n) for n in _leaf_counts()))
    assert forms == {(1, 1), (1, 2), (2, 2)}            # 2 bytes, 33 bytes, 64 bytes
    for n in range(2, 511):
        assert (2, 1) not in _level1_messages(n), n      # 33 bytes with the digest first: merkle.rs cannot produce it
    # the data-root trees: all 64-byte messages, over items of one and of two roots
    roots = {frozenset(M.item_sizes(r + c)) for r, c, _ in C.commit_cases()}
    assert frozenset({1}) in roots and frozenset({1, 2}) in roots


def test_depth_zero_samples_occur_and_stay_below_a_third():
    some = 0
    for n in sorted(set(C.OPEN_ALL_SIDES) | set(C.OPEN_SAMPLED[:2])):
        nt = M.nonterminating(n)
        some += len(nt)
        assert 3 * len(nt) <= n, n
        if n & (n - 1) == 0:
            assert not nt, n
    assert some > 0 and len(M.nonterminating(3)) == 1
    # the three path forms: depth D + 1 (two-leaf item), D (one-leaf items side by side), 0
    for n in (3, 5, 6, 33):
        assert n in C.OPEN_ALL_SIDES
    leafs = [bytes([i]) for i in range(6)]
    assert sorted({len(p) if p else 0 for p in (M.open_(i, leafs) for i in range(6))}) == [0, 3]
    leafs = [bytes([i]) for i in range(5)]
    assert sorted({len(p) if p else 0 for p in (M.open_(i, leafs) for i in range(5))}) == [0, 2, 3]
    # the sampled case sees all three as well
    pos = C.positions_sampled(*C.OPEN_SAMPLED, seed=7)
    nt = M.nonterminating(255)
    hit = sum(1 for q, r, c, d in pos.tolist() if (c if d else r) in nt)
    assert 0 < hit < len(pos) / 3


def test_inputs_are_never_symmetric_and_positions_cover_everything():
    for r, c, q in C.commit_cases():
        m = C.squares(r, c, q, seed=1)
        assert m.shape == (q, r, c) and m.dtype == np.uint8
        if r == c:
            assert all(not np.array_equal(m[i], m[i].T) for i in range(q)), (r, c, q)
        assert np.array_equal(m, C.squares(r, c, q, seed=1))
    p = C.positions_all(3, 5, 2)
    assert len(p) == 2 * 2 * 15 and len({tuple(x) for x in p.tolist()}) == len(p)
    s = C.positions_sampled(*C.OPEN_SAMPLED, seed=7)
    assert s.shape == (512, 4) and s[:, 0].max() == 2 and set(s[:, 3].tolist()) == {0, 1}
