"""CPU: tests/merkle_model.py (numpy + hashlib; the reference of tests/test_gpu_merkle_levels.py) against the C oracle
(oracle/mzk_oracle_merkle.c), with which it shares no code: leaf bytes against orc_bincode_field / orc_bincode_field_signed (Fr, M128)
and goldilocks_model's leaf (M64, M64X3), roots against orc.merkle_commit_ref for 2^1 .. 2^12 leaves of all four fields, paths against
orc.merkle_open_ref, every level against the literal fri_prove_model.merkle_levels, and the reference's own test (merkle.rs:76-93).
Then the properties the GPU tests rely on: the covering index set covers, the leaf vectors hold every digit-count combination."""
import numpy as np
import pytest
import fri_prove_model as fpm
import goldilocks_model as gm
import merkle_model as mm
import orc

FIELDS = [mm.FR, mm.M128, mm.M64, mm.M64X3]
IDS = ["Fr", "M128", "M64", "M64X3"]
ORC_ID = {mm.FR: orc.FR, mm.M128: orc.M128}


def _independent_leaves(fid, arr, neg=None):
    """the leaf bytes without merkle_model: the C oracle for Fr / M128, goldilocks_model for the Goldilocks ids"""
    if fid in ORC_ID:
        if neg is None:
            return orc.field_leaves_fast(ORC_ID[fid], arr)
        return [orc.bincode_field_signed(v, mm.LIMBS[fid], s) for v, s in zip(orc.from_limbs(arr), neg)]
    F = gm.FIELDS[fid]
    return [F.leaf(e) for e in mm.to_ints(fid, arr)]


@pytest.mark.parametrize("fid", FIELDS, ids=IDS)
@pytest.mark.parametrize("lg", range(1, 13))
def test_leaves_roots_levels_and_paths_against_the_oracle(fid, lg):
    n = 1 << lg
    arr = mm.leaf_vector(fid, n, 100 + lg)
    blob, off = mm.leaves(fid, arr)
    lv = mm.leaf_list(blob, off)
    assert lv == _independent_leaves(fid, arr)
    nd = mm.nodes(blob, off)
    assert nd.shape == (n - 1, 32)
    assert mm.root(nd) == orc.merkle_commit_ref(lv)
    levels = fpm.merkle_levels(lv)                          # the literal form, level by level
    for l, want in enumerate(levels, start=1):
        s = mm.level_start(n, l)
        assert nd[s:s + (n >> l)].tobytes() == b"".join(want), l
    idx = np.arange(n) if lg <= 5 else np.unique(np.array([0, 1, 2, n - 1, n - 2, n // 2, n // 2 - 1, n // 3, 161, 162 + 5], dtype=np.int64) % n)
    stride = 64
    paths, plens = mm.expected_open(fid, arr, nd, idx, stride)
    assert paths.shape == (len(idx), lg, stride) and plens.shape == (len(idx), lg)
    for q, i in enumerate(idx.tolist()):
        want = orc.merkle_open_ref(i, lv)
        got = [paths[q, l, :int(plens[q, l])].tobytes() for l in range(lg)]
        assert got == want, i
        assert not paths[q, 0, int(plens[q, 0]):].any() and not paths[q, 1:, 32:].any()      # nothing behind an entry
        assert orc.merkle_verify_ref(mm.root(nd), i, got, lv[i])


@pytest.mark.parametrize("fid", [mm.FR, mm.M128], ids=["Fr", "M128"])
@pytest.mark.parametrize("lg", [1, 4, 9, 11])
def test_signed_leaves_against_the_oracle(fid, lg):
    n = 1 << lg
    mag, neg = mm.signed_vector(fid, n, 200 + lg)
    blob, off = mm.leaves(fid, mag, neg)
    lv = mm.leaf_list(blob, off)
    assert lv == _independent_leaves(fid, mag, neg)
    zero = ~mag.any(axis=1)
    assert (zero & (neg == 1)).any() and all(lv[i] == bytes(9) for i in np.flatnonzero(zero))      # -0 is NoSign
    assert n < 16 or (any(l[0] == 0xff for l in lv) and any(l[0] == 1 for l in lv))
    nd = mm.nodes(blob, off)
    assert mm.root(nd) == orc.merkle_commit_ref(lv)
    idx = np.array([0, 1, n - 1, n // 2], dtype=np.int64) % n
    paths, plens = mm.expected_open(fid, mag, nd, idx, 48, neg)
    for q, i in enumerate(idx.tolist()):
        assert [paths[q, l, :int(plens[q, l])].tobytes() for l in range(lg)] == orc.merkle_open_ref(i, lv)


def test_reference_merkle_test_leaf1_to_leaf4():
    """merkle.rs:76-93 (pinned on a hashlib restatement in test_oracle_merkle.py): the model's levels over byte leaves"""
    lv = [b"leaf1", b"leaf2", b"leaf3", b"leaf4"]
    blob = np.frombuffer(b"".join(lv), dtype=np.uint8)
    off = np.array([0, 5, 10, 15, 20], dtype=np.int64)
    nd = mm.nodes(blob, off)
    assert mm.root(nd) == orc.merkle_commit_ref(lv)
    proof = orc.merkle_open_ref(2, lv)
    assert proof == [lv[3], nd[0].tobytes()]
    assert orc.merkle_verify_ref(mm.root(nd), 2, proof, lv[2]) and not orc.merkle_verify_ref(mm.root(nd), 2, proof, lv[3])


def test_a_batch_is_its_trees_side_by_side():
    """nodes(stop = trees): the last rows are the roots of the trees taken one by one"""
    per, trees = 16, 5
    arr = mm.leaf_vector(mm.M128, per * trees, 7)
    blob, off = mm.leaves(mm.M128, arr)
    nd = mm.nodes(blob, off, stop=trees)
    assert nd.shape == (per * trees - trees, 32)
    for t in range(trees):
        b, o = mm.leaves(mm.M128, arr[t * per:(t + 1) * per])
        assert nd[nd.shape[0] - trees + t].tobytes() == orc.merkle_commit_ref(mm.leaf_list(b, o))


@pytest.mark.parametrize("n", [2, 4, 32, 1 << 14, 1 << 15, 1 << 17])
def test_the_covering_set_holds_every_digest_and_leaf(n):
    idx = mm.covering_indices(n).astype(np.int64)
    depth = n.bit_length() - 1
    assert len(idx) == (n if n <= 1 << 14 else n // 2)
    seen = np.zeros(n - 1, dtype=bool)
    for l in range(1, depth):
        seen[mm.level_start(n, l) + ((idx >> l) ^ 1)] = True
    assert seen[:-1].all() and not seen[-1]                 # every digest but the root, which no path holds
    revealed = np.zeros(n, dtype=bool)
    revealed[idx ^ 1] = True
    assert revealed[1::2].all() and (revealed.all() or n > 1 << 14)


@pytest.mark.parametrize("fid", FIELDS, ids=IDS)
def test_leaf_vectors_hold_every_digit_count_combination(fid):
    n = 1 << 11
    arr = mm.leaf_vector(fid, n, 5)
    C, K, D, comps = mm.combos(fid), len(mm.CLASSES[fid]), mm.DIGITS[fid], mm.COMPS[fid]
    assert C == {mm.FR: 81, mm.M128: 25, mm.M64: 9, mm.M64X3: 81}[fid]
    vals = mm.to_ints(fid, arr)
    flat = [c for v in vals for c in (v if comps > 1 else (v,))]
    assert all(0 <= c < mm.MOD[fid] for c in flat)           # canonical
    counts = np.stack([mm._digit_count(mm._digits(arr[:, j:j + 1] if comps > 1 else arr)) for j in range(comps)], axis=1)
    seen, P = {}, n // 2
    rest = np.ones(n, dtype=bool)
    for i in range(P):
        j = i if 2 * i < P else P - 1 - i                   # the formula of pair_combination, written out
        if (j // C) % 2 == 0:
            c = (j + j // (2 * C)) % C
            want = (mm.CLASSES[fid][c // K], mm.CLASSES[fid][c % K])
            assert (tuple(counts[2 * i]), tuple(counts[2 * i + 1])) == want, i
            seen.setdefault(c, []).append(i)
            rest[2 * i:2 * i + 2] = False
    assert sorted(seen) == list(range(C))
    # every combination on even and on odd pairs, in the first and in the last 128-pair workgroup of the tree, and at several
    # positions of a 64-pair workgroup; (a, b) and (b, a) both occur, so every class meets the even and the odd lane of a pair
    for c, v in seen.items():
        assert {i % 2 for i in v} == {0, 1}, c
        assert min(v) < 128 and max(v) >= P - 128, c
        assert len(v) >= 6 and len({i % 64 for i in v}) >= 4, c      # (C = 81 at 2^11 leaves: four runs per half)
    # the rest is uniform: full-length elements almost everywhere
    assert (counts[rest] == D).mean() > 0.99
    # zero digits below the top do occur in the special elements
    if D > 2:
        dig = mm._digits(arr)[~rest]
        inner = [(row[:k - 1] == 0).any() for row, k in zip(dig, counts[~rest][:, 0]) if k > 2]
        assert any(inner) and not all(inner)


def test_goldilocks_classes_are_the_leaf_length_classes_of_the_gpu_test():
    import test_gpu_goldilocks as tg      # (a GPU test module, but it touches neither the library nor the device at import: only its fixture does)
    for F in (gm.M64, gm.M64X3):
        es = tg._leaf_cases(F, 8)[:8] + tg._leaf_cases(F, 13)       # (the base list, cycled)
        got = {tuple(len(fpm.leaf(c)) // 4 - 2 for c in (e if F.limbs == 3 else (e,))) for e in es}
        assert got == set(mm.CLASSES[F.fid]), F.name
    # every leaf length the classes give
    arr = mm.leaf_vector(mm.M64X3, 1 << 9, 1)
    blob, off = mm.leaves(mm.M64X3, arr)
    assert set(np.diff(off).tolist()) >= {8, 21, 25, 30, 34, 39, 43, 55, 59}
