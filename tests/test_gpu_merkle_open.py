"""The three ways to open a Merkle tree at the C boundary -- mzk_merkle_open, mzk_merkle_open_batch and mzk_merkle_open_multi, which
share one gather-and-unpack path -- called through lib() into numpy buffers pre-filled with 0xA5: they must leave identical paths,
path_lens and depths, equal to tests/merkle_model.py, and must not touch a byte behind an entry's length.  Field trees of all four
field ids at 2, 4 and 64 leaves (a depth-1 path holds no digest at all), one call over several trees against the trees opened one by
one, and byte-leaf trees of 2, 4, 5, 6 and 7 leaves against the reference's recursion restated in tests/das_model.py (open_: None where
Merkle::open would not end; those indices are MZK_E_LENGTH).  The layout and the unpack themselves run on the host in
test_hostcheck_merkle_open.py."""
import ctypes
import numpy as np
import pytest
import das_model
import merkle_model as mm

pytestmark = pytest.mark.gpu

SZ = ctypes.c_size_t
E_LENGTH = -5
NAMES = {mm.FR: "Fr", mm.M128: "M128", mm.M64: "M64", mm.M64X3: "M64X3"}
FIELD_TREES = [(fid, False) for fid in (mm.FR, mm.M128, mm.M64, mm.M64X3)] + [(mm.FR, True), (mm.M128, True)]


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _buffers(entries, stride):
    return np.full((entries, stride), 0xA5, dtype=np.uint8), np.full(entries, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)


def _ok(mz, rc):
    assert rc == 0, mz.lib().mzk_last_error().decode()


def open_single(mz, tree, index, entries, stride):
    """mzk_merkle_open: (rc, depth, paths (entries, stride), path_lens (entries,))"""
    paths, lens = _buffers(entries, stride)
    d = SZ(12345)
    rc = mz.lib().mzk_merkle_open(tree._h, SZ(index), _ptr(paths), SZ(stride), _ptr(lens), ctypes.byref(d))
    return rc, d.value, paths, lens


def open_batch(mz, tree, idx, depth, stride):
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    paths, lens = _buffers(idx.shape[0] * depth, stride)
    d = SZ(12345)
    _ok(mz, mz.lib().mzk_merkle_open_batch(tree._h, _ptr(idx), SZ(idx.shape[0]), _ptr(paths), SZ(stride), _ptr(lens), ctypes.byref(d)))
    return d.value, paths, lens


def open_multi(mz, trees, index_lists, stride):
    """mzk_merkle_open_multi over trees (None: a null handle): (depths, paths, path_lens)"""
    T = len(trees)
    flat = np.ascontiguousarray([i for ix in index_lists for i in ix], dtype=np.uint64)
    handles = (ctypes.c_void_p * T)(*[t._h if t is not None else None for t in trees])
    counts = (SZ * T)(*[len(ix) for ix in index_lists])
    depths = (SZ * T)(*[12345] * T)
    entries = sum(len(ix) * (t.n.bit_length() - 1) for t, ix in zip(trees, index_lists) if t is not None)
    paths, lens = _buffers(entries, stride)
    _ok(mz, mz.lib().mzk_merkle_open_multi(handles, SZ(T), _ptr(flat), counts, _ptr(paths), SZ(stride), _ptr(lens), depths))
    return list(depths), paths, lens


def expected(fid, arr, neg, nd, idx, stride):
    """merkle_model.expected_open on a 0xA5 background: (paths (count * depth, stride), path_lens (count * depth,))"""
    paths, lens = mm.expected_open(fid, arr, nd, idx, stride, neg)
    paths, lens = paths.reshape(-1, stride), lens.reshape(-1)
    out = np.full(paths.shape, 0xA5, dtype=np.uint8)
    keep = np.arange(stride)[None, :] < lens[:, None]
    out[keep] = paths[keep]
    return out, lens


@pytest.fixture(scope="module")
def field_tree(mz):
    """field_tree(fid, n, signed) -> (tree, elements, signs, digests by the model): built once per module, closed behind it"""
    built = {}

    def get(fid, n, signed):
        key = (fid, n, signed)
        if key not in built:
            arr, neg = mm.signed_vector(fid, n, 40 + n) if signed else (mm.leaf_vector(fid, n, 40 + n), None)
            blob, off = mm.leaves(fid, arr, neg)
            tree = mz.MerkleTree(fid, arr, negative=neg) if signed else mz.MerkleTree(fid, arr)
            built[key] = (tree, arr, neg, mm.nodes(blob, off))
        return built[key]

    yield get
    for tree, _, _, _ in built.values():
        tree.close()


@pytest.mark.parametrize("n", [2, 4, 64])
@pytest.mark.parametrize("fid,signed", FIELD_TREES, ids=[NAMES[f] + ("-signed" if s else "") for f, s in FIELD_TREES])
def test_the_three_calls_agree_with_each_other_and_the_model(mz, field_tree, fid, signed, n):
    tree, arr, neg, nd = field_tree(fid, n, signed)
    depth, stride = n.bit_length() - 1, 64
    idx = np.arange(n, dtype=np.uint64)
    want, want_lens = expected(fid, arr, neg, nd, idx, stride)
    d, paths, lens = open_batch(mz, tree, idx, depth, stride)
    assert d == depth
    assert np.array_equal(lens, want_lens)
    assert np.array_equal(paths, want), mm.first_mismatch(paths.reshape(n, depth, stride), want.reshape(n, depth, stride), idx)
    ds, mpaths, mlens = open_multi(mz, [tree], [idx], stride)
    assert ds == [depth] and np.array_equal(mpaths, paths) and np.array_equal(mlens, lens)
    for i in range(n):
        rc, d1, p1, l1 = open_single(mz, tree, i, depth, stride)
        _ok(mz, rc)
        assert d1 == depth, i
        assert np.array_equal(p1, paths[i * depth:(i + 1) * depth]) and np.array_equal(l1, lens[i * depth:(i + 1) * depth]), i


def test_no_opening_still_writes_the_depth(mz, field_tree):
    tree = field_tree(mm.M128, 64, False)[0]
    d = SZ(12345)
    _ok(mz, mz.lib().mzk_merkle_open_batch(tree._h, None, SZ(0), None, SZ(64), None, ctypes.byref(d)))
    assert d.value == 6


def test_several_trees_in_one_call_equal_the_trees_one_by_one(mz, field_tree):
    """a 2-leaf Fr tree, a null handle with no index, a 64-leaf signed M128 tree (an index repeated) and an 8-leaf M64X3 tree"""
    shapes = [(mm.FR, 2, False, [1, 0]), None, (mm.M128, 64, True, [5, 63, 5, 0, 32]), (mm.M64X3, 8, False, [7, 2, 2, 4])]
    stride = 64
    trees, lists, want, want_lens, want_depths = [], [], [], [], []
    for sh in shapes:
        if sh is None:
            trees.append(None); lists.append([]); want_depths.append(0)
            continue
        fid, n, signed, idx = sh
        tree, arr, neg, nd = field_tree(fid, n, signed)
        depth = n.bit_length() - 1
        d, p, l = open_batch(mz, tree, idx, depth, stride)
        model, model_lens = expected(fid, arr, neg, nd, idx, stride)
        assert d == depth and np.array_equal(p, model) and np.array_equal(l, model_lens)
        trees.append(tree); lists.append(idx); want.append(p); want_lens.append(l); want_depths.append(depth)
    depths, paths, lens = open_multi(mz, trees, lists, stride)
    assert depths == want_depths
    assert np.array_equal(paths, np.concatenate(want)) and np.array_equal(lens, np.concatenate(want_lens))


@pytest.mark.parametrize("n", [2, 4, 5, 6, 7])
def test_byte_trees_open_as_the_reference_recursion(mz, n):
    rng = np.random.default_rng(n)
    leaf_lens = [0, 33, 1, 32, 70, 5, 31][:n]      # an empty leaf, leaves shorter and longer than a digest
    leafs = [rng.integers(0, 256, size=k, dtype=np.uint8).tobytes() for k in leaf_lens]
    stride, entries = max(32, max(leaf_lens)), 4
    tree = mz.MerkleTree(leaves=leafs)
    try:
        assert tree.root() == das_model.commit(leafs)
        opened = refused = 0
        for i in range(n):
            want = das_model.open_(i, leafs)
            rc, depth, paths, lens = open_single(mz, tree, i, entries, stride)
            if want is None:      # the one-leaf half of a three-leaf slice
                assert rc == E_LENGTH, i
                refused += 1
                continue
            _ok(mz, rc)
            opened += 1
            assert depth == len(want) <= entries, i
            want_paths, want_lens = _buffers(entries, stride)
            for k, e in enumerate(want):
                want_paths[k, :len(e)] = np.frombuffer(e, dtype=np.uint8)
                want_lens[k] = len(e)
            assert np.array_equal(lens, want_lens), i
            assert np.array_equal(paths, want_paths), i
        assert opened >= 2 and refused == len(das_model.nonterminating(n)) == {2: 0, 4: 0, 5: 1, 6: 2, 7: 1}[n]
    finally:
        tree.close()
