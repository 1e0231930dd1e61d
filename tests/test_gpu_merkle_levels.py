"""The Merkle level schedule on the GPU, node by node: every distinct step list of merkle_hash_levels (mzk_merkle_plan.h; pinned on the
host by test_hostcheck_merkle_plan.py) from 2^11 to 2^19 leaves, compared with tests/merkle_model.py (numpy + hashlib, pinned on the
oracle by test_merkle_model.py).  A root only proves the digests that the kernels hand upwards through LDS; the copy of every digest
in global memory is what the openings read, so each tree is opened at a covering index set through mzk_merkle_open_batch into one
numpy buffer and compared with the model in one np.array_equal -- every digest of every level and every revealed leaf.  The leaf
vectors hold every combination of the two digit counts of a leaf pair (the odd lane of k_merkle_leaf_pairs_lp starts behind the even
lane's digits and shares words with it).  Every root here is compared with hashlib through the model."""
import ctypes, hashlib
import numpy as np
import pytest
import merkle_model as mm
import orc

pytestmark = pytest.mark.gpu

SZ = ctypes.c_size_t
NAMES = {mm.FR: "Fr", mm.M128: "M128", mm.M64: "M64", mm.M64X3: "M64X3"}
STRIDE = {mm.FR: 48, mm.M128: 32, mm.M64: 64, mm.M64X3: 64}      # path entry stride: the longest leaf (41, 25, 17, 59 bytes) fits


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_MODEL = {}


def model(fid, n, signed=False, trees=1):
    """(elements, Sign::Minus flags or None, every digest by the model) of the leaf vector of n elements: computed once per module"""
    key = (fid, n, signed, trees)
    if key not in _MODEL:
        arr, neg = mm.signed_vector(fid, n, 1000 + n % 9973) if signed else (mm.leaf_vector(fid, n, 1000 + n % 9973), None)
        blob, off = mm.leaves(fid, arr, neg)
        _MODEL[key] = (arr, neg, mm.nodes(blob, off, stop=trees))
    return _MODEL[key]


def open_batch(mz, tree, idx, stride):
    """mzk_merkle_open_batch into zeroed numpy buffers: (paths (count, depth, stride), path_lens (count, depth))"""
    idx = np.ascontiguousarray(idx, dtype=np.uint64)
    depth = tree.n.bit_length() - 1
    paths = np.zeros((idx.shape[0], depth, stride), dtype=np.uint8)
    lens = np.zeros((idx.shape[0], depth), dtype=np.uint64)
    d = SZ()
    rc = mz.lib().mzk_merkle_open_batch(tree._h, _ptr(idx), SZ(idx.shape[0]), _ptr(paths), SZ(stride), _ptr(lens), ctypes.byref(d))
    assert rc == 0, mz.lib().mzk_last_error().decode()
    assert d.value == depth
    return paths, lens


def check_openings(mz, tree, fid, arr, nd, idx, neg=None, what=""):
    stride = STRIDE[fid]
    want, want_lens = mm.expected_open(fid, arr, nd, idx, stride, neg)
    got, got_lens = open_batch(mz, tree, idx, stride)
    assert np.array_equal(got, want), "%s: %s" % (what, mm.first_mismatch(got, want, idx))
    assert np.array_equal(got_lens, want_lens), what


def commit_dev(mz, fid, arr):
    """mzk_merkle_commit_field_dev: the one-shot commit of a device-resident codeword (the root comes back through the mailbox)"""
    import torch
    d = torch.from_numpy(arr.view(np.int64).reshape(-1).copy()).to(torch.device("cuda", 0))
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    root, ln = (ctypes.c_uint8 * 48)(), SZ()
    rc = mz.lib().mzk_merkle_commit_field_dev(fid, ctypes.c_void_p(d.data_ptr()), SZ(arr.shape[0]), root, SZ(48), ctypes.byref(ln), st)
    assert rc == 0, mz.lib().mzk_last_error().decode()
    torch.cuda.synchronize()
    return bytes(root[:ln.value])


# ---- single trees: one of each step list, both sides of LEAF_PAIR_MAX (2^16 | 2^17 leaves) and LEVEL_PAIR_MAX ----------------------------
@pytest.mark.parametrize("fid", [mm.FR, mm.M128], ids=["Fr", "M128"])
@pytest.mark.parametrize("lg", [11, 12, 13, 14, 15, 16, 17])
def test_every_digest_and_leaf_of_a_single_tree(mz, fid, lg):
    n = 1 << lg
    arr, _, nd = model(fid, n)
    want_root = mm.root(nd)
    assert mz.merkle_commit_field(fid, arr) == want_root
    assert commit_dev(mz, fid, arr) == want_root
    t = mz.MerkleTree(fid, arr)
    try:
        assert t.root() == want_root
        check_openings(mz, t, fid, arr, nd, mm.covering_indices(n), what="%s 2^%d" % (NAMES[fid], lg))
        vals, sg = t.leaves(np.arange(n), with_sign=True)
        assert np.array_equal(vals, arr) and not sg.any()
    finally:
        t.close()


@pytest.mark.parametrize("fid", [mm.FR, mm.M128], ids=["Fr", "M128"])
@pytest.mark.parametrize("lg", [18, 19])
def test_chained_level_kernels_of_a_large_tree(mz, fid, lg):
    """a second and a third k_merkle_level in a row: the root, and the even-index paths at a stride of 64 indices"""
    n = 1 << lg
    arr, _, nd = model(fid, n)
    want_root = mm.root(nd)
    assert mz.merkle_commit_field(fid, arr) == want_root
    assert commit_dev(mz, fid, arr) == want_root
    t = mz.MerkleTree(fid, arr)
    try:
        assert t.root() == want_root
        check_openings(mz, t, fid, arr, nd, np.arange(0, n, 64, dtype=np.uint64), what="%s 2^%d" % (NAMES[fid], lg))
    finally:
        t.close()


# ---- signed leaves: once for each leaf kernel taking `neg` ---------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [mm.FR, mm.M128], ids=["Fr", "M128"])
@pytest.mark.parametrize("lg", [14, 17])
def test_signed_tree(mz, fid, lg):
    n = 1 << lg
    mag, neg, nd = model(fid, n, signed=True)
    t = mz.MerkleTree(fid, mag, negative=neg)
    try:
        assert t.root() == mm.root(nd)
        check_openings(mz, t, fid, mag, nd, mm.covering_indices(n), neg=neg, what="signed %s 2^%d" % (NAMES[fid], lg))
    finally:
        t.close()


# ---- the Goldilocks ids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [mm.M64, mm.M64X3], ids=["M64", "M64X3"])
@pytest.mark.parametrize("lg", [13, 14, 17])
def test_goldilocks_tree(mz, fid, lg):
    n = 1 << lg
    arr, _, nd = model(fid, n)
    assert mz.merkle_commit_field(fid, arr) == mm.root(nd)
    t = mz.MerkleTree(fid, arr)
    try:
        t.stride = 64
        assert t.root() == mm.root(nd)
        check_openings(mz, t, fid, arr, nd, mm.covering_indices(n), what="%s 2^%d" % (NAMES[fid], lg))
    finally:
        t.close()


# ---- batches: every ending (step lists: test_hostcheck_merkle_plan.py) -----------------------------------------------------------------
BATCHES = [(2048, 3),       # lp, multi<2>, level_pair, tail of 384 nodes (not a power of two)
           (8192, 5),       # lp, multi<3>, multi<2>, level_pair, tail of 320
           (16, 512),       # lp, multi<3>: ends on its third level, no tail
           (16, 511),       # lp, multi<2>, level_pair: no tail
           (32, 300),       # lp, multi<3>, level_pair: no tail
           (32768, 3),      # one lane per pair, level, multi<3>, multi<2>, level_pair, tail of 384
           (4, 600)]        # lp, level_pair: more trees than the tail holds nodes


@pytest.mark.parametrize("fid", [mm.FR, mm.M128], ids=["Fr", "M128"])
@pytest.mark.parametrize("per,trees", BATCHES)
def test_every_root_of_a_batch(mz, fid, per, trees):
    import torch
    n = per * trees
    arr, _, nd = model(fid, n, trees=trees)
    want = nd[nd.shape[0] - trees:].tobytes()
    roots = mz.merkle_commit_field_batch(fid, arr.reshape(trees, per, mm.LIMBS[fid]))
    assert len(roots) == trees
    bad = [k for k in range(trees) if roots[k] != want[32 * k:32 * k + 32]]
    assert not bad, "trees %s (of %d)" % (bad[:8], len(bad))
    # the device-pointer form, on a stream of the caller's
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d = torch.from_numpy(arr.view(np.int64).reshape(-1).copy()).to(torch.device("cuda", 0), non_blocking=False)
    out = np.zeros(32 * trees, dtype=np.uint8)
    rc = mz.lib().mzk_merkle_commit_field_batch_dev(fid, ctypes.c_void_p(d.data_ptr()), SZ(per), SZ(trees), _ptr(out), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, mz.lib().mzk_last_error().decode()
    s.synchronize()
    assert out.tobytes() == want


# ---- FRI rounds with the trees kept: the round trees share one block, d_nodes advances by len - 1 digests per round ----------------------
@pytest.mark.parametrize("fid,lg,rounds,signed", [(mm.M128, 17, 8, False), (mm.FR, 15, 5, False), (mm.M128, 14, 4, True)],
                         ids=["M128-2^17", "Fr-2^15", "M128-2^14-signed"])
def test_fri_rounds_with_the_trees_kept(mz, fid, lg, rounds, signed):
    n, p = 1 << lg, mm.MOD[fid]
    ofid = orc.M128 if fid == mm.M128 else orc.FR
    if signed:
        cw, neg = mm.signed_vector(fid, n, 77)
    else:
        cw, neg = mm.leaf_vector(fid, n, 77), None
    omega, offset = orc.root_of(ofid, lg), (orc.M128_GEN if fid == mm.M128 else 5)

    def challenge(rnd, last, root):
        return None if last else int.from_bytes(hashlib.sha3_256(root + bytes([rnd])).digest(), "little") % p

    cws, roots, trees = mz.fri_commit(fid, cw, omega, offset, rounds, challenge, negative=neg, keep_trees=True)
    try:
        # nothing of the round trees lives in workspace: another tree of another size, and the plain loop (which reuses the workspace's
        # digest buffer every round), run between their build and their openings
        other_arr, _, other_nd = model(fid, 1 << 13)
        other = mz.MerkleTree(fid, other_arr)
        assert other.root() == mm.root(other_nd)
        other.close()
        cws0, roots0 = mz.fri_commit(fid, cw, omega, offset, rounds, challenge, negative=neg)
        assert roots0 == roots and all(np.array_equal(a, b) for a, b in zip(cws, cws0))
        if signed:
            canon = orc.to_limbs([(p - v) % p if s else v for v, s in zip(orc.from_limbs(cw), neg)], mm.LIMBS[fid])
            assert np.array_equal(cws[0], canon)
        else:
            assert np.array_equal(cws[0], cw)
        om, of = omega, offset
        for r in range(rounds):
            m = n >> r
            if r:
                alpha = challenge(r - 1, False, roots[r - 1])
                assert np.array_equal(cws[r], orc.fri_fold_ref(ofid, cws[r - 1], alpha, of, om)), r
                om, of = om * om % p, of * of % p
            leaves_arr, leaves_neg = (cw, neg) if (r == 0 and signed) else (cws[r], None)
            blob, off = mm.leaves(fid, leaves_arr, leaves_neg)
            nd = mm.nodes(blob, off)
            assert roots[r] == mm.root(nd), r
            assert trees[r].root() == mm.root(nd), r
            check_openings(mz, trees[r], fid, leaves_arr, nd, mm.covering_indices(m), neg=leaves_neg, what="round %d" % r)
    finally:
        for t in trees:
            if t is not None:
                t.close()


# ---- byte leaves: the block edges of k_merkle_leaf_pairs_bytes ---------------------------------------------------------------------------
def test_byte_leaves_at_the_block_edges(mz):
    """pair messages of 0, 1, 135, 136, 137, 271, 272 and 273 bytes (the rate is 136: the padded final block begins at those edges), each
    length on even and on odd pairs, split between the two leaves at a random point; root and single openings against hashlib"""
    n = 1 << 12
    rng = np.random.default_rng(12)
    edges = [0, 1, 135, 136, 137, 271, 272, 273]
    lv = []
    for i in range(n // 2):
        total = edges[(i % 16) // 2]            # pairs 2j and 2j + 1 of every sixteen: length j
        cut = int(rng.integers(0, total + 1))
        msg = rng.integers(0, 256, size=total, dtype=np.uint8).tobytes()
        lv += [msg[:cut], msg[cut:]]
    assert {(len(lv[2 * i]) + len(lv[2 * i + 1]), i % 2) for i in range(n // 2)} == {(e, par) for e in edges for par in (0, 1)}
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(x) for x in lv])
    nd = mm.nodes(np.frombuffer(b"".join(lv), dtype=np.uint8), off)
    t = mz.MerkleTree(leaves=lv)
    try:
        assert t.root() == mm.root(nd)
        for i in list(range(16)) + list(range(n // 2 - 16, n // 2)):
            for idx in (2 * i, 2 * i + 1):
                want = [lv[idx ^ 1]] + [nd[mm.level_start(n, l) + ((idx >> l) ^ 1)].tobytes() for l in range(1, 12)]
                assert t.open(idx) == want, idx
    finally:
        t.close()
