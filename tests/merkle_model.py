"""Merkle::commit / Merkle::open (algebra/merkle.rs:15-46) over field-element leaves, restated on numpy byte matrices and
hashlib.sha3_256 -- no code shared with the C oracle (oracle/mzk_oracle_merkle.c), which tests/test_merkle_model.py pins it against.
fri_prove_model.merkle_levels is the literal form; this one is laid out for whole trees of 2^11 .. 2^19 leaves:

  leaves(fid, arr, neg)            the leaf bytes of every element as one blob + offsets
  nodes(blob, off, stop)           every digest, level 1 first, in the order the library keeps them (n - stop digests of 32 bytes)
  expected_open(...)               what mzk_merkle_open_batch writes for an index array, as one array (fancy indexing, no per-path objects)
  covering_indices(n)              indices whose paths hold every digest of every level (and, up to 2^14 leaves, reveal every leaf)
  leaf_vector(fid, n, seed)        elements in which every combination of the two digit counts of a leaf pair occurs
  signed_vector(fid, n, seed)      the same with Sign::Minus on a third of the elements

Field ids are the library's: 0 = Fr, 1 = M128, 3 = M64 (Goldilocks), 4 = M64X3 (its cubic extension).  No GPU, no library."""
import hashlib
import numpy as np

FR, M128, M64, M64X3 = 0, 1, 3, 4
P_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P_M128 = 270497897142230380135924736767050121217
P_M64 = (1 << 64) - (1 << 32) + 1
LIMBS = {FR: 4, M128: 2, M64: 1, M64X3: 3}
MOD = {FR: P_FR, M128: P_M128, M64: P_M64, M64X3: P_M64}
# an element is COMPS big integers of DIGITS 32-bit digits each, every one below the modulus
COMPS = {FR: 1, M128: 1, M64: 1, M64X3: 3}
DIGITS = {FR: 8, M128: 4, M64: 2, M64X3: 2}
# Digit-count classes of an element, one count per component.  Fr / M128: every count 0 .. DIGITS.  The Goldilocks ids: the leaf-length
# classes of _leaf_cases in test_gpu_goldilocks.py (zero; one / two / three significant coefficients, zero coefficients below a
# non-zero one, one- and two-digit coefficients) -- tests/test_merkle_model.py checks this list against that function.
CLASSES = {
    FR: [(k,) for k in range(9)],
    M128: [(k,) for k in range(5)],
    M64: [(0,), (1,), (2,)],
    M64X3: [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 2), (2, 1, 2)],
}


def combos(fid):
    """C: the number of (class of the even element, class of the odd element) combinations of a leaf pair: 81, 25, 9, 81"""
    return len(CLASSES[fid]) ** 2


# ---- leaf bytes -------------------------------------------------------------------------------------------------------------------
def _digits(col):
    """(n, limbs) uint64 -> (n, 2 limbs) 32-bit digits, least significant first, as uint64"""
    col = np.ascontiguousarray(col, dtype="<u8")
    return col.view("<u4").reshape(col.shape[0], -1).astype(np.uint64)


def _digit_count(dig):
    nz = dig != 0
    return np.where(nz.any(axis=1), dig.shape[1] - np.argmax(nz[:, ::-1], axis=1), 0)


def _bigint_part(dig, neg=None):
    """bincode(BigInt): Sign as i8 (NoSign 0 for zero, else Plus 1 / Minus 0xff), u64 digit count, the significant u32 digits.
    Returns the zero-padded byte matrix (n, 9 + 4 D) and the lengths."""
    n, D = dig.shape
    k = _digit_count(dig)
    mat = np.zeros((n, 9 + 4 * D), dtype=np.uint8)
    sign = np.where(neg.astype(bool), 0xff, 1) if neg is not None else 1
    mat[:, 0] = np.where(k == 0, 0, sign)
    mat[:, 1] = k
    mat[:, 9:] = dig.astype("<u4").view(np.uint8).reshape(n, 4 * D)
    return mat, 9 + 4 * k


def leaf_matrix(fid, arr, neg=None):
    """the leaf bytes of every element: (zero-padded byte matrix (n, L), validity mask (n, L)); the bytes of leaf i are mat[i][mask[i]]"""
    arr = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, LIMBS[fid])
    n = arr.shape[0]
    if fid in (FR, M128, M64):
        mat, lens = _bigint_part(_digits(arr), neg)
        return mat, np.arange(mat.shape[1])[None, :] < lens[:, None]
    assert neg is None      # bincode(ExtendedFieldElement): u64 count of coefficients after trimming trailing zeros, then their leaves
    kc = np.where(arr[:, 2] != 0, 3, np.where(arr[:, 1] != 0, 2, np.where(arr[:, 0] != 0, 1, 0)))
    head = np.zeros((n, 8), dtype=np.uint8)
    head[:, 0] = kc
    mats, masks = [head], [np.ones((n, 8), dtype=bool)]
    for j in range(3):
        m, lens = _bigint_part(_digits(arr[:, j:j + 1]))
        mats.append(m)
        masks.append(np.arange(m.shape[1])[None, :] < np.where(j < kc, lens, 0)[:, None])
    return np.hstack(mats), np.hstack(masks)


def leaves(fid, arr, neg=None):
    """(blob, off): leaf i is blob[off[i]:off[i + 1]]"""
    mat, mask = leaf_matrix(fid, arr, neg)
    off = np.zeros(mat.shape[0] + 1, dtype=np.int64)
    off[1:] = np.cumsum(mask.sum(axis=1))
    return mat[mask], off


def leaf_list(blob, off):
    raw, o = blob.tobytes(), off.tolist()
    return [raw[o[i]:o[i + 1]] for i in range(len(o) - 1)]


# ---- levels -----------------------------------------------------------------------------------------------------------------------
def nodes(blob, off, stop=1):
    """Every digest of the tree over the leaves (blob, off), level 1 first: (n - stop, 32) uint8.  stop > 1: the leaves are those of
    `stop` trees of one power-of-two size back to back, hashed down to their roots, which are the last `stop` rows."""
    h = hashlib.sha3_256
    raw, po = blob.tobytes(), off[::2].tolist()
    lv = b"".join([h(raw[po[i]:po[i + 1]]).digest() for i in range(len(po) - 1)])
    out = [lv]
    while len(lv) // 32 > stop:
        lv = b"".join([h(lv[o:o + 64]).digest() for o in range(0, len(lv), 64)])
        out.append(lv)
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 32)


def level_start(n, l):
    """first row of level l >= 1 (n >> l digests) in nodes()"""
    return n - (n >> (l - 1))


def root(nd):
    return nd[-1].tobytes()


def covering_indices(n):
    """The even indices put node (i >> l) ^ 1 of every level l into some path -- every digest below the root -- and reveal every odd
    leaf; up to 2^14 leaves the odd indices join them, so that every leaf is revealed too."""
    return np.arange(0, n, 2 if n > 1 << 14 else 1, dtype=np.uint64)


def expected_open(fid, arr, nd, idx, stride, neg=None):
    """What mzk_merkle_open_batch leaves in a zeroed buffer for the indices idx: paths (count, depth, stride) uint8 -- entry 0 the
    sibling leaf, entry l the sibling digest of level l -- and path_lens (count, depth) uint64."""
    mat, mask = leaf_matrix(fid, arr, neg)
    n = mat.shape[0]
    depth = n.bit_length() - 1
    padded = np.where(mask, mat, 0).astype(np.uint8)      # (the significant bytes of a leaf are a prefix only for one-component leaves)
    lens = mask.sum(axis=1)
    if not (mask[:, 1:] <= mask[:, :-1]).all():            # M64X3: compact every row
        order = np.argsort(~mask, axis=1, kind="stable")
        padded = np.where(np.arange(mat.shape[1])[None, :] < lens[:, None], np.take_along_axis(mat, order, axis=1), 0).astype(np.uint8)
    width = int(lens.max())
    assert width <= stride
    idx = np.asarray(idx, dtype=np.int64)
    paths = np.zeros((idx.shape[0], depth, stride), dtype=np.uint8)
    plens = np.full((idx.shape[0], depth), 32, dtype=np.uint64)
    paths[:, 0, :width] = padded[idx ^ 1, :width]
    plens[:, 0] = lens[idx ^ 1]
    for l in range(1, depth):
        paths[:, l, :32] = nd[level_start(n, l) + ((idx >> l) ^ 1)]
    return paths, plens


def first_mismatch(got, want, idx):
    """where two path arrays first differ, in the tree's terms: 'leaf j' or 'level l node j' (None when equal)"""
    bad = np.argwhere((got != want).any(axis=2))
    if bad.shape[0] == 0:
        return None
    q, l = int(bad[0][0]), int(bad[0][1])
    i = int(idx[q])
    what = "leaf %d" % (i ^ 1) if l == 0 else "level %d node %d" % (l, (i >> l) ^ 1)
    return "%s (path %d of index %d; %d of %d entries differ)" % (what, q, i, bad.shape[0], got.shape[0] * got.shape[1])


# ---- leaf vectors -------------------------------------------------------------------------------------------------------------------
def _top_bound(fid):
    """exclusive bound on the most significant digit of a full-length component that keeps it below the modulus whatever the other
    digits are: the modulus' own top digit"""
    return MOD[fid] >> (32 * (DIGITS[fid] - 1))


def pair_combination(fid, pairs):
    """(special, combo) per pair.  With C = combos(fid) and j the distance of pair i from the nearer end of the vector (j = i in the
    first half, pairs - 1 - i in the second): the pair is special where (j // C) % 2 == 0, and its combination is
    (j + j // (2 C)) % C -- the issue's i % C, rotated by one from run to run and mirrored in the second half."""
    C = combos(fid)
    i = np.arange(pairs)
    j = np.where(2 * i < pairs, i, pairs - 1 - i)
    return (j // C) % 2 == 0, (j + j // (2 * C)) % C


def leaf_vector(fid, n, seed):
    """(n, limbs) uint64 canonical elements.  A special pair (pair_combination) has digit-count combination c: its even element class
    CLASSES[fid][c // K], its odd element class CLASSES[fid][c % K], K classes.  A component of digit count k has a non-zero digit
    k - 1, nothing above it and random digits below, a quarter of them zero.  Every other element is uniform.  Runs of C special pairs
    alternate with runs of uniform pairs; the rotation moves a combination by one pair from run to run and the mirror image has the
    other parity, so every combination meets both parities of the pair index and moving positions in the 64- and 128-pair workgroups
    of the leaf kernels, and the first and the last C pairs of a vector hold all of them: the first and last 128-pair workgroup (a
    64-pair workgroup cannot hold 81).  With (a, b) comes (b, a), so every class meets both lanes of a pair."""
    rng = np.random.default_rng(seed)
    comps, D, K, C = COMPS[fid], DIGITS[fid], len(CLASSES[fid]), combos(fid)
    top = _top_bound(fid)
    dig = rng.integers(0, 1 << 32, size=(n, comps, D), dtype=np.uint64)
    dig[:, :, D - 1] = rng.integers(0, top, size=(n, comps), dtype=np.uint64)
    e = np.arange(n)
    pair, par = e // 2, e % 2
    special, combo = (a[pair] for a in pair_combination(fid, (n + 1) // 2))
    cls = np.where(par == 0, combo // K, combo % K)
    ks = np.array(CLASSES[fid], dtype=np.int64)[cls]                   # (n, comps) digit counts
    col = np.arange(D)[None, None, :]
    sp = special[:, None, None]
    thin = rng.random((n, comps, D)) < 0.25
    dig[sp & thin & (col < ks[:, :, None] - 1)] = 0
    dig[sp & (col >= ks[:, :, None])] = 0
    tops = np.where(ks == D, rng.integers(1, top, size=(n, comps), dtype=np.uint64), rng.integers(1, 1 << 32, size=(n, comps), dtype=np.uint64))
    at_top = sp & (col == ks[:, :, None] - 1)
    dig[at_top] = np.broadcast_to(tops[:, :, None], dig.shape)[at_top]
    d = dig.reshape(n, comps * D)
    return np.ascontiguousarray(d[:, 0::2] | (d[:, 1::2] << np.uint64(32)))


def signed_vector(fid, n, seed):
    """(magnitudes, negative): leaf_vector with Sign::Minus on every third element -- among them elements of magnitude 0 (pairs 0, 3,
    6 start with one), which still serialise as NoSign: BigInt has no negative zero"""
    assert fid in (FR, M128)
    mag = leaf_vector(fid, n, seed)
    neg = (np.arange(n) % 3 == 0).astype(np.uint8)
    return mag, neg


def to_ints(fid, arr):
    """elements as Python ints (Fr / M128 / M64) or tuples of ints (M64X3)"""
    a = np.asarray(arr, dtype=np.uint64).reshape(-1, LIMBS[fid]).tolist()
    if fid == M64X3:
        return [tuple(r) for r in a]
    return [sum(w << (64 * j) for j, w in enumerate(r)) for r in a]
