"""The Goldilocks ids on the GPU -- MZK_FIELD_M64 (p = 2^64 - 2^32 + 1) and MZK_FIELD_M64X3 (its cubic extension, x^3 - x + 1) --
through the existing entry points: transforms, coset LDE, FRI fold, Merkle trees and the FRI commit loop of the reference's
test_fri_efield (zkstark/fri.rs:546-594), each against tests/goldilocks_model.py.  Every output coefficient is also checked to be
canonical (< p)."""
import ctypes, random
import numpy as np
import pytest
import fri_prove_model as fpm
import goldilocks_model as gm

pytestmark = pytest.mark.gpu

P = gm.P
E_ARG, E_LENGTH, E_ROOT_ORDER = -1, -5, -3
FIELDS = [gm.M64, gm.M64X3]
IDS = [F.name for F in FIELDS]
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def arr(F, elems):
    return np.array([F.words(e) for e in elems], dtype=np.uint64).reshape(len(elems), F.limbs)


def elems(F, a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, F.limbs)
    assert (a < np.uint64(P)).all(), "non-canonical coefficient in an output"
    return [F.from_words(row) for row in a.tolist()]


def scalar(F, e):
    """an element as the int the Python wrappers take: c0 + c1 2^64 + c2 2^128"""
    return sum(int(w) << (64 * i) for i, w in enumerate(F.words(e)))


def rand_elems(F, seed, n):
    rng = random.Random(seed)
    out = [F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for _ in range(n)]
    if n >= 2:                           # 0 and p - 1 among the data
        out[n // 2] = F.zero
        out[n - 1] = F.from_words([P - 1] * F.limbs)
    return out


_DATA, _REF = {}, {}


def data(F, n, row=0):
    k = (F.fid, n, row)
    if k not in _DATA:
        _DATA[k] = rand_elems(F, 1000 * F.fid + 17 * n + row, n)
    return _DATA[k]


def ref_ntt(F, n, row=0, inverse=False):
    """the model's literal recursion over data(F, n, row): computed once per module"""
    k = (F.fid, n, row, inverse)
    if k not in _REF:
        w = gm.root_of_unity(F, n.bit_length() - 1)
        _REF[k] = (gm.intt if inverse else gm.ntt)(F, w, data(F, n, row))
    return _REF[k]


# ---- transforms --------------------------------------------------------------------------------------------------------------
def test_root_of_unity(mz):
    for F in FIELDS:
        for lg in (0, 1, 10, 31, 32):
            assert mz.root_of_unity(F.fid, lg) == scalar(F, gm.root_of_unity(F, lg))
        with pytest.raises(mz.MzkError) as e:
            mz.root_of_unity(F.fid, 33)
        assert e.value.code == E_ARG


@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("lg", range(0, 15))
def test_ntt_and_intt_against_the_literal_recursion(mz, F, lg):
    """n = 2^0 .. 2^14: one pass up to 2^12, two passes above"""
    n = 1 << lg
    w = scalar(F, gm.root_of_unity(F, lg))
    v = arr(F, data(F, n))
    assert elems(F, mz.ntt(F.fid, w, v)) == ref_ntt(F, n)
    assert elems(F, mz.intt(F.fid, w, v)) == ref_ntt(F, n, inverse=True)


# the first size of every pass count above 2^14 that fits 2^24: three passes from 2^17 on (four only from 2^25)
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("lg", [17])
def test_large_transform_round_trip_sparse_outputs_and_linearity(mz, F, lg):
    n = 1 << lg
    rng = random.Random(lg + F.fid)
    wF = gm.root_of_unity(F, lg)
    w = scalar(F, wF)
    dense = np.array([rng.randrange(P) for _ in range(n * F.limbs)], dtype=np.uint64).reshape(n, F.limbs)
    dense[0], dense[n - 1] = 0, P - 1
    t_dense = mz.ntt(F.fid, w, dense)
    assert (t_dense < np.uint64(P)).all()
    assert np.array_equal(mz.intt(F.fid, w, t_dense), dense)
    pos = sorted(set([0, n - 1] + rng.sample(range(1, n - 1), 62)))
    sp = {j: F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for j in pos}
    sparse = np.zeros((n, F.limbs), dtype=np.uint64)
    for j, e in sp.items():
        sparse[j] = F.words(e)
    t_sparse = mz.ntt(F.fid, w, sparse)
    assert (t_sparse < np.uint64(P)).all()
    ks = sorted(set([0, n - 1] + rng.sample(range(1, n - 1), 4094)))
    w0 = F.words(wF)[0]
    for k in ks:                         # the direct sum: out[k] = sum_j x[j] w^(j k), w a base value
        acc = [0] * F.limbs
        for j, e in sp.items():
            t = pow(w0, j * k % n, P)
            for c, x in enumerate(F.words(e)):
                acc[c] += x * t
        assert [a % P for a in acc] == t_sparse[k].tolist(), k
    both = ((dense.astype(object) + sparse.astype(object)) % P).astype(np.uint64)
    t_both = mz.ntt(F.fid, w, both)
    assert (t_both < np.uint64(P)).all()
    assert np.array_equal(((t_both.astype(object) - t_dense.astype(object)) % P).astype(np.uint64), t_sparse)


@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n", [1 << 8, 1 << 13])
@pytest.mark.parametrize("batch", [1, 2, 5])
def test_batched_transforms(mz, F, n, batch):
    w = scalar(F, gm.root_of_unity(F, n.bit_length() - 1))
    rows = np.stack([arr(F, data(F, n, r)) for r in range(batch)])
    got = mz.ntt_batch(F.fid, w, rows)
    for r in range(batch):
        assert elems(F, got[r]) == ref_ntt(F, n, r)
    back = mz.ntt_batch(F.fid, w, got, inverse=True)
    assert (back < np.uint64(P)).all() and np.array_equal(back, rows)


def test_transform_argument_errors(mz):
    F = gm.M64X3
    v = arr(F, data(F, 8))
    with pytest.raises(mz.MzkError) as e:                     # a root outside the base field has no 2-power order
        mz.ntt(F.fid, scalar(F, (1, 1, 0)), v)
    assert e.value.code == E_ROOT_ORDER
    with pytest.raises(mz.MzkError) as e:
        mz.ntt(gm.M64.fid, scalar(gm.M64, gm.root_of_unity(gm.M64, 4)), arr(gm.M64, data(gm.M64, 8)))
    assert e.value.code == E_ROOT_ORDER


# ---- coset LDE ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n_coef,order", [(1 << 8, 1 << 12), (96, 1 << 10), (1 << 6, 1 << 6), (1 << 13, 1 << 13), (1, 1)])
def test_coset_lde_against_the_model(mz, F, n_coef, order):
    """one pass with padding, an odd coefficient count, n_coef == order, and the two-pass transform (the pre-scale in its first pass)"""
    rng = random.Random(order + n_coef)
    coef = rand_elems(F, 31 * order + n_coef, n_coef)
    g = gm.root_of_unity(F, order.bit_length() - 1)
    for off in (7, rng.randrange(2, P)):
        want = gm.fast_coset_evaluate(F, coef, F.from_int(off), g, order)
        assert elems(F, mz.coset_lde(F.fid, arr(F, coef), off, scalar(F, g), order)) == want
    got = mz.coset_lde_batch(F.fid, np.stack([arr(F, coef), arr(F, coef[::-1])]), 7, scalar(F, g), order)
    assert elems(F, got[0]) == gm.fast_coset_evaluate(F, coef, F.from_int(7), g, order)
    assert elems(F, got[1]) == gm.fast_coset_evaluate(F, coef[::-1], F.from_int(7), g, order)


def test_coset_lde_argument_errors(mz):
    F = gm.M64X3
    g = scalar(F, gm.root_of_unity(F, 4))
    c = arr(F, data(F, 8))
    with pytest.raises(mz.MzkError) as e:
        mz.coset_lde(F.fid, c, scalar(F, (7, 1, 0)), g, 16)
    assert e.value.code == E_ARG
    for fid, cc in ((F.fid, arr(F, data(F, 32))), (gm.M64.fid, arr(gm.M64, data(gm.M64, 32)))):
        with pytest.raises(mz.MzkError) as e:
            mz.coset_lde(fid, cc, 7, g & ((1 << 64) - 1), 16)
        assert e.value.code == E_LENGTH


# ---- fold ---------------------------------------------------------------------------------------------------------------------
# a lane folds outputs t, t + 256, ...; a workgroup 1024 consecutive ones: n / 2 = 256 | 257 and 1024 | 1025 straddle both boundaries
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n", [2, 4, 1 << 6, 1 << 10, 512, 514, 2048, 2050])
def test_fold_against_the_model(mz, F, n):
    rng = random.Random(n)
    lg = max((n - 1).bit_length(), 1)
    omega, offset = gm.root_of_unity(F, lg), F.from_int(rng.randrange(2, P))
    cw = rand_elems(F, 5 * n + 1, n)
    alphas = [F.zero, F.from_int(rng.randrange(1, P)), F.from_words([rng.randrange(1, P) for _ in range(F.limbs)])]
    for alpha in alphas:
        got = mz.fri_fold(F.fid, arr(F, cw), scalar(F, alpha), scalar(F, offset), scalar(F, omega))
        assert elems(F, got) == gm.fold(F, cw, alpha, offset, omega), (n, alpha)


# ---- Merkle ---------------------------------------------------------------------------------------------------------------------
def _commit(leaves):                       # merkle.rs:15-25
    if len(leaves) == 1:
        return leaves[0]
    mid = len(leaves) // 2
    return fpm._h(_commit(leaves[:mid]) + _commit(leaves[mid:]))


def _open(i, leaves):                      # merkle.rs:27-46
    if len(leaves) == 2:
        return [leaves[1 - i]]
    mid = len(leaves) // 2
    if i < mid:
        return _open(i, leaves[:mid]) + [_commit(leaves[mid:])]
    return _open(i - mid, leaves[mid:]) + [_commit(leaves[:mid])]


def _leaf_cases(F, n):
    """elements covering every leaf length: zero, one / two / three significant coefficients, zero coefficients below a non-zero one,
    one- and two-digit coefficients"""
    cs = [(1 << 32) - 1, 1 << 32, P - 1]
    if F.limbs == 1:
        base = [0] + cs + [1, 5]
    else:
        base = [(0, 0, 0)] + [t for c in cs for t in ((c, 0, 0), (0, c, 0), (0, 0, c))] + [(P - 1, P - 1, P - 1), (5, 0, 0), (1 << 32, 7, P - 1)]
    rng = random.Random(n)
    out = [base[i % len(base)] for i in range(n)]
    if n > 2 * len(base):
        out[len(base):] = [rng.choice(base) if rng.random() < 0.5 else F.from_words([rng.randrange(P) for _ in range(F.limbs)]) for _ in range(n - len(base))]
    return out


@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n", [1, 2, 3, 8, 1 << 10])
def test_merkle_tree_root_paths_and_leaves(mz, F, n):
    """n = 3 is ragged: the tree is kept over byte leaves, as for Fr -- paths open where Merkle::open terminates (not the one-leaf half
    of the three-leaf slice) and mzk_merkle_leaves serves field-element trees only"""
    es = _leaf_cases(F, n)
    leaves = [F.leaf(e) for e in es]
    if n == 1 << 10:
        assert {len(l) for l in leaves} >= ({8, 21, 25, 30, 39, 43, 59} if F.limbs == 3 else {9, 13, 17})
    want_root = _commit(leaves)
    assert mz.merkle_commit_field(F.fid, arr(F, es)) == want_root
    t = mz.MerkleTree(F.fid, arr(F, es))
    try:
        t.stride = 64
        assert t.root() == want_root
        if n == 3:
            for i in (1, 2):
                assert t.open(i) == _open(i, leaves), i
        elif n >= 2:
            levels = fpm.merkle_levels(leaves)
            want = [fpm.merkle_open(i, leaves, levels) for i in range(n)]
            assert want[n - 1] == _open(n - 1, leaves)
            assert t.open_many(list(range(n))) == want
            for i in (0, n - 1):
                assert t.open(i) == want[i]
        if n != 3:
            vals, neg = t.leaves(list(range(n)), with_sign=True)
            assert elems(F, vals) == es and not neg.any()
    finally:
        t.close()


def test_a_short_path_stride_fails_only_where_a_leaf_does_not_fit(mz):
    F = gm.M64X3
    es = [(5, 0, 0), (5, 0, 0), (P - 1, P - 1, P - 1), (0, 0, 0)]
    t = mz.MerkleTree(F.fid, arr(F, es))
    try:
        t.stride = 48
        assert t.open(0)[0] == F.leaf(es[1])             # a 21-byte sibling fits
        with pytest.raises(mz.MzkError) as e:            # the 59-byte sibling of leaf 3 does not
            t.open(3)
        assert e.value.code == E_LENGTH
    finally:
        t.close()


# ---- the test_fri_efield flow ---------------------------------------------------------------------------------------------------
def _gpu_prove(mz, F, cw, omega, offset, expansion, tests):
    """FRI::prove with the commit loop, the openings and the revealed values on the GPU and the model's transcript as the callback"""
    n = len(cw)
    rounds = fpm.num_rounds(n, expansion, tests)
    stream = []

    def challenge(rnd, last, root):
        stream.append([root])
        return None if last else scalar(F, gm.sample(F, fpm.fiat_shamir(stream)))

    none, roots, trees = mz.fri_commit(F.fid, arr(F, cw), scalar(F, omega), scalar(F, offset), rounds, challenge, keep_trees=True, codewords=False)
    try:
        assert none is None
        m = n >> (rounds - 1)
        last = elems(F, trees[-1].leaves(list(range(m))))
        stream.append([F.leaf(v) for v in last])
        top = fpm.sample_indices(fpm.fiat_shamir(stream), n // 2, m, tests)
        lists, per_round, indices = [[] for _ in range(rounds)], [], list(top)
        for i in range(rounds - 1):
            half = (n >> i) // 2
            indices = [idx % half for idx in indices]
            a, b = list(indices), [idx + half for idx in indices]
            per_round.append((a, b))
            lists[i] += a + b
            lists[i + 1] += a
        paths = mz.merkle_open_multi(trees, lists)
        values = [elems(F, trees[r].leaves(lists[r])) if lists[r] else [] for r in range(rounds)]
        layers, used = [], [0] * rounds
        for i, (a, b) in enumerate(per_round):
            s, k = used[i], len(a)
            va, pa = values[i][s:s + k], paths[i][s:s + k]
            vb, pb = values[i][s + k:s + 2 * k], paths[i][s + k:s + 2 * k]
            used[i] += 2 * k
            s = used[i + 1]
            vc, pc = values[i + 1][s:s + k], paths[i + 1][s:s + k]
            used[i + 1] += k
            layers.append({"a": (va, pa), "b": (vb, pb), "c": (vc, pc)})
        return {"top_level_indices": top, "last_codeword": last, "merkle_roots": roots, "revealed_layers": layers}
    finally:
        for t in trees:
            if t is not None:
                t.close()


@pytest.fixture(scope="module")
def efield_case():
    F = gm.M64X3
    omega, offset = gm.root_of_unity(F, 10), F.from_int(7)
    coef = [F.from_int(i) for i in range(64)]
    return omega, offset, coef, gm.ntt(F, omega, coef + [F.zero] * (1024 - 64))


def _same_proof(got, want):
    for k in ("top_level_indices", "last_codeword", "merkle_roots", "revealed_layers"):
        assert got[k] == want[k], k


def test_fri_efield_flow_matches_the_model_and_verifies(mz, efield_case):
    F = gm.M64X3
    omega, offset, coef, cw = efield_case
    got = _gpu_prove(mz, F, cw, omega, offset, 16, 17)
    _same_proof(got, gm.prove(F, cw, omega, offset, 16, 17))
    points = []
    assert gm.verify(F, got, omega, offset, 1024, 16, 17, points)
    for x, y in points:
        assert gm.poly_eval(F, coef, gm.fpow(F, omega, x)) == y


def test_fri_efield_flow_rejects_the_corrupted_codeword(mz, efield_case):
    F = gm.M64X3
    omega, offset, coef, cw = efield_case
    bad = [F.one] * 21 + cw[21:]
    got = _gpu_prove(mz, F, bad, omega, offset, 16, 17)
    _same_proof(got, gm.prove(F, bad, omega, offset, 16, 17))
    assert not gm.verify(F, got, omega, offset, 1024, 16, 17, [])


def test_fri_flow_over_the_base_field_matches_the_model(mz):
    F = gm.M64
    omega, offset = gm.root_of_unity(F, 10), 7
    cw = rand_elems(F, 99, 1024)
    _same_proof(_gpu_prove(mz, F, cw, omega, offset, 16, 17), gm.prove(F, cw, omega, offset, 16, 17))


def test_fri_commit_argument_errors(mz):
    for F in FIELDS:
        cw = arr(F, data(F, 8))
        w = scalar(F, gm.root_of_unity(F, 3))
        with pytest.raises(mz.MzkError) as e:             # signs are not represented for these fields
            mz.fri_commit(F.fid, cw, w, 7, 2, lambda *a: 1, negative=np.zeros(8, dtype=np.uint8), keep_trees=True)
        assert e.value.code == E_ARG
    F = gm.M64X3
    with pytest.raises(mz.MzkError) as e:                 # a one-element round: its leaf (up to 59 bytes) has no room in a root slot
        mz.fri_commit(F.fid, arr(F, data(F, 4)), scalar(F, gm.root_of_unity(F, 2)), 7, 3, lambda *a: 1)
    assert e.value.code == E_LENGTH
    cws, roots = mz.fri_commit(gm.M64.fid, arr(gm.M64, data(gm.M64, 4)), gm.root_of_unity(gm.M64, 2), 7, 3, lambda *a: 1)
    assert roots[2] == gm.M64.leaf(int(cws[2][0, 0])) and len(cws[2]) == 1
    with pytest.raises(mz.MzkError) as e:                 # offset outside the base field
        mz.fri_commit(F.fid, arr(F, data(F, 8)), scalar(F, gm.root_of_unity(F, 3)), scalar(F, (7, 0, 1)), 2, lambda *a: 1)
    assert e.value.code == E_ARG


# ---- everything else keeps refusing the new ids -----------------------------------------------------------------------------------
def test_other_entry_points_refuse_the_goldilocks_ids(mz):
    L = mz.lib()
    one = np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.uint64)
    out = np.zeros(64, dtype=np.uint64)
    scratch = np.zeros(256, dtype=np.uint64)
    zeros = np.zeros(64, dtype=np.uint64)
    exps = np.array([1, 0], dtype=np.uint32)
    off01 = np.array([0, 1, 2], dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    H, O = p(one), p(out)
    plan_head = (SZ(4), SZ(1), SZ(1), SZ(1), SZ(1))
    calls = [("mzk_fri_prove", (H, None, SZ(4), H, H, SZ(2), SZ(1), O, SZ(512)), "fri_prove"),
             ("mzk_stark_plan", plan_head + (p(exps), p(off01), SZ(1), p(zeros), p(zeros), SZ(1), p(scratch)), "stark_plan"),
             ("mzk_fast_multiply", (H, SZ(1), H, SZ(1), H, SZ(2), O, p(scratch)), "fast_multiply"),
             ("mzk_merkle_commit_field_signed", (H, p(zeros), SZ(1), O, SZ(48), p(scratch)), "merkle"),
             ("mzk_merkle_commit_field_batch", (H, SZ(2), SZ(1), O), "merkle")]
    for fn, rest, who in calls:
        for fid in (gm.FIELD_M64, gm.FIELD_M64X3):
            rc = getattr(L, fn)(ctypes.c_int(fid), *rest)
            assert rc == E_ARG and L.mzk_last_error().decode() == "%s: bad field id %d" % (who, fid), (fn, fid, rc, L.mzk_last_error())
