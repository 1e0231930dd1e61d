"""Every split of log2 n into passes that mzk_gl.hip chooses between 2^15 and 2^25, M64 and M64X3.

  lg     15     16     17       18       19       20       21       22       23       24       25
  split  (7,8)  (8,8)  (5,6,6)  (6,6,6)  (6,6,7)  (6,7,7)  (7,7,7)  (7,7,8)  (7,8,8)  (8,8,8)  (6,6,6,7)

Up to 2^18 the transforms, batches and the coset LDE (the pre-scale in the first strided pass) are compared element for element with
the numpy model of tests/goldilocks_model.py.  Above, every size is tied to the one below it, which runs another split, by one
radix-2 step done on the host: with h = n / 2 and w of order n,

    ntt_n(x)[0::2] = ntt_h(x[:h] + x[h:])               ntt_n(x)[1::2] = ntt_h((x[:h] - x[h:]) * w^j)

(root w^2 on the right), and the same with w^-1 and a factor 1/2 for the inverse.  The chain ends at 2^18, which is checked densely.
2^25 is the only size whose inter-pass twiddles read the third tier of the power tables (gl_pow_lookup, E >> 24).  An M64X3 transform
with its base-field root is the M64 transform of each coefficient column, which is how one model serves both ids; the ladder for
M64X3 stops at 2^22, the index arithmetic being the same for both.  Every output is also checked to be canonical (< p)."""
import random
import numpy as np
import pytest
import goldilocks_model as gm

pytestmark = pytest.mark.gpu

P = gm.P
FIELDS = [gm.M64, gm.M64X3]
IDS = [F.name for F in FIELDS]
HALF = (P + 1) // 2


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    yield m
    _DATA.clear()
    _REF.clear()
    _RUNG.clear()


def root(lg):
    return gm.root_of_unity(gm.M64, lg)


def canonical(a):
    assert (a < np.uint64(P)).all(), "non-canonical coefficient in an output"
    return a


def rand(seed, n, cols):
    """uniform elements with 0 first and p - 1 last"""
    x = np.random.default_rng(seed).integers(0, P, size=(n, cols), dtype=np.uint64)
    x[0], x[-1] = 0, P - 1
    return x


# ---- 2^15 .. 2^18 against the numpy model ---------------------------------------------------------------------------------------
# One (n, 3) array per size and row: M64X3 takes all of it, M64 its first column, and one model transform serves both.
_DATA, _REF = {}, {}


def data3(lg, row=0):
    k = (lg, row)
    if k not in _DATA:
        _DATA[k] = rand(100 * lg + row, 1 << lg, 3)
        _DATA[k].setflags(write=False)
    return _DATA[k]


def ref3(lg, row=0, inverse=False):
    k = (lg, row, inverse)
    if k not in _REF:
        _REF[k] = (gm.np_intt if inverse else gm.np_ntt)(data3(lg, row), root(lg))
        _REF[k].setflags(write=False)
    return _REF[k]


@pytest.mark.parametrize("lg", range(15, 19))
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_forward_and_inverse_against_the_model(mz, F, lg):
    x = data3(lg)[:, :F.limbs]
    assert np.array_equal(canonical(mz.ntt(F.fid, root(lg), x)), ref3(lg)[:, :F.limbs])
    assert np.array_equal(canonical(mz.intt(F.fid, root(lg), x)), ref3(lg, inverse=True)[:, :F.limbs])


@pytest.mark.parametrize("lg", [15, 17])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_batch_against_the_model(mz, F, lg):
    rows = np.stack([data3(lg, r)[:, :F.limbs] for r in range(3)])
    got = canonical(mz.ntt_batch(F.fid, root(lg), rows))
    for r in range(3):
        assert np.array_equal(got[r], ref3(lg, r)[:, :F.limbs]), r
    assert np.array_equal(canonical(mz.ntt_batch(F.fid, root(lg), got, inverse=True)), rows)


def lde_ref(lg, ncoef, off):
    """fast_coset_evaluate (ntt.rs:254-269) of the first ncoef rows of data3(lg): times offset^i, padded, transformed"""
    k = ("lde", lg, ncoef, off)
    if k not in _REF:
        padded = np.zeros((1 << lg, 3), dtype=np.uint64)
        padded[:ncoef] = gm.np_mul(data3(lg)[:ncoef], gm.np_powers(off, ncoef)[:, None])
        _REF[k] = gm.np_ntt(padded, root(lg))
    return _REF[k]


@pytest.mark.parametrize("whole", [False, True], ids=["quarter+3", "whole"])
@pytest.mark.parametrize("lg", [15, 17, 18])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_coset_lde_against_the_model(mz, F, lg, whole):
    """order / 4 + 3 coefficients (an odd count: the zero padding starts inside a tile) and `order` of them (none)"""
    order = 1 << lg
    ncoef = order if whole else order // 4 + 3
    coef = data3(lg)[:ncoef, :F.limbs]
    for off in (7, random.Random(lg + ncoef).randrange(2, P)):
        got = canonical(mz.coset_lde(F.fid, coef, off, root(lg), order))
        assert np.array_equal(got, lde_ref(lg, ncoef, off)[:, :F.limbs]), off


# ---- the ladder above 2^18 ----------------------------------------------------------------------------------------------------------
LADDER = [(gm.M64, lg) for lg in range(19, 26)] + [(gm.M64X3, lg) for lg in range(19, 23)]
LADDER_IDS = ["%s-%d" % (F.name, lg) for F, lg in LADDER]
_RUNG = {}


def rung(F, lg):
    """x of 2^lg elements, s = x[:h] + x[h:], d = x[:h] - x[h:] and w^j, j < h: what the forward and the inverse step share (only
    the latest rung is kept: 2^25 is 256 MiB)"""
    k = (F.fid, lg)
    if k not in _RUNG:
        _RUNG.clear()
        h = 1 << (lg - 1)
        w = root(lg)
        assert w * w % P == root(lg - 1)
        x = rand(7000 + 10 * lg + F.fid, 2 * h, F.limbs)
        _RUNG[k] = x, gm.np_add(x[:h], x[h:]), gm.np_sub(x[:h], x[h:]), gm.np_powers(w, h)
    return _RUNG[k]


@pytest.mark.parametrize("F,lg", LADDER, ids=LADDER_IDS)
def test_forward_ladder(mz, F, lg):
    x, s, d, pw = rung(F, lg)
    w = root(lg)
    X = canonical(mz.ntt(F.fid, w, x))
    assert np.array_equal(X[0::2], canonical(mz.ntt(F.fid, w * w % P, s)))
    assert np.array_equal(X[1::2], canonical(mz.ntt(F.fid, w * w % P, gm.np_mul(d, pw[:, None]))))


@pytest.mark.parametrize("F,lg", LADDER, ids=LADDER_IDS)
def test_inverse_ladder(mz, F, lg):
    """intt_n(x)[0::2] = 1/2 intt_h(s), intt_n(x)[1::2] = 1/2 intt_h(d * w^-j); w^h = -1, so w^-j = -w^(h - j) for 0 < j < h"""
    x, s, d, pw = rung(F, lg)
    w, h = root(lg), 1 << (lg - 1)
    ipw = np.empty_like(pw)
    ipw[0] = 1
    ipw[1:] = np.uint64(P) - pw[:0:-1]
    for j in (1, h // 2, h - 1):
        assert int(ipw[j]) == pow(w, P - 1 - j, P)
    Y = canonical(mz.intt(F.fid, w, x))
    half = np.uint64(HALF)
    assert np.array_equal(Y[0::2], gm.np_mul(canonical(mz.intt(F.fid, w * w % P, s)), half))
    assert np.array_equal(Y[1::2], gm.np_mul(canonical(mz.intt(F.fid, w * w % P, gm.np_mul(d, ipw[:, None]))), half))


@pytest.mark.parametrize("lg", [19, 21])
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
def test_batch_equals_the_single_calls_of_the_ladder(mz, F, lg):
    rows = np.stack([rand(9000 + 10 * lg + r, 1 << lg, F.limbs) for r in range(2)])
    got = canonical(mz.ntt_batch(F.fid, root(lg), rows))
    for r in range(2):
        assert np.array_equal(got[r], mz.ntt(F.fid, root(lg), rows[r])), r
    assert np.array_equal(canonical(mz.ntt_batch(F.fid, root(lg), got, inverse=True)), rows)
