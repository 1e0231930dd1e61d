"""The G2 kernels (myzkp_amd/csrc/mzk_g2.hip) at every shape of their sum: k_g2_sum folds n records with a stride of 128 and then a 7-level
tree in LDS, so equal and opposite operands meet in it only where the input puts them there -- these inputs do.  Expectations come from
discrete logs: every point is d_i G2 from a pool of 16, the wanted value is (sum k_i d_i mod r) G2, one oracle multiplication per case
(orc.g2_mul, which tests/test_oracle_g2.py pins).  Also here: the device entry point on a caller's stream, the host form's refusals, and
kzg_setup_g2 past one workgroup of k_g2_powers."""
import ctypes, random
import numpy as np
import pytest
import orc
from orc import P_FR as R, P_FQ as Q, G2_GEN as G2, G2_INF

pytestmark = pytest.mark.gpu

E_RANGE = -6


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


@pytest.fixture(scope="module")
def pool():
    """16 (d, d G2): the only points of this file, so that every expectation is one multiplication of the generator"""
    rnd = random.Random(0x6732)
    ds = [rnd.randrange(1, R) for _ in range(16)]
    return [(d, orc.g2_mul(G2, d)) for d in ds]


def neg(P):
    return (P[0], ((-P[1][0]) % Q, (-P[1][1]) % Q))


class Batch:
    """records (k, d, point): d the discrete log of the point as given (None: infinity), k the scalar as passed"""
    def __init__(self, pool):
        self.pool, self.recs = pool, []

    def add(self, k, i, negate=False):
        if i is None:
            self.recs.append((k, 0, G2_INF))
        else:
            d, P = self.pool[i % 16]
            self.recs.append((k, (R - d) if negate else d, neg(P) if negate else P))
        return self

    def negated(self, t):
        k, d, P = self.recs[t]
        self.recs.append((k, (R - d) % R, P if P == G2_INF else neg(P)))

    def arrays(self):
        return orc.to_limbs([k for k, _, _ in self.recs], 4), orc.g2_to_arr([P for _, _, P in self.recs])

    def want(self):
        return orc.g2_mul(G2, sum((k % R) * d for k, d, _ in self.recs) % R)

    def check(self, mz):
        s, p = self.arrays()
        got = mz.msm_g2(s, p)
        assert got == self.want(), (len(self.recs), got)
        return got


def random_batch(pool, n, seed):
    rnd = random.Random(seed)
    b = Batch(pool)
    for _ in range(n):
        b.add(rnd.randrange(R), rnd.randrange(16), rnd.randrange(2) == 1)
    return b


def test_oracle_of_zero_is_infinity():
    assert orc.g2_mul(G2, 0) == G2_INF


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300])
def test_msm_at_every_fold_boundary(mz, pool, n):
    random_batch(pool, n, n).check(mz)


@pytest.mark.parametrize("n", [129, 257])
def test_msm_against_the_literal_oracle_sum(mz, pool, n):
    s, p = random_batch(pool, n, 1000 + n).arrays()
    assert mz.msm_g2(s, p) == orc.g2_msm_ref(s, p)


@pytest.mark.parametrize("n", [128, 256])
def test_all_records_the_same(mz, pool, n):
    """every tree level doubles identical representatives (and at 256 the strided fold does first)"""
    b = Batch(pool)
    for _ in range(n):
        b.add(0x1234567890abcdef1234567890abcdef % R, 3)
    assert b.check(mz) != G2_INF


@pytest.mark.parametrize("n", [128, 256])
def test_one_group_element_from_different_pairs(mz, pool, n):
    """k_i d_i constant mod r with different d_i: every level doubles, the two representatives differ (P and R of x2_add are
    multiples of p with non-zero limbs); records i and i + 64, i + 128 use different points"""
    c = 0x2545f4914f6cdd1d2545f4914f6cdd1d2545f4914f6cdd1d % R
    b = Batch(pool)
    for i in range(n):
        j = (i + i // 16) % 16
        ngt = (i // 7) % 2 == 1
        d = pool[j][0]
        b.add((c if not ngt else R - c) * pow(d, -1, R) % R, j, ngt)
    assert all(k * d % R == c for k, d, _ in b.recs)
    assert len({(k, d) for k, d, _ in b.recs[:16]}) == 16 and b.recs[0][:2] != b.recs[64][:2]
    assert b.check(mz) == orc.g2_mul(G2, n * c % R)


@pytest.mark.parametrize("n", [128, 256])
def test_level_one_cancels_everywhere(mz, pool, n):
    """record[i + 64] = -record[i]: all of level one cancels, the rest of the tree is infinity + infinity"""
    rnd = random.Random(n)
    b = Batch(pool)
    for blk in range(n // 128):
        for i in range(64):
            b.add(rnd.randrange(1, R), rnd.randrange(16))
        for i in range(64):
            b.negated(128 * blk + i)
    assert b.check(mz) == G2_INF


@pytest.mark.parametrize("n", [128, 256])
def test_cancellation_only_at_the_last_level(mz, pool, n):
    """record[2 j + 1] = -record[2 j], otherwise distinct: lane 0 sums the even records, lane 1 their negatives, they meet at off = 1"""
    rnd = random.Random(n + 1)
    b = Batch(pool)
    ks = rnd.sample(range(1, 1 << 60), n // 2)
    for j in range(n // 2):
        b.add(ks[j] * 0x9e3779b97f4a7c15f39cc0605cedc835 % R, j)
        b.negated(2 * j)
    assert len({(k, d) for k, d, _ in b.recs[::2]}) == n // 2
    assert b.check(mz) == G2_INF


def test_strided_fold_doubles(mz, pool):
    """n = 384, record[t + 128] = record[t]: the strided fold of every lane meets its own record again, then a random one"""
    b = random_batch(pool, 128, 77)
    b.recs += b.recs[:128]
    b.recs += random_batch(pool, 128, 78).recs
    b.check(mz)


def test_strided_fold_cancels(mz, pool):
    """n = 384, record[t + 128] = -record[t], record[t + 256] random: cancellation in the strided fold, then infinity + point"""
    b = random_batch(pool, 128, 79)
    for t in range(128):
        b.negated(t)
    b.recs += random_batch(pool, 128, 80).recs
    assert len(b.recs) == 384
    b.check(mz)


@pytest.mark.parametrize("n", [128, 256])
def test_infinity_points_and_zero_scalars_in_every_fourth_slot(mz, pool, n):
    rnd = random.Random(n + 2)
    b = Batch(pool)
    for i in range(n):
        if i % 4 == 1:
            b.add(rnd.randrange(R), None)
        elif i % 4 == 3:
            b.add(0, rnd.randrange(16))
        else:
            b.add(rnd.randrange(R), rnd.randrange(16))
    assert b.check(mz) != G2_INF


def test_all_infinity_input_and_one_infinity(mz, pool):
    b = Batch(pool)
    for i in range(128):
        b.add(i + 1, None)
    assert b.check(mz) == G2_INF
    assert Batch(pool).add(5, None).check(mz) == G2_INF


def test_scalars_are_canonicalised(mz, pool):
    """the kernel reduces k itself (k_g2_pair_mul); the wanted value uses k mod r"""
    ks = [0, 1, 2, R - 1, R, R + 1, 2 * R, 5 * R + 7, 1 << 255, (1 << 256) - 1]
    assert max(ks) < 1 << 256
    b = Batch(pool)
    for i, k in enumerate(ks):
        b.add(k, i)
    assert [int(x) for x in orc.from_limbs(b.arrays()[0])] == ks          # they reach the library as given
    assert b.check(mz) != G2_INF
    for i, k in enumerate(ks):                                          # and one by one
        Batch(pool).add(k, i).check(mz)


# ---- the device entry point ---------------------------------------------------------------------------------------------------------
GUARD = 64


def _dev(mz):
    import torch
    return torch, mz.lib(), torch.device("cuda", 0)


PAD = 0x5a5a5a5a5a5a5a5a


def _upload(torch, dev, a):
    """the array xor PAD on the device (default stream): what the side stream's kernel turns into the real input"""
    return torch.from_numpy((a.reshape(-1) ^ np.uint64(PAD)).view(np.int64)).to(dev)


def _enqueue(torch, L, side, ms, mp, n, out):
    """the inputs are WRITTEN BY A KERNEL of the side stream (an xor over the masked upload), the call is enqueued behind it with no
    synchronisation; returns the tensors that have to stay alive until the caller has synchronised"""
    with torch.cuda.stream(side):
        d_s, d_p = ms ^ PAD, mp ^ PAD
        rc = L.mzk_msm_g2_bn254_dev(ctypes.c_void_p(d_s.data_ptr()), ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(n),
                                    ctypes.c_void_p(out.data_ptr() + GUARD), ctypes.c_void_p(side.cuda_stream))
    assert rc == 0, L.mzk_last_error()
    return d_s, d_p


def _result(out):
    b = out.cpu().numpy()
    assert (b[:GUARD] == 0xa5).all() and (b[GUARD + 128:] == 0xa5).all(), "guard bytes overwritten"
    return b[GUARD:GUARD + 128].copy()


def test_dev_entry_point_on_a_side_stream(mz, pool):
    torch, L, dev = _dev(mz)
    side = torch.cuda.Stream(device=dev)
    b200, b3 = random_batch(pool, 200, 200), random_batch(pool, 3, 3)
    (s200, p200), (s3, p3) = b200.arrays(), b3.arrays()
    outs = [torch.full((GUARD + 128 + GUARD,), 0xa5, dtype=torch.uint8, device=dev) for _ in range(3)]
    up = [_upload(torch, dev, a) for a in (s200, p200, s3, p3)]
    torch.cuda.synchronize()
    with torch.cuda.stream(side):          # something for the stream to be busy with while the calls are enqueued
        busy = torch.empty(1 << 26, dtype=torch.int64, device=dev).fill_(3)
    # n = 200 then n = 3 on the same stream with nothing in between: their record scratch is shared
    keep = [busy, _enqueue(torch, L, side, up[0], up[1], 200, outs[0]), _enqueue(torch, L, side, up[2], up[3], 3, outs[1])]
    # n = 0 over a pre-filled output: 128 zero bytes, guards intact (null inputs are fine for an empty sum)
    with torch.cuda.stream(side):
        assert L.mzk_msm_g2_bn254_dev(None, None, ctypes.c_size_t(0), ctypes.c_void_p(outs[2].data_ptr() + GUARD), ctypes.c_void_p(side.cuda_stream)) == 0
    side.synchronize()
    del keep
    r200, r3, r0 = _result(outs[0]), _result(outs[1]), _result(outs[2])
    assert not r0.any()
    for r, b, (s, p) in ((r200, b200, (s200, p200)), (r3, b3, (s3, p3))):
        got = orc.arr_to_g2(r.view(np.uint64))[0]
        assert got == b.want()
        assert got == mz.msm_g2(s, p)                                    # the host form
    assert L.mzk_msm_g2_bn254_dev(None, None, ctypes.c_size_t(1), ctypes.c_void_p(outs[2].data_ptr() + GUARD), ctypes.c_void_p(side.cuda_stream)) == -1
    assert L.mzk_msm_g2_bn254_dev(None, None, ctypes.c_size_t(0), None, ctypes.c_void_p(side.cuda_stream)) == -1


# ---- refusals of the host form ------------------------------------------------------------------------------------------------------
def test_host_form_refuses_a_coordinate_equal_to_q(mz, pool):
    """in each of the four positions: MZK_E_RANGE, the message names the index; the next call is right"""
    b = random_batch(pool, 5, 55)
    s, p = b.arrays()
    for rec, pos in ((0, 0), (1, 1), (3, 2), (4, 3)):
        bad = p.copy()
        bad[rec, 4 * pos:4 * pos + 4] = orc.to_limbs([Q], 4).reshape(-1)
        with pytest.raises(mz.MzkError) as e:
            mz.msm_g2(s, bad)
        assert e.value.code == E_RANGE
        assert "coordinate %d " % (4 * rec + pos) in e.value.message + " ", e.value.message
        assert mz.msm_g2(s, p) == b.want()


# ---- kzg_setup_g2 -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g7():
    return orc.g2_mul(G2, 7)


@pytest.mark.parametrize("max_d", [0, 1, 63, 64, 65, 130])
def test_setup_powers_past_one_workgroup(mz, g7, max_d):
    alpha = random.Random(max_d).randrange(2, R)
    got = mz.kzg_setup_g2(alpha, max_d, g7)
    assert got.shape == (max_d + 1, 16)
    assert np.array_equal(got, orc.kzg_setup_g2_ref(alpha, max_d, g7))


def test_setup_powers_of_special_alphas(mz, g7):
    g, ng, inf = orc.g2_to_arr([g7])[0], orc.g2_to_arr([neg(g7)])[0], orc.g2_to_arr([G2_INF])[0]
    assert np.array_equal(mz.kzg_setup_g2(1, 130, g7), np.tile(g, (131, 1)))                       # alpha = 1: every power is g
    got = mz.kzg_setup_g2(R - 1, 130, g7)                                                          # alpha = -1: g, -g, g, ...
    assert np.array_equal(got[0::2], np.tile(g, (66, 1))) and np.array_equal(got[1::2], np.tile(ng, (65, 1)))
    got = mz.kzg_setup_g2(0, 130, g7)                                                              # alpha = 0: g, then infinities
    assert np.array_equal(got[0], g) and np.array_equal(got[1:], np.tile(inf, (130, 1)))
    got = mz.kzg_setup_g2(random.Random(9).randrange(2, R), 130, G2_INF)                           # the all-zero generator
    assert got.shape == (131, 16) and not got.any()
    with pytest.raises(mz.MzkError) as e:                                                          # alpha = r is not canonical
        mz.kzg_setup_g2(R, 3, g7)
    assert e.value.code == E_RANGE
    assert np.array_equal(mz.kzg_setup_g2(1, 2, g7), np.tile(g, (3, 1)))                           # and the next call is right
