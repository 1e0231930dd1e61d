"""mzk_fast_coset_divide_batch_dev: many numerators in HBM over one denominator.  Every row must equal mzk_fast_coset_divide of that
row (the host-buffer form) and the oracle's literal restatement of ntt.rs:271-330, bit for bit: rows of different squared-down order
in one call, the degree < 8 branch, untrimmed rows, a denominator with a zero on the coset (inverse(0) = 0), every error code."""
import ctypes, random
import numpy as np
import pytest
import orc
from orc import FR, M128

pytestmark = pytest.mark.gpu
E_ARG, E_NOT_POW2, E_ROOT_ORDER, E_ROOT_PRIM, E_LENGTH, E_RANGE = -1, -2, -3, -4, -5, -6


@pytest.fixture(scope="module")
def env():
    import torch
    import myzkp_amd as mz
    mz.init(0)
    return torch, mz, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def to_dev(env, arr):
    torch, _, dev, _ = env
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64).reshape(-1).copy()).to(dev)


def batch(env, fid, rows, rhs, offset, root, order, lhs_stride=None, out_stride=None, lens=None):
    """rows / rhs: limb arrays; returns the quotient rows as limb arrays (and checks the zero tail of every out row)"""
    torch, mz, dev, st = env
    nl = orc.LIMBS[fid]
    lens = lens if lens is not None else [r.shape[0] for r in rows]
    lhs_stride = lhs_stride if lhs_stride is not None else max([r.shape[0] for r in rows] + [1])
    out_stride = out_stride if out_stride is not None else lhs_stride
    flat = np.full((max(len(rows), 1) * lhs_stride, nl), 0x0123456789ABCDEF, dtype=np.uint64)      # what lies beyond a row's length is not read
    for i, r in enumerate(rows):
        flat[i * lhs_stride:i * lhs_stride + r.shape[0]] = r
    d_l, d_r = to_dev(env, flat), to_dev(env, rhs if rhs.shape[0] else np.zeros((1, nl), dtype=np.uint64))
    d_o = torch.full((max(len(rows), 1) * out_stride * nl,), -1, dtype=torch.int64, device=dev)
    out_lens = mz.fast_coset_divide_batch_dev(fid, d_l.data_ptr(), lhs_stride, lens, d_r.data_ptr(), rhs.shape[0], offset, root, order,
                                              d_o.data_ptr(), out_stride, st)
    torch.cuda.synchronize()
    assert torch.equal(d_l.cpu(), torch.from_numpy(flat.view(np.int64).reshape(-1))), "the numerators were written"
    out = d_o.cpu().numpy().view(np.uint64).reshape(-1, nl)
    res = []
    for i in range(len(rows)):
        row = out[i * out_stride:(i + 1) * out_stride]
        assert not row[out_lens[i]:].any(), "row %d is not zero behind its quotient" % i
        res.append(row[:out_lens[i]].copy())
    return res


def check_rows(env, fid, rows, rhs, offset, root, order, **kw):
    mz = env[1]
    got = batch(env, fid, rows, rhs, offset, root, order, **kw)
    for i, r in enumerate(rows):
        single = mz.fast_coset_divide(fid, r, rhs, offset, root, order)
        rc, want = orc.fast_coset_divide_ref(fid, r, rhs, offset, root, order)
        assert rc == 0
        assert np.array_equal(got[i], single), "row %d differs from mzk_fast_coset_divide" % i
        assert np.array_equal(got[i], want), "row %d differs from the oracle" % i
    return got


def _mul(p, a, b):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return out


@pytest.mark.parametrize("fid", [M128, FR])
def test_rows_of_different_order_and_the_small_branch(env, fid):
    """numerators of 5 .. 1500 coefficients over one denominator of 4: orders 16 .. 2048 and the degree < 8 branch in one call;
    inexact divisions (the recipe's own result), trailing zeros on some rows"""
    nl = orc.LIMBS[fid]
    rhs = orc.synth_vector(fid, 31, 4)
    zeros = lambda k: np.zeros((k, nl), dtype=np.uint64)
    sizes = [5, 8, 9, 16, 17, 100, 100, 127, 128, 129, 700, 1500, 6, 1024]
    rows = [orc.synth_vector(fid, 900 + i, n) for i, n in enumerate(sizes)]
    rows[3] = np.concatenate([rows[3], zeros(5)])            # untrimmed: the order comes from the trimmed degree
    rows[10] = np.concatenate([rows[10], zeros(400)])        # 700 coefficients in 1100: order 1024, not 2048
    rows[12] = np.concatenate([rows[12], zeros(30)])         # degree 5 behind 30 zeros: still the long-division branch
    offset = orc.M128_GEN if fid == M128 else 7
    got = check_rows(env, fid, rows, rhs, offset, orc.root_of(fid, 11), 1 << 11)
    assert [g.shape[0] for g in got] == [n - 4 + 1 for n in sizes]
    check_rows(env, fid, rows, rhs, offset, orc.root_of(fid, 11), 1 << 11, lhs_stride=1600, out_stride=1497)


@pytest.mark.parametrize("fid", [M128, FR])
def test_exact_quotients_of_transition_shape(env, fid):
    """what FastStark::prove does: several multiples of one zerofier, all of one order, divided in one call: the cofactors come back"""
    p, nl = orc.MOD[fid], orc.LIMBS[fid]
    rnd = random.Random(4 + fid)
    z = [rnd.randrange(p) for _ in range(27)] + [1]
    qs = [[rnd.randrange(p) for _ in range(n)] + [rnd.randrange(1, p)] for n in (78, 78, 70, 60)]
    rows = [orc.to_limbs(_mul(p, q, z), nl) for q in qs]
    offset = orc.M128_GEN if fid == M128 else 5
    got = check_rows(env, fid, rows, orc.to_limbs(z + [0, 0], nl), offset, orc.root_of(fid, 7), 128)
    assert [orc.from_limbs(g) for g in got] == qs


def test_large_rows(env):
    """numerators of 2^16, 2^15 + 3 and 2^15 coefficients over a denominator of 2^12: the first two share the order 2^16, the third runs at
    2^15; against the host form"""
    mz = env[1]
    rhs = orc.synth_vector(M128, 77, 1 << 12)
    rows = [orc.synth_vector(M128, 78, 1 << 16), orc.synth_vector(M128, 79, (1 << 15) + 3), orc.synth_vector(M128, 80, 1 << 15)]
    root, order = orc.root_of(M128, 18), 1 << 18
    got = batch(env, M128, rows, rhs, orc.M128_GEN, root, order)
    for g, r in zip(got, rows):
        assert np.array_equal(g, mz.fast_coset_divide(M128, r, rhs, orc.M128_GEN, root, order))


def test_divisor_vanishing_on_the_coset(env):
    """rhs = X - offset has a root ON the evaluation coset: that codeword entry divides by zero -> el * 0 (field.rs:209-232)"""
    p = orc.MOD[M128]
    offset = orc.M128_GEN
    rows = [orc.synth_vector(M128, 5, 40), orc.synth_vector(M128, 6, 64), orc.synth_vector(M128, 7, 33)]
    rhs = orc.to_limbs([(p - offset) % p, 1], 2)
    check_rows(env, M128, rows, rhs, offset, orc.root_of(M128, 6), 64)


def test_error_codes(env):
    torch, mz, dev, st = env
    a = orc.to_limbs(list(range(1, 12)), 2)
    b = orc.to_limbs([1, 2, 3], 2)
    z = orc.to_limbs([0, 0, 0], 2)
    root = orc.root_of(M128, 6)

    def code(rows, rhs, offset, rt, order, **kw):
        with pytest.raises(mz.MzkError) as e:
            batch(env, M128, rows, rhs, offset, rt, order, **kw)
        return e.value.code

    assert code([a, a], z, 3, root, 64) == E_ARG                             # rhs zero
    assert code([a, b], b, 3, root, 64) == E_LENGTH                          # rhs.degree() >= lhs.degree() in the second row
    assert code([a, z], b, 3, root, 64) == E_LENGTH                          # a zero numerator has degree -1
    assert code([a], b, 3, root, 32) == E_ROOT_ORDER
    assert code([a], b, 3, root, 128) == E_ROOT_PRIM
    big = orc.synth_vector(M128, 1, 100)
    assert code([a, big], b, 3, root, 64) == E_NOT_POW2 == orc.fast_coset_divide_ref(M128, big, b, 3, root, 64)[0]
    big = orc.synth_vector(M128, 1, 128)
    assert code([big], b, 3, root, 64) == E_ROOT_ORDER == orc.fast_coset_divide_ref(M128, big, b, 3, root, 64)[0]
    assert code([a], b, orc.MOD[M128], root, 64) == E_RANGE                  # offset == p
    assert code([a], b, 3, root, 64, lhs_stride=16, lens=[17]) == E_LENGTH   # a length beyond the stride
    assert code([a], b, 3, root, 64, out_stride=8) == E_LENGTH               # quotient of 9 coefficients
    d = torch.zeros(64, dtype=torch.int64, device=dev)
    sz, vp = ctypes.c_size_t, ctypes.c_void_p
    three, rt = orc.to_limbs([3], 2), orc.to_limbs([root], 2)
    for bad in (2, 7, -1):                                                   # Fq and unknown fields (the wrapper itself has no limbs for them)
        rc = mz.lib().mzk_fast_coset_divide_batch_dev(bad, vp(d.data_ptr()), sz(11), (sz * 1)(11), sz(1), vp(d.data_ptr()), sz(3), vp(three.ctypes.data),
                                                      vp(rt.ctypes.data), sz(64), vp(d.data_ptr()), sz(11), (sz * 1)(), vp(st))
        assert rc == E_ARG
    for args in ((0, 11, [11], d.data_ptr(), 3, 3, root, 64, d.data_ptr(), 11), (d.data_ptr(), 11, [11], 0, 3, 3, root, 64, d.data_ptr(), 11),
                 (d.data_ptr(), 11, [11], d.data_ptr(), 3, 3, root, 64, 0, 11)):
        with pytest.raises(mz.MzkError) as e:
            mz.fast_coset_divide_batch_dev(M128, *args, st)
        assert e.value.code == E_ARG
    assert mz.fast_coset_divide_batch_dev(M128, 0, 0, [], 0, 0, 3, root, 64, 0, 0, st) == []     # no rows: nothing to do
    assert len(batch(env, M128, [a], b, 3, root, 64)[0]) == 9                # and the context still works


def test_workspace_is_shared_cleanly_with_other_calls(env):
    """the call between unrelated ones (a transform, evaluate_symbolic, the host-buffer division, the boundary division): their
    results are unchanged by it and its own by them; releasing the workspace afterwards succeeds and the call still works"""
    torch, mz, dev, st = env
    rhs = orc.synth_vector(M128, 41, 5)
    rows = [orc.synth_vector(M128, 42 + i, n) for i, n in enumerate((300, 300, 90, 7))]     # 7: the long-division branch
    root, order = orc.root_of(M128, 10), 1 << 10
    v = orc.synth_vector(M128, 50, 1 << 12)
    cons = [[(3, (1, 2)), (5, (0, 1))]]
    point = [orc.synth_vector(M128, 51, 40), orc.synth_vector(M128, 52, 33)]

    def others():
        return (mz.ntt(M128, orc.root_of(M128, 12), v).tobytes(), [r.tobytes() for r in mz.mpoly_compose(M128, cons, point)],
                mz.fast_coset_divide(M128, rows[0], rhs, orc.M128_GEN, root, order).tobytes(),
                [q.tobytes() for q in mz.poly_div_roots(M128, [rows[1], rows[2]], [[3, 4, 5], [6]])])

    before = others()
    mine = [g.tobytes() for g in batch(env, M128, rows, rhs, orc.M128_GEN, root, order)]
    assert others() == before
    assert [g.tobytes() for g in batch(env, M128, rows, rhs, orc.M128_GEN, root, order)] == mine
    assert mine[0] == before[2]
    mz.trim_workspace()
    assert [g.tobytes() for g in batch(env, M128, rows, rhs, orc.M128_GEN, root, order)] == mine
    assert others() == before
