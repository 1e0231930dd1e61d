"""Division by a product of linear factors on the GPU (mzk_poly_div_roots, mzk_poly_div_roots_dev): the boundary quotients of
FastStark::prove, fast_stark.rs:217-224.  The library divides root by root (one synthetic division per root, remainder dropped);
the reference does Polynomial long division by the expanded zerofier (polynomial.rs:371-405), and that is what every result is
compared with here, in Python integers: both fields, both sides of the one-workgroup limit (2^13 coefficients), ragged root counts,
repeated and extreme roots, exact and inexact divisions, untrimmed inputs, empty quotients, every documented error code."""
import ctypes, random
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
FR, M128 = 0, 1
PRIME = {FR: 21888242871839275222246405745257275088548364400416034343698204186575808495617, M128: 270497897142230380135924736767050121217}
NL = {FR: 4, M128: 2}
E_ARG, E_LENGTH, E_RANGE = -1, -5, -6
LENGTHS = [1, 2, 31, 32, 33, 1 << 13, (1 << 13) + 1, (1 << 16) + 5, 1 << 20]
ROOT_COUNTS = [0, 1, 2, 5]


@pytest.fixture(scope="module")
def env():
    import torch
    import myzkp_amd as mz
    mz.init(0)
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    return torch, mz, dev, st


def limbs(fid, vals):
    a = np.zeros((len(vals), NL[fid]), dtype=np.uint64)
    for j in range(NL[fid]):
        a[:, j] = np.array([(int(v) >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for v in vals], dtype=np.uint64) if len(vals) else 0
    return a


def ints(a):
    a = np.asarray(a, dtype=np.uint64)
    a = a.reshape(-1, a.shape[-1])
    acc = np.zeros(a.shape[0], dtype=object)
    for j in range(a.shape[1]):
        acc = acc + (a[:, j].astype(object) << (64 * j))
    return [int(v) for v in acc]


def trim(a):
    n = len(a)
    while n and a[n - 1] == 0:
        n -= 1
    return a[:n]


def zerofier(roots, p):
    z = [1]
    for r in roots:                                      # z * (X - r)
        z = [((z[i - 1] if i else 0) - r * (z[i] if i < len(z) else 0)) % p for i in range(len(z) + 1)]
    return z


def long_div(a, b, p):
    """the quotient of div_rem_ref (polynomial.rs:371-405): both trimmed, the zero polynomial when deg a < deg b, remainder dropped"""
    a, b = trim([v % p for v in a]), trim(b)
    assert b
    if len(a) < len(b):
        return []
    rem = list(a)
    inv = pow(b[-1], p - 2, p)
    q = [0] * (len(a) - len(b) + 1)
    for i in range(len(q) - 1, -1, -1):
        c = rem[i + len(b) - 1] * inv % p
        q[i] = c
        if c:
            for j, bj in enumerate(b):
                rem[i + j] = (rem[i + j] - c * bj) % p
    return trim(q)


def mul(a, b, p):
    out = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            out[i + j] = (out[i + j] + x * y) % p
    return out


def rand_poly(rnd, p, n):
    return [rnd.getrandbits(300) % p for _ in range(n - 1)] + [1 + rnd.getrandbits(300) % (p - 1)] if n else []


def div_host(mz, fid, polys, roots, **kw):
    return [ints(q) for q in mz.poly_div_roots(fid, [limbs(fid, f) for f in polys], roots, **kw)]


def div_dev(env, fid, polys, roots, stride=None):
    torch, mz, dev, st = env
    stride = stride if stride is not None else max([len(f) for f in polys] + [0])
    flat = np.zeros((max(len(polys) * stride, 1), NL[fid]), dtype=np.uint64)
    for i, f in enumerate(polys):
        flat[i * stride:i * stride + len(f)] = limbs(fid, f)
    d_in = torch.from_numpy(flat.view(np.int64).reshape(-1).copy()).to(dev)
    d_out = torch.full_like(d_in, -1)                   # the call must clear what lies behind a quotient
    lens = mz.poly_div_roots_dev(fid, d_in.data_ptr(), stride, [len(f) for f in polys], roots, d_out.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(d_in.cpu(), torch.from_numpy(flat.view(np.int64).reshape(-1))), "the input rows were written"
    out = d_out.cpu().numpy().view(np.uint64).reshape(-1, NL[fid])
    rows = []
    for i in range(len(polys)):
        row = ints(out[i * stride:(i + 1) * stride])
        assert all(v == 0 for v in row[lens[i]:]), "row %d is not zero behind its quotient" % i
        rows.append(row[:lens[i]])
    return rows


@pytest.mark.parametrize("fid", [FR, M128])
@pytest.mark.parametrize("n", LENGTHS)
def test_every_length_and_root_count_matches_long_division(env, fid, n):
    """one call with four rows of n coefficients and 0, 1, 2 and 5 roots (ragged root counts in one call): host and device forms"""
    rnd = random.Random(1000 * fid + n)
    p = PRIME[fid]
    polys = [rand_poly(rnd, p, n) for _ in ROOT_COUNTS]
    roots = [[rnd.randrange(p) for _ in range(k)] for k in ROOT_COUNTS]
    want = [long_div(f, zerofier(r, p), p) for f, r in zip(polys, roots)]
    assert [len(w) for w in want] == [max(n - k, 0) if k else n for k in ROOT_COUNTS]
    assert div_host(env[1], fid, polys, roots) == want
    assert div_dev(env, fid, polys, roots) == want


@pytest.mark.parametrize("fid", [FR, M128])
def test_ragged_rows_special_roots_and_divisions(env, fid):
    rnd = random.Random(77 + fid)
    p = PRIME[fid]
    g = rand_poly(rnd, p, 40)
    rr = [rnd.randrange(p) for _ in range(3)]
    polys, roots = [], []
    polys.append(mul(g, zerofier(rr, p), p)); roots.append(rr)                       # exact: the quotient is g
    polys.append([(v + (i == 0)) % p for i, v in enumerate(polys[0])]); roots.append(rr)   # inexact: remainder 1 dropped
    polys.append(rand_poly(rnd, p, 50)); roots.append([rr[0], rr[0], rr[0], rr[1]])  # a repeated root
    polys.append(rand_poly(rnd, p, 9000)); roots.append([0, p - 1])                  # roots 0 and p - 1, a long row beside short ones
    polys.append(rand_poly(rnd, p, 17)); roots.append([0])
    polys.append(rand_poly(rnd, p, 17) + [0] * 20); roots.append(rr)                 # untrimmed input
    polys.append(rand_poly(rnd, p, 3) + [0] * 30); roots.append(rr)                  # trimmed length 3 <= 3 roots: zero, though 33 > 3 given
    polys.append(rand_poly(rnd, p, 4) + [0] * 30); roots.append(rr)                  # trimmed length 4: one coefficient
    polys.append([0] * 25); roots.append([5])                                        # the zero polynomial, untrimmed
    polys.append([0] * 25); roots.append([])
    polys.append(rand_poly(rnd, p, 12) + [0] * 3); roots.append([])                  # no roots: the row trimmed
    polys.append(rand_poly(rnd, p, 5)); roots.append([rnd.randrange(p) for _ in range(5)])   # len == roots: empty
    polys.append(rand_poly(rnd, p, 5)); roots.append([rnd.randrange(p) for _ in range(9)])   # len < roots: empty
    polys.append([]); roots.append([1, 2])
    polys.append(rand_poly(rnd, p, 1)); roots.append([])
    want = [long_div(f, zerofier(r, p), p) for f, r in zip(polys, roots)]
    assert want[0] == g and want[1] == g and want[6] == [] and len(want[7]) == 1 and want[8] == [] and want[11] == [] and want[12] == []
    assert div_host(env[1], fid, polys, roots) == want
    assert div_dev(env, fid, polys, roots) == want
    assert div_dev(env, fid, polys, roots, stride=9100) == want                      # a stride beyond the longest row
    assert div_host(env[1], fid, polys[:3], roots[:3], stride=64) == want[:3]
    assert env[1].poly_div_roots(fid, [], []) == []


def test_fr_single_root_equals_the_kzg_opening_quotient(env):
    """(f - f(u)) / (X - u) of open_kzg is the same floor quotient: mzk_kzg_open_quotient_dev row by row"""
    torch, mz, dev, st = env
    rnd = random.Random(5)
    p = PRIME[FR]
    L = mz.lib()
    for n in (2, 33, 1 << 13, (1 << 13) + 1, (1 << 16) + 5):
        f, u = rand_poly(rnd, p, n), rnd.randrange(p)
        d_f = torch.from_numpy(limbs(FR, f).view(np.int64).reshape(-1).copy()).to(dev)
        d_q = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_y = torch.zeros(4, dtype=torch.int64, device=dev)
        ul = limbs(FR, [u])
        rc = L.mzk_kzg_open_quotient_dev(ctypes.c_void_p(d_f.data_ptr()), ctypes.c_size_t(n), ul.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.c_void_p(d_y.data_ptr()), ctypes.c_void_p(d_q.data_ptr()), ctypes.c_void_p(st))
        assert rc == 0, L.mzk_last_error().decode()
        torch.cuda.synchronize()
        kzg_q = ints(d_q.cpu().numpy().view(np.uint64).reshape(-1, 4)[:n - 1])
        assert div_dev(env, FR, [f], [[u]]) == [trim(kzg_q)]


def test_many_rows_in_one_call(env):
    """a boundary-quotient shaped batch: many registers of one length, each with its own few roots"""
    rnd = random.Random(11)
    p = PRIME[M128]
    polys = [rand_poly(rnd, p, 300) for _ in range(70)]
    roots = [[rnd.randrange(p) for _ in range(i % 4)] for i in range(70)]
    assert div_dev(env, M128, polys, roots) == [long_div(f, zerofier(r, p), p) for f, r in zip(polys, roots)]


@pytest.mark.parametrize("fid", [FR, M128])
def test_error_codes(env, fid):
    torch, mz, dev, st = env
    L = mz.lib()
    p, nl = PRIME[fid], NL[fid]
    sz = ctypes.c_size_t
    f = limbs(fid, [1, 2, 3, 4])
    out = np.zeros_like(f)
    lens, olens = (sz * 1)(4), (sz * 1)()
    r = limbs(fid, [7, 8])
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    call = lambda *a: L.mzk_poly_div_roots(*a)
    ok_args = [fid, ptr(f), sz(4), lens, sz(1), ptr(r), (sz * 2)(0, 2), ptr(out), olens]
    assert call(*ok_args) == 0 and olens[0] == 2
    for k in (1, 3, 6, 7, 8):                                        # polys, lens, root_offsets, out, out_lens
        a = list(ok_args); a[k] = None
        assert call(*a) == E_ARG, k
    a = list(ok_args); a[5] = None
    assert call(*a) == E_ARG                                         # roots missing while some are asked for
    a = list(ok_args); a[5] = None; a[6] = (sz * 2)(0, 0)
    assert call(*a) == 0 and olens[0] == 4                           # no roots at all: roots may be null
    for bad in (2, 3, -1):
        a = list(ok_args); a[0] = bad
        assert call(*a) == E_ARG
    a = list(ok_args); a[5] = ptr(limbs(fid, [7, p]))
    assert call(*a) == E_RANGE                                       # root == p
    a = list(ok_args); a[1] = ptr(limbs(fid, [1, 2, p, 4]))
    assert call(*a) == E_RANGE                                       # host form: coefficient == p
    a = list(ok_args); a[6] = (sz * 2)(2, 0)
    assert call(*a) == E_LENGTH                                      # decreasing offsets
    a = list(ok_args); a[2] = sz(3)
    assert call(*a) == E_LENGTH                                      # stride < len
    a = list(ok_args); a[4] = sz(0); a[1] = a[3] = a[6] = a[7] = a[8] = None
    assert call(*a) == 0                                             # count == 0: nothing is read
    with pytest.raises(mz.MzkError) as e:
        mz.poly_div_roots(fid, [f], [[p]])
    assert e.value.code == E_RANGE
    # the device form: the same checks but for the coefficients, which it does not read on the host
    d = torch.zeros(8 * nl, dtype=torch.int64, device=dev)
    with pytest.raises(mz.MzkError) as e:
        mz.poly_div_roots_dev(fid, d.data_ptr(), 3, [4], [[1]], d.data_ptr() + 4 * 8 * nl, st)
    assert e.value.code == E_LENGTH
    with pytest.raises(mz.MzkError) as e:
        mz.poly_div_roots_dev(fid, 0, 4, [4], [[1]], d.data_ptr(), st)
    assert e.value.code == E_ARG
    with pytest.raises(mz.MzkError) as e:
        mz.poly_div_roots_dev(fid, d.data_ptr(), 4, [4], [[p]], d.data_ptr() + 4 * 8 * nl, st)
    assert e.value.code == E_RANGE


def test_kzg_and_workspace_unaffected(env):
    """the division shares the engine and the workspace slots of the KZG openings: an opening before and after gives the same bytes, and
    the workspace can be released afterwards"""
    torch, mz, dev, st = env
    rnd = random.Random(3)
    p = PRIME[FR]
    n = 5000
    f, u = rand_poly(rnd, p, n), rnd.randrange(p)
    L = mz.lib()

    def opening():
        d_f = torch.from_numpy(limbs(FR, f).view(np.int64).reshape(-1).copy()).to(dev)
        d_q = torch.zeros(4 * n, dtype=torch.int64, device=dev)
        d_y = torch.zeros(4, dtype=torch.int64, device=dev)
        ul = limbs(FR, [u])
        assert L.mzk_kzg_open_quotient_dev(ctypes.c_void_p(d_f.data_ptr()), ctypes.c_size_t(n), ul.ctypes.data_as(ctypes.c_void_p),
                                           ctypes.c_void_p(d_y.data_ptr()), ctypes.c_void_p(d_q.data_ptr()), ctypes.c_void_p(st)) == 0
        torch.cuda.synchronize()
        return ints(d_y.cpu().numpy().view(np.uint64).reshape(1, 4))[0], d_q.cpu()

    y0, q0 = opening()
    assert y0 == sum(c * pow(u, i, p) for i, c in enumerate(f)) % p
    g = [rand_poly(rnd, PRIME[M128], 20000) for _ in range(3)]
    roots = [[1, 2, 3], [4], [5, 6]]
    mine = div_dev(env, M128, g, roots)
    y1, q1 = opening()
    assert y1 == y0 and torch.equal(q0, q1)
    assert div_dev(env, M128, g, roots) == mine == [long_div(a, zerofier(r, PRIME[M128]), PRIME[M128]) for a, r in zip(g, roots)]
    mz.trim_workspace()
    assert div_dev(env, M128, g[:1], roots[:1]) == mine[:1]
