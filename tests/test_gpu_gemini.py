"""Gemini on the GPU (mzk_gemini_*): split-and-fold, commit_gemini and open_gemini (algebra/gemini.rs:51-144) bit-exact against the
model (tests/gemini_model.py), the golden vectors, the CPU oracle and the trapdoor identities, on every SRS handle layout."""
import ctypes, json, os, random, sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import pytest
import orc
import gemini_model as gm

pytestmark = pytest.mark.gpu
P = gm.P


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as mz
    mz.init(0)
    return mz


def arr(v):
    return orc.to_limbs(list(v), 4)


def rand_coefs(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(P) for _ in range(n)]


def levels_model(coefs, rhos):
    return [arr(f) for f in gm.split_and_fold(coefs, rhos)]


def handle(mz, L, torch, powers, with_tables=1, direct_bits=0):
    """an mzk_srs handle of the given layout over device-resident powers, wrapped as a myzkp_amd.Srs"""
    p = np.ascontiguousarray(powers, dtype=np.uint64)
    d = torch.from_numpy(p.view(np.int64).reshape(-1).copy()).cuda()
    h = ctypes.c_void_p()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mzk_srs_from_device_ex(ctypes.c_void_p(d.data_ptr()), ctypes.c_size_t(p.shape[0]), ctypes.c_int(with_tables), ctypes.byref(h), st)
    assert rc == 0, L.mzk_last_error().decode()
    torch.cuda.synchronize()
    s = mz.Srs.__new__(mz.Srs)
    s._h, s.n = h, p.shape[0]
    s._keep = d                                      # the points stay alive as long as the handle
    if direct_bits:
        assert s.build_direct(direct_bits) == direct_bits
    return s


@pytest.mark.parametrize("el", list(range(0, 13)) + [20])
def test_split_fold_matches_model(mz, el):
    n = 1 << el
    coefs = rand_coefs(10 + el, n)
    rhos = rand_coefs(50 + el, el)
    got = mz.gemini_split_fold(arr(coefs), rhos)
    want = gm.split_and_fold(coefs, rhos)
    assert len(got) == el + 1
    for i in range(el + 1):
        assert np.array_equal(got[i], arr(want[i])), i


@pytest.mark.parametrize("el", [5, 12, 20])
def test_split_fold_dev_equals_host(mz, el):
    import torch
    n = 1 << el
    c = arr(rand_coefs(70 + el, n))
    rhos = rand_coefs(80 + el, el)
    host = np.concatenate(mz.gemini_split_fold(c, rhos))
    d_out = torch.zeros((2 * n - 1) * 4, dtype=torch.int64, device="cuda")
    d_out[:n * 4] = torch.from_numpy(c.view(np.int64).reshape(-1).copy()).cuda()
    st = torch.cuda.current_stream().cuda_stream
    mz.gemini_split_fold_dev(d_out.data_ptr(), n, rhos, d_out.data_ptr(), st)        # in place: level 0 already there
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(-1, 4), host)
    d_in = torch.from_numpy(c.view(np.int64).reshape(-1).copy()).cuda()
    d_out2 = torch.zeros_like(d_out)
    mz.gemini_split_fold_dev(d_in.data_ptr(), n, rhos, d_out2.data_ptr(), st)
    torch.cuda.synchronize()
    assert torch.equal(d_out, d_out2)


def test_golden_vectors(mz):
    d = json.load(open(os.path.join(HERE, "golden", "gemini_vectors.json")))
    srs = mz.Srs(orc.kzg_setup_ref(d["alpha"], d["max_d"]))
    for case, rhos in (("gemini", d["gemini"]["rhos"]), ("sumcheck", d["sumcheck"]["rs"])):
        g = d[case]
        coefs = g["coef"] if case == "gemini" else g["coefs"]
        levels = mz.gemini_split_fold(arr(coefs), rhos)
        assert [orc.from_limbs(l) for l in levels] == g["levels"]
        assert [list(p) for p in srs.gemini_commit(levels)] == g["commits"]
        ys, ws, deg = srs.gemini_open(levels, g["beta"])
        assert [list(y) for y in ys] == g["ys"]
        assert [list(p) for p in ws] == g["ws"]
        assert [list(p) for p in deg] == g["deg"]
        assert ws[-1] == (0, 0)                    # level el - 1: two coefficients, empty quotient
        mu = g["levels"][-1][0]
        assert gm.gemini_relation(rhos, g["beta"], [y[0] for y in ys], [y[1] for y in ys], [y[2] for y in ys[1:]] + [mu])
    srs.close()


@pytest.mark.parametrize("el", [1, 4, 10])
def test_levels_match_the_oracle(mz, el):
    n = 1 << el
    alpha = 0xC0FFEE + el
    max_d = n + 3
    powers = orc.kzg_setup_ref(alpha, max_d)
    srs = mz.Srs(powers)
    coefs = rand_coefs(90 + el, n)
    rhos = rand_coefs(91 + el, el)
    beta = rand_coefs(92 + el, 1)[0]
    levels = mz.gemini_split_fold(arr(coefs), rhos)
    commits = srs.gemini_commit(levels)
    ys, ws, deg = srs.gemini_open(levels, beta)
    us = [beta, gm.neg(beta), beta * beta % P]
    for i, f in enumerate(levels):
        assert commits[i] == orc.msm_ref(f, powers[:f.shape[0]]), i
        rc, want = orc.kzg_degree_bound_ref(f, powers, 1 << (el - i))
        assert rc == 0 and deg[i] == want, i
        if i < el:
            wys, ww = orc.kzg_batch_open_ref(f, us, powers)
            assert list(ys[i]) == wys and ws[i] == ww, i
    fs = [orc.from_limbs(l) for l in levels]
    assert gm.debug_verify(rhos, fs[-1][0], fs, beta)
    srs.close()


@pytest.mark.parametrize("el", [16, 20])
def test_trapdoor_identities(mz, el):
    n = 1 << el
    alpha = 0x5EED0000 + el
    max_d = n + 5
    srs = mz.Srs(mz.kzg_setup_g1(alpha, max_d))
    coefs = rand_coefs(200 + el, n)
    rhos = rand_coefs(201 + el, el)
    beta = rand_coefs(202 + el, 1)[0]
    levels = mz.gemini_split_fold(arr(coefs), rhos)
    commits = srs.gemini_commit(levels)
    ys, ws, deg = srs.gemini_open(levels, beta)
    gm.trapdoor_check(levels, beta, alpha, max_d, commits, ys, ws, deg)
    srs.close()


def _layout_results(srs, levels, beta):
    return srs.gemini_commit(levels), srs.gemini_open(levels, beta)


def _same_proof_on_layouts(mz, el, npts, alpha, seed, layouts):
    """commit + open of one random g on handles of the given layouts over the same powers: all equal, the first one also checked
    by the trapdoor identities.  layouts: (with_tables, direct_bits, table budget, expected bucket sets)"""
    import torch
    L = mz.lib()
    n = 1 << el
    powers = mz.kzg_setup_g1(alpha, npts - 1)
    coefs, rhos, beta = rand_coefs(seed, n), rand_coefs(seed + 1, el), rand_coefs(seed + 2, 1)[0]
    levels = mz.gemini_split_fold(arr(coefs), rhos)
    first = None
    try:
        for wt, db, budget, sets in layouts:
            assert L.mzk_set_table_budget(ctypes.c_size_t(budget)) == 0
            srs = handle(mz, L, torch, powers, wt, db)
            assert L.mzk_srs_bucket_sets(srs._h) == sets, (wt, budget)
            got = _layout_results(srs, levels, beta)
            if first is None:
                first = got
                (ys, ws, deg) = got[1]
                gm.trapdoor_check(levels, beta, alpha, npts - 1, got[0], ys, ws, deg)
            assert got == first, (wt, db, budget)
            srs.close()
    finally:
        L.mzk_set_table_budget(ctypes.c_size_t(0))


def test_small_levels_on_every_handle_layout(mz):
    """2^12 coefficients against 2^12 + 3 powers: every level is small.  On the handles with a grid-batched path (10-bit default,
    8-bit and 10-bit explicit, direct tables over the 10-bit ones) commitments, quotients and degree bounds go through one batched
    pass each, the degree bounds at a base shifted by max_d - 2^12 (for the direct tables: 2^(c-1) records per point); on the
    16-bit and no-table handles every level is a generic MSM over plain copies of the points it uses."""
    _same_proof_on_layouts(mz, 12, (1 << 12) + 3, 0xABCDEF, 300,
                           [(1, 0, 0, 1), (8, 0, 0, 1), (16, 0, 0, 1), (0, 0, 0, 0), (1, 8, 0, 1), (10, 0, 0, 1)])


def test_sliced_table_msm_on_narrow_and_direct_handles(mz):
    """2^13 coefficients against 2^13 + 3 powers: level 0 is above the batched size, so its commitment, quotient and degree bound are
    single MSMs on the handle's narrow window tables, the degree bound with the tables entered max_d - 2^13 = 2 rows further on (also
    on a handle that holds direct tables, which single MSMs do not use); the levels below go through the batched pass."""
    _same_proof_on_layouts(mz, 13, (1 << 13) + 3, 0x24681357, 320, [(1, 0, 0, 1), (8, 0, 0, 1), (12, 0, 0, 1), (1, 8, 0, 1)])


def test_sliced_table_msm_on_wide_degraded_and_no_table_handles(mz):
    """2^17 coefficients against 2^17 + 5 powers: level 0 is above the size that takes plain points, so its commitment, quotient and
    degree bound (tables entered max_d - 2^17 = 4 rows further on) are MSMs on the handle's own layout -- 16-bit tables with one,
    two and four bucket sets (mzk_set_table_budget), 17-bit tables, and no tables (prepared points with their phi images one table
    stride further on); levels of 2^16 and below are generic MSMs over plain copies of the points."""
    npts = (1 << 17) + 5
    full = 16 * npts * 64
    _same_proof_on_layouts(mz, 17, npts, 0x97531, 340,
                           [(1, 0, 0, 1), (1, 0, full - 1, 2), (1, 0, 8 * npts * 64 - 1, 4), (17, 0, 0, 1), (0, 0, 0, 0), (1, 0, 1, 0)])


def test_open_dev_equals_host(mz):
    import torch
    el = 11
    n = 1 << el
    srs = mz.Srs(mz.kzg_setup_g1(0x77, n + 1))
    c = arr(rand_coefs(400, n))
    rhos, beta = rand_coefs(401, el), rand_coefs(402, 1)[0]
    levels = mz.gemini_split_fold(c, rhos)
    packed = np.concatenate(levels)
    commits = srs.gemini_commit(levels)
    ys, ws, deg = srs.gemini_open(levels, beta)
    L = mz.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    d_l = torch.from_numpy(packed.view(np.int64).reshape(-1).copy()).cuda()
    d_c = torch.zeros((el + 1) * 8, dtype=torch.int64, device="cuda")
    d_y = torch.zeros(el * 12, dtype=torch.int64, device="cuda")
    d_w = torch.zeros(el * 8, dtype=torch.int64, device="cuda")
    d_d = torch.zeros((el + 1) * 8, dtype=torch.int64, device="cuda")
    dp = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.mzk_gemini_commit_srs_dev(srs._h, dp(d_l), ctypes.c_size_t(n), dp(d_c), st) == 0
    b = orc.to_limbs([beta], 4)
    assert L.mzk_gemini_open_srs_dev(srs._h, dp(d_l), ctypes.c_size_t(n), orc.ptr(b), dp(d_y), dp(d_w), dp(d_d), st) == 0
    torch.cuda.synchronize()
    h = lambda t: t.cpu().numpy().view(np.uint64)
    assert mz.array_to_points(h(d_c)) == commits
    y = orc.from_limbs(h(d_y).reshape(-1, 4))
    assert [tuple(y[3 * i:3 * i + 3]) for i in range(el)] == ys
    assert mz.array_to_points(h(d_w)) == ws and mz.array_to_points(h(d_d)) == deg
    srs.close()


def test_error_paths(mz):
    from myzkp_amd import MzkError
    srs = mz.Srs(mz.kzg_setup_g1(0x99, 16))           # 17 powers: max_d = 16
    for n, code in ((3, -2), (0, -2), (12, -2)):
        with pytest.raises(MzkError) as e:
            mz.gemini_split_fold(np.zeros((n, 4), dtype=np.uint64), [1] * 2)
        assert e.value.code == code, n
    with pytest.raises(MzkError) as e:
        mz.gemini_split_fold(arr(range(8)), [1, 2])
    assert e.value.code == -5
    with pytest.raises(MzkError) as e:
        mz.gemini_split_fold(arr(range(8)), [1, P, 2])
    assert e.value.code == -6
    levels = mz.gemini_split_fold(arr(range(1, 17)), [3, 5, 7, 11])
    with pytest.raises(MzkError) as e:                  # 2^4 coefficients need max_d >= 16: a 16-power SRS is one short
        mz.Srs(mz.kzg_setup_g1(0x99, 15)).gemini_open(levels, 1234)
    assert e.value.code == -5
    with pytest.raises(MzkError) as e:
        srs.gemini_open(levels, P)
    assert e.value.code == -6
    for b in (0, 1, P - 1):
        with pytest.raises(MzkError) as e:
            srs.gemini_open(levels, b)
        assert e.value.code == -1, b
    # nothing left behind: the next call is right
    ys, ws, deg = srs.gemini_open(levels, 1234)
    fs = [orc.from_limbs(l) for l in levels]
    assert [list(y) for y in ys] == [[gm.poly_eval(f, u) for u in (1234, P - 1234, 1234 * 1234)] for f in fs[:4]]
    srs.close()
