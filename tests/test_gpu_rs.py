"""Reed-Solomon over GF(2^8) on the device (myzkp_amd/csrc/mzk_rs.hip: encode in both forms, the Fr columns, syndromes, decode, the 2D
code) against tests/rs_model.py, the Python restatement of algebra/reedsolomon.rs -- every comparison bit for bit.  Shapes are the
smallest at which each path can go wrong: every parity-register count and the boundaries between them, the lane and the wave encoder,
batches around the workgroup and wave sizes, strided and in-place encoder views.  Decoding is covered at the group widths 8 (d = 1, 4,
5, 8), 32 (d = 32) and 64 (d = 128), the syndromes at d = 4, 8, 32 and 254, the 2D code up to 9 x 8.  Width 16, d at the boundaries
of every width, errors placed after the lane ownership, miscorrection, the 2D code beyond one stride per lane, the wave encoder's
64-byte chunk boundaries and the lane encoder's two read paths side by side are in test_gpu_rs_matrix.py."""
import ctypes, random
import numpy as np
import pytest
import rs_model as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init_devices([0])
    yield m
    m.init_devices([0])


def _rows(rnd, batch, width):
    return np.array([[rnd.randrange(256) for _ in range(width)] for _ in range(batch)], dtype=np.uint8).reshape(batch, width)


def _model_encode(n, k, msgs):
    rs = M.ReedSolomon(n, k)
    return np.array([rs.encode_fixed([int(v) for v in row]) for row in msgs], dtype=np.uint8).reshape(len(msgs), n)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


# ---- encode -------------------------------------------------------------------------------------------------------------------------
def test_encode_every_shape_up_to_20(mz):
    rnd = random.Random(11)
    for n in range(1, 21):
        for k in range(1, n + 1):
            msgs = _rows(rnd, 3, k)
            assert np.array_equal(mz.rs_encode(n, k, msgs), _model_encode(n, k, msgs)), (n, k)
            assert np.array_equal(mz.rs_generator_poly(n, k), np.array(M.ReedSolomon(n, k).generator_polynomial(), dtype=np.uint8)), (n, k)


@pytest.mark.parametrize("d", [0, 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 253, 254])
def test_encode_at_the_form_boundaries(mz, d):
    """1, 2, 4, 8 parity registers per lane up to d = 32, one codeword per wave beyond; n = 255 throughout (k = 1 at d = 254)"""
    rnd = random.Random(100 + d)
    n, k = 255, 255 - d
    msgs = _rows(rnd, 5, k)
    assert np.array_equal(mz.rs_encode(n, k, msgs), _model_encode(n, k, msgs))


@pytest.mark.parametrize("n", [1, 2, 5, 33, 34, 200])
def test_encode_one_message_symbol(mz, n):
    msgs = np.array([[1], [0xFF], [0], [0x53]], dtype=np.uint8)
    assert np.array_equal(mz.rs_encode(n, 1, msgs), _model_encode(n, 1, msgs))


@pytest.mark.parametrize("n, k", [(16, 8), (255, 223)])
@pytest.mark.parametrize("batch", [1, 63, 64, 65, 257])
def test_encode_batches_around_wave_and_workgroup(mz, n, k, batch):
    rnd = random.Random(batch * 1000 + n)
    msgs = _rows(rnd, batch, k)
    assert np.array_equal(mz.rs_encode(n, k, msgs), _model_encode(n, k, msgs))


@pytest.mark.parametrize("n, k", [(16, 8), (15, 8), (255, 223), (255, 100)])
def test_encode_special_messages(mz, n, k):
    rnd = random.Random(n + k)
    msgs = _rows(rnd, 4, k)
    msgs[0, :] = 0
    msgs[1, :] = 0xFF
    msgs[2, k - 1] = 0                       # the reference's vector is one shorter here
    msgs[3, k // 2:] = 0                     # ... and much shorter here
    got = mz.rs_encode(n, k, msgs)
    assert np.array_equal(got, _model_encode(n, k, msgs))
    rs = M.ReedSolomon(n, k)
    for row, g in zip(msgs, got):            # device form = reference form, zero-extended
        ref = rs.encode([int(v) for v in row])
        assert list(g[:len(ref)]) == ref and not g[len(ref):].any()
    assert not got[0].any()


@pytest.mark.parametrize("n, k", [(16, 8), (13, 6), (60, 20)])
def test_encode_strided_views(mz, n, k):
    """symbol stride != 1 and codeword stride != n on both sides; bytes between the symbols stay untouched"""
    import torch
    rnd = random.Random(n * 7 + k)
    batch, ms, mc, cs, cc = 70, 3, 3 * k + 5, 2, 2 * n + 7
    msgs = _rows(rnd, batch, k)
    src = np.full(batch * mc, 0xAA, dtype=np.uint8)
    for b in range(batch):
        src[b * mc: b * mc + ms * k: ms] = msgs[b]
    d_src, d_dst = _dev(src), torch.full((batch * cc,), 0x55, dtype=torch.uint8, device="cuda")
    mz.rs_encode_view_dev(n, k, d_src.data_ptr(), ms, mc, batch, d_dst.data_ptr(), cs, cc, None, _stream())
    torch.cuda.synchronize()
    out = d_dst.cpu().numpy()
    want = np.full(batch * cc, 0x55, dtype=np.uint8)
    model = _model_encode(n, k, msgs)
    for b in range(batch):
        want[b * cc: b * cc + cs * n: cs] = model[b]
    assert np.array_equal(out, want)
    # the transposed output: symbol i of every codeword contiguous (codeword stride 1, symbol stride batch)
    d_t = torch.zeros(n * batch, dtype=torch.uint8, device="cuda")
    mz.rs_encode_view_dev(n, k, d_src.data_ptr(), ms, mc, batch, d_t.data_ptr(), batch, 1, None, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy().reshape(n, batch), model.T)


@pytest.mark.parametrize("n, k", [(16, 8), (15, 8), (60, 20)])
def test_encode_in_place(mz, n, k):
    """the one in-place form the header allows: the message already in positions d .. n-1 of its codeword"""
    import torch
    rnd = random.Random(n * 9 + k)
    batch, d = 66, n - k
    msgs = _rows(rnd, batch, k)
    buf = np.full((batch, n), 0xEE, dtype=np.uint8)
    buf[:, d:] = msgs
    d_buf = _dev(buf.reshape(-1))
    mz.rs_encode_view_dev(n, k, d_buf.data_ptr() + d, 1, n, batch, d_buf.data_ptr(), 1, n, None, _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_buf.cpu().numpy().reshape(batch, n), _model_encode(n, k, msgs))


# ---- the Fr columns -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [8, 65])
def test_columns_are_the_widened_transpose(mz, batch):
    import torch
    rnd = random.Random(batch)
    n, k = 16, 8
    msgs = _rows(rnd, batch, k)
    d_m = _dev(msgs.reshape(-1))
    d_c = torch.zeros(batch * n, dtype=torch.uint8, device="cuda")
    d_f = torch.full((n * batch * 4,), -1, dtype=torch.int64, device="cuda")
    mz.rs_encode_dev(n, k, d_m.data_ptr(), batch, d_c.data_ptr(), d_f.data_ptr(), _stream())
    torch.cuda.synchronize()
    code = _model_encode(n, k, msgs)
    assert np.array_equal(d_c.cpu().numpy().reshape(batch, n), code)
    want = np.zeros((n, batch, 4), dtype=np.uint64)
    want[:, :, 0] = code.T
    assert np.array_equal(d_f.cpu().numpy().view(np.uint64).reshape(n, batch, 4), want)


def test_avail_encode_then_commit_without_a_host_step(mz):
    """test_avail_no_error's shape (das/avail.rs:176-182): 32 bytes in chunks of 8, codewords of 16, one commitment per symbol position
    over the 4 chunks (avail.rs:87-98) -- encode with columns, then mzk_kzg_commit_srs_many_dev on them"""
    import torch
    import orc
    n, k, batch = 16, 8, 4
    data = np.arange(32, dtype=np.uint8).reshape(batch, k)
    pts = orc.synth_points(3, batch)
    srs = mz.Srs(pts)
    d_m = _dev(data.reshape(-1))
    d_c = torch.zeros(batch * n, dtype=torch.uint8, device="cuda")
    d_f = torch.zeros(n * batch * 4, dtype=torch.int64, device="cuda")
    d_o = torch.full((n * 8,), -1, dtype=torch.int64, device="cuda")
    st = _stream()
    mz.rs_encode_dev(n, k, d_m.data_ptr(), batch, d_c.data_ptr(), d_f.data_ptr(), st)
    rc = mz.lib().mzk_kzg_commit_srs_many_dev(srs._h, ctypes.c_void_p(d_f.data_ptr()), ctypes.c_size_t(batch), ctypes.c_size_t(n), ctypes.c_void_p(d_o.data_ptr()),
                                              ctypes.c_void_p(st))
    assert rc == 0, mz.lib().mzk_last_error()
    torch.cuda.synchronize()
    got = mz.array_to_points(d_o.cpu().numpy().view(np.uint64).reshape(n, 8))
    code = _model_encode(n, k, data)
    want = [mz.kzg_commit(mz.to_limbs([int(v) for v in code[:, i]], 4), pts) for i in range(n)]
    srs.close()
    assert got == want


# ---- syndromes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, k", [(7, 3), (16, 8), (255, 223), (255, 1)])
def test_syndromes_of_random_words(mz, n, k):
    rnd = random.Random(n * 3 + k)
    words = _rows(rnd, 5, n)
    rs = M.ReedSolomon(n, k)
    words[0] = rs.encode_fixed([int(v) for v in words[0, n - k:]])      # one codeword among them: all zero
    want = np.array([rs.compute_syndromes([int(v) for v in w]) for w in words], dtype=np.uint8)
    got = mz.rs_syndromes(n, k, words)
    assert np.array_equal(got, want)
    assert not got[0].any() and got[1:].any()


# ---- decode -------------------------------------------------------------------------------------------------------------------------
def _hit(rnd, cw, positions, value):
    r = list(cw)
    for p in positions:
        r[p] ^= value if value else rnd.randrange(1, 256)
    return r


def _decode_cases(n, k):
    """received words with e = 0 .. t + 2 errors: positions from {0, d-1, d, n-1} first or random, values 1, 0xFF or random"""
    rnd = random.Random(n * 1000 + k)
    rs = M.ReedSolomon(n, k)
    d, t = n - k, (n - k) // 2
    special = [p for p in dict.fromkeys([0, max(d - 1, 0), min(d, n - 1), n - 1])]
    words = []
    for e in range(0, min(t + 2, n) + 1):
        cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
        others = [p for p in range(n) if p not in special]
        rnd.shuffle(others)
        edge = (special + others)[:e]
        if n <= 32:
            words += [_hit(rnd, cw, edge, 1), _hit(rnd, cw, edge, 0xFF), _hit(rnd, cw, rnd.sample(range(n), e), 0), _hit(rnd, cw, rnd.sample(range(n), e), 0xFF)]
        else:
            words += [_hit(rnd, cw, edge, (1, 0xFF)[e & 1]), _hit(rnd, cw, rnd.sample(range(n), e), 0)] if e <= 2 or e >= t - 1 or e % 8 == 0 else \
                     [_hit(rnd, cw, rnd.sample(range(n), e), 0)]
    return rs, words


@pytest.mark.parametrize("n, k", [(7, 3), (8, 3), (16, 8), (12, 11), (255, 223), (255, 127)])
def test_decode_zero_to_t_plus_two_errors(mz, n, k):
    rs, words = _decode_cases(n, k)
    want = [rs.decode_status(w) for w in words]
    corr, msgs, status = mz.rs_decode(n, k, np.array(words, dtype=np.uint8), with_corrected=True)
    t = (n - k) // 2
    assert [int(s) for s in status] == [w[2] for w in want]
    assert np.array_equal(corr, np.array([w[0] for w in want], dtype=np.uint8))
    assert np.array_equal(msgs, np.array([w[1] for w in want], dtype=np.uint8).reshape(len(words), k))
    assert set(range(t + 1)) <= set(int(s) for s in status)              # every correctable count occurred and was corrected
    if t >= 1:
        assert 255 in status                                                # and beyond t the reference's None did


def test_decode_neighbouring_groups_take_different_paths(mz):
    """130 codewords whose error counts cycle 0, 1, .., t, t + 1: the eight-lane groups of one wave are clean, correcting and failing
    side by side"""
    rnd = random.Random(77)
    n, k = 16, 8
    rs = M.ReedSolomon(n, k)
    t = 4
    words = []
    for b in range(130):
        cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
        words.append(_hit(rnd, cw, rnd.sample(range(n), b % (t + 2)), 0))
    want = [rs.decode_status(w) for w in words]
    msgs, status = mz.rs_decode(n, k, np.array(words, dtype=np.uint8))
    assert [int(s) for s in status] == [w[2] for w in want]
    assert np.array_equal(msgs, np.array([w[1] for w in want], dtype=np.uint8))
    assert [int(s) for s in status[:5]] == [0, 1, 2, 3, 4]


def test_decode_with_either_output_left_out(mz):
    import torch
    rnd = random.Random(78)
    n, k, batch = 16, 8, 9
    rs = M.ReedSolomon(n, k)
    words = [_hit(rnd, rs.encode_fixed([rnd.randrange(256) for _ in range(k)]), rnd.sample(range(n), b % 6), 0) for b in range(batch)]
    want = [rs.decode_status(w) for w in words]
    d_r = _dev(np.array(words, dtype=np.uint8).reshape(-1))
    for with_corr, with_msgs in ((True, False), (False, True), (False, False)):
        d_c = torch.full((batch * n,), 0x77, dtype=torch.uint8, device="cuda")
        d_m = torch.full((batch * k,), 0x77, dtype=torch.uint8, device="cuda")
        d_s = torch.full((batch,), 0x77, dtype=torch.uint8, device="cuda")
        mz.rs_decode_dev(n, k, d_r.data_ptr(), batch, d_c.data_ptr() if with_corr else None, d_m.data_ptr() if with_msgs else None, d_s.data_ptr(), _stream())
        torch.cuda.synchronize()
        assert [int(s) for s in d_s.cpu().numpy()] == [w[2] for w in want]
        c, m = d_c.cpu().numpy().reshape(batch, n), d_m.cpu().numpy().reshape(batch, k)
        assert np.array_equal(c, np.array([w[0] for w in want], dtype=np.uint8)) if with_corr else (c == 0x77).all()
        assert np.array_equal(m, np.array([w[1] for w in want], dtype=np.uint8)) if with_msgs else (m == 0x77).all()


# ---- 2D -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("message, errors", [
    ([2, 4, 6], []),                                                       # test_no_errors_2d            (reedsolomon.rs:525-535)
    ([2, 8, 3], [(1, 1, 10)]),                                             # test_single_error_correction_2d      (:537-546)
    ([5, 4, 16], [(1, 0, 6), (1, 1, 5)]),                                  # test_multiple_error_correction_2d    (:548-558)
    ([8, 2, 3], [(1, 0, 6), (0, 1, 5)]),                                   # test_too_many_errors_2d              (:560-570)
])
def test_the_references_four_2d_tests(mz, message, errors):
    code = mz.rs2d_encode(4, 4, message)
    assert code.tolist() == M.encode_rs2d(message, M.setup_rs2d(4, 4, 3))
    assert [int(code[2][2]), int(code[2][3]), int(code[3][2])] == message
    for r, c, v in errors:
        code[r][c] = (int(code[r][c]) + v) & 0xFF                           # u8 addition, as the reference's tests do it
    got, cs, rs_ = mz.rs2d_decode(4, 4, code, 3, with_status=True)
    want, wcs, wrs = M.setup_rs2d(4, 4, 3).decode_status(code.tolist())
    assert want == message and got.tolist() == message
    assert cs.tolist() == wcs and rs_.tolist() == wrs


@pytest.mark.parametrize("col_n, row_n, message_len", [(6, 5, 7), (8, 8, 16), (9, 7, 10)])
def test_2d_round_trip_one_error_per_column_and_a_column_beyond_repair(mz, col_n, row_n, message_len):
    """message_len a perfect square (16) and not (7, 10: the matrix is zero-padded)"""
    rnd = random.Random(col_n * 100 + row_n)
    rs = M.ReedSolomon2D(col_n, row_n, message_len)
    data = [rnd.randrange(256) for _ in range(message_len)]
    code = mz.rs2d_encode(col_n, row_n, data)
    assert code.tolist() == rs.encode(data)
    assert mz.rs2d_decode(col_n, row_n, code, message_len).tolist() == data
    hit = code.copy()
    for c in range(row_n):
        hit[rnd.randrange(col_n)][c] ^= rnd.randrange(1, 256)
    got, cs, rs_ = mz.rs2d_decode(col_n, row_n, hit, message_len, with_status=True)
    want, wcs, wrs = rs.decode_status(hit.tolist())
    assert (None if got is None else got.tolist()) == want and cs.tolist() == wcs and rs_.tolist() == wrs
    if (col_n - rs.size) // 2 >= 1:
        assert want == data
    # a column the column code cannot repair: the first error pattern on column 1 that the model answers with None
    for attempt in range(50):
        broken = code.copy()
        for r in rnd.sample(range(col_n), min(col_n, (col_n - rs.size) // 2 + 2)):
            broken[r][1] ^= rnd.randrange(1, 256)
        want, wcs, wrs = rs.decode_status(broken.tolist())
        if wcs[1] == 255:
            break
    assert want is None and wcs[1] == 255
    got, cs, rs_ = mz.rs2d_decode(col_n, row_n, broken, message_len, with_status=True)
    assert got is None and cs.tolist() == wcs and rs_.tolist() == wrs


def test_2d_device_form(mz):
    import torch
    rnd = random.Random(5)
    col_n, row_n, ml = 8, 8, 16
    data = [rnd.randrange(256) for _ in range(ml)]
    d_d = _dev(np.array(data, dtype=np.uint8))
    d_code = torch.full((col_n * row_n,), 0x99, dtype=torch.uint8, device="cuda")
    mz.rs2d_encode_dev(col_n, row_n, d_d.data_ptr(), ml, d_code.data_ptr(), _stream())
    d_back = torch.zeros(ml, dtype=torch.uint8, device="cuda")
    d_ok = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    mz.rs2d_decode_dev(col_n, row_n, d_code.data_ptr(), ml, d_back.data_ptr(), d_ok.data_ptr(), None, None, _stream())
    torch.cuda.synchronize()
    assert d_code.cpu().numpy().reshape(col_n, row_n).tolist() == M.ReedSolomon2D(col_n, row_n, ml).encode(data)
    assert int(d_ok.cpu()[0]) == 1 and d_back.cpu().numpy().tolist() == data


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_in_the_plans_words(mz):
    L = mz.lib()
    buf = np.zeros(1024, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    sz = ctypes.c_size_t
    for n, k in ((256, 8), (16, 0), (8, 9)):
        for rc in (L.mzk_rs_encode(sz(n), sz(k), p, sz(1), p), L.mzk_rs_syndromes(sz(n), sz(k), p, sz(1), p), L.mzk_rs_decode(sz(n), sz(k), p, sz(1), p, p, p),
                   L.mzk_rs_generator_poly(sz(n), sz(k), p)):
            assert rc == -1
            assert L.mzk_last_error().decode() == "rs: (n, k) = (%d, %d) is outside 1 <= k <= n <= 255 (the evaluation points 2^i repeat from n = 256 on)" % (n, k)
    for batch in (0, (1 << 31) + 1):
        assert L.mzk_rs_encode(sz(16), sz(8), p, sz(batch), p) == -1
        assert L.mzk_last_error().decode() == "rs: a batch of %d codewords is outside 1 .. 2^31" % batch
        assert L.mzk_rs_decode_dev(sz(16), sz(8), p, sz(batch), p, p, p, None) == -1
    assert L.mzk_rs2d_encode(sz(4), sz(4), p, sz(17), p) == -1              # size 5 > 4
    assert "outside 1 <= k <= n <= 255" in L.mzk_last_error().decode()
    assert L.mzk_rs2d_encode(sz(4), sz(4), p, sz(0), p) == -1
