"""The Reed-Solomon decoder at every group width and the 2D code strided (myzkp_amd/csrc/mzk_rs.hip) against tests/rs_model.py, bit
for bit, on the tables of tests/rs_matrix_cases.py (which tests/test_rs_matrix_cases.py checks without a GPU):

  * decode and syndromes at W = 8, 16, 32, 64 with d at, just below and just above every width, one to three coefficients per lane,
    errors placed after the lane ownership (one lane's stride, a whole stride, W - 1 .. W + 1, a burst) and 0 .. t + 2 of them, the
    outcomes interleaved inside a wave;
  * words that the decoder accepts although they are wrong, because they are within t of ANOTHER codeword;
  * the 2D code where its column pass -- the strided, in-place form of every kernel -- is the copy, the lane encoder with 8 registers,
    the wave encoder, and the decoder at W = 16, 32, 64 beyond a lane's first stride; up to 70 column statuses;
  * the wave encoder at the 64-byte chunk boundaries of the message, the lane encoder through its word path and its byte path on the
    same messages."""
import numpy as np
import pytest
import rs_matrix_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init_devices([0])
    yield m
    m.init_devices([0])


def _u8(rows):
    return np.array(rows, dtype=np.uint8)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _full(count, value):
    import torch
    return torch.full((count,), value, dtype=torch.uint8, device="cuda")


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _ids(cases):
    return ["-".join(str(v) for v in c) for c in cases]


# ---- decode and syndromes, 1D -------------------------------------------------------------------------------------------------------
def _batch(n, k):
    words, want = C.words(n, k), C.expected(n, k)
    recv = _u8([w[1] for w in words])
    return recv, _u8([w[0] for w in want]), _u8([w[1] for w in want]).reshape(len(words), k), _u8([w[2] for w in want]), \
        _u8([w[3] for w in want]).reshape(len(words), n - k)


@pytest.mark.parametrize("n, k", C.CODES, ids=_ids(C.CODES))
def test_decode_at_every_group_width(mz, n, k):
    recv, corr, msgs, status, _ = _batch(n, k)
    got_c, got_m, got_s = mz.rs_decode(n, k, recv, with_corrected=True)
    assert got_s.tolist() == status.tolist()
    assert np.array_equal(got_c, corr)
    assert np.array_equal(got_m, msgs)


@pytest.mark.parametrize("n, k", C.DEV_CODES, ids=_ids(C.DEV_CODES))
def test_decode_device_form_writes_what_it_owns(mz, n, k):
    recv, corr, msgs, status, _ = _batch(n, k)
    batch = len(recv)
    d_r = _dev(recv.reshape(-1))
    d_c, d_m, d_s = _full(batch * n + 8, 0x5A), _full(batch * k + 8, 0x5A), _full(batch + 8, 0x5A)
    mz.rs_decode_dev(n, k, d_r.data_ptr(), batch, d_c.data_ptr(), d_m.data_ptr(), d_s.data_ptr(), _stream())
    c, m, s = _host(d_c), _host(d_m), _host(d_s)
    assert s[:batch].tolist() == status.tolist()
    assert np.array_equal(c[:batch * n].reshape(batch, n), corr)
    assert np.array_equal(m[:batch * k].reshape(batch, k), msgs)
    assert (c[batch * n:] == 0x5A).all() and (m[batch * k:] == 0x5A).all() and (s[batch:] == 0x5A).all()
    assert np.array_equal(_host(d_r).reshape(batch, n), recv)


@pytest.mark.parametrize("n, k", C.CODES, ids=_ids(C.CODES))
def test_syndromes_at_every_group_width(mz, n, k):
    recv, _, _, _, syn = _batch(n, k)
    batch, d = len(recv), n - k
    assert np.array_equal(mz.rs_syndromes(n, k, recv), syn)
    d_w, d_s = _dev(recv.reshape(-1)), _full(batch * d + 8, 0x5A)
    mz.rs_syndromes_dev(n, k, d_w.data_ptr(), batch, d_s.data_ptr(), _stream())
    s = _host(d_s)
    assert np.array_equal(s[:batch * d].reshape(batch, d), syn) and (s[batch * d:] == 0x5A).all()


def test_miscorrection_is_the_models(mz):
    """more than t errors within t of another codeword: status <= t, the word a codeword, but not the one that was sent"""
    n, k = C.MISCORRECTION_CODE
    words, want = C.miscorrection_words(), C.miscorrection_expected()
    got_c, got_m, got_s = mz.rs_decode(n, k, _u8([w[1] for w in words]), with_corrected=True)
    assert got_s.tolist() == [w[2] for w in want]
    assert np.array_equal(got_c, _u8([w[0] for w in want]))
    assert np.array_equal(got_m, _u8([w[1] for w in want]))
    wrong = [i for i, (w, x) in enumerate(zip(words, want)) if x[2] != 255 and got_c[i].tolist() != list(w[0])]
    assert len(wrong) >= 3 and not mz.rs_syndromes(n, k, got_c[wrong]).any()


# ---- 2D -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, pattern", C.CASES_2D, ids=_ids([s + (p,) for s, p in C.CASES_2D]))
def test_2d_encode_and_decode_with_statuses(mz, shape, pattern):
    col_n, row_n, ml = shape
    data, code, hit, (want, wcs, wrs) = C.case_2d(shape, pattern)
    if pattern == "A":                                                      # the encoder once per shape
        assert np.array_equal(mz.rs2d_encode(col_n, row_n, list(data)), _u8(code))
    got, cs, rs_ = mz.rs2d_decode(col_n, row_n, _u8(hit), ml, with_status=True)
    assert cs.tolist() == wcs and rs_.tolist() == wrs
    assert (None if got is None else got.tolist()) == want
    assert (mz.rs2d_decode(col_n, row_n, _u8(hit), ml) is None) == (want is None)          # `ok` without the statuses asked for


def _dev_round_trip(mz, shape, pattern, with_status):
    import torch
    col_n, row_n, ml = shape
    size = C.M.isqrt_ceil(ml)
    data, code, hit, (want, wcs, wrs) = C.case_2d(shape, pattern)
    d_d = _dev(_u8(data))
    d_code = _full(col_n * row_n + 8, 0xC3)                                # every byte of the code is written, none behind it
    mz.rs2d_encode_dev(col_n, row_n, d_d.data_ptr(), ml, d_code.data_ptr(), _stream())
    c = _host(d_code)
    assert np.array_equal(c[:col_n * row_n].reshape(col_n, row_n), _u8(code)) and (c[col_n * row_n:] == 0xC3).all()
    d_hit = _dev(_u8(hit).reshape(-1))
    d_back, d_cs, d_rs = _full(ml + 8, 0xC3), _full(row_n + 8, 0xC3), _full(size + 8, 0xC3)
    d_ok = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    mz.rs2d_decode_dev(col_n, row_n, d_hit.data_ptr(), ml, d_back.data_ptr(), d_ok.data_ptr() + 4, d_cs.data_ptr() if with_status else None,
                       d_rs.data_ptr() if with_status else None, _stream())
    back, cs, rs_, ok = _host(d_back), _host(d_cs), _host(d_rs), _host(d_ok)
    assert ok.tolist() == [-7, int(want is not None), -7]
    if want is not None:
        assert back[:ml].tolist() == want
    assert (back[ml:] == 0xC3).all()
    if with_status:
        assert cs[:row_n].tolist() == wcs and rs_[:size].tolist() == wrs
        assert (cs[row_n:] == 0xC3).all() and (rs_[size:] == 0xC3).all()
    else:
        assert (cs == 0xC3).all() and (rs_ == 0xC3).all()
    assert np.array_equal(_host(d_hit).reshape(col_n, row_n), _u8(hit))    # the received code is only read


@pytest.mark.parametrize("shape", C.SHAPES, ids=_ids(C.SHAPES))
def test_2d_device_forms(mz, shape):
    _dev_round_trip(mz, shape, "A", True)


@pytest.mark.parametrize("pattern", ["A", "C"])
def test_2d_device_forms_without_status_pointers(mz, pattern):
    _dev_round_trip(mz, (20, 12, 64), pattern, False)


# ---- encoders -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", C.WAVE_K)
def test_wave_encoder_at_the_chunk_boundaries(mz, k):
    n = k + C.WAVE_D
    msgs, code = C.encode_case(n, k, C.WAVE_BATCH)
    assert np.array_equal(mz.rs_encode(n, k, _u8(msgs)), _u8(code))


@pytest.mark.parametrize("k", C.WAVE_K_STRIDED)
def test_wave_encoder_strided(mz, k):
    n, batch = k + C.WAVE_D, C.WAVE_BATCH
    msgs, code = C.encode_case(n, k, batch)
    mc, cc = 2 * k + 3, 2 * n + 5
    src = np.full(batch * mc, 0xAA, dtype=np.uint8)
    want = np.full(batch * cc, 0x55, dtype=np.uint8)
    for b in range(batch):
        src[b * mc: b * mc + 2 * k: 2] = msgs[b]
        want[b * cc: b * cc + 2 * n: 2] = code[b]
    d_src, d_dst = _dev(src), _full(batch * cc, 0x55)
    mz.rs_encode_view_dev(n, k, d_src.data_ptr(), 2, mc, batch, d_dst.data_ptr(), 2, cc, None, _stream())
    assert np.array_equal(_host(d_dst), want)


@pytest.mark.parametrize("n, k", C.LANE_CODES, ids=_ids(C.LANE_CODES))
def test_lane_encoder_word_path_and_byte_path_agree_with_the_model(mz, n, k):
    """the same messages through the 32-bit path (everything aligned) and through the byte path that a view takes when it misses only
    the alignment: the message base, the output base or the codeword stride"""
    batch = C.LANE_BATCH
    msgs, code = C.encode_case(n, k, batch)
    guard = 16
    for name, moff, ooff, extra in C.LANE_PLACEMENTS:
        cc = n + extra
        src = np.full(guard + moff + batch * k + guard, 0xAA, dtype=np.uint8)
        src[guard + moff: guard + moff + batch * k] = _u8(msgs).reshape(-1)
        want = np.full(guard + ooff + batch * cc + guard, 0x55, dtype=np.uint8)
        for b in range(batch):
            want[guard + ooff + b * cc: guard + ooff + b * cc + n] = code[b]
        d_src, d_dst = _dev(src), _full(len(want), 0x55)
        assert d_src.data_ptr() % 4 == 0 and d_dst.data_ptr() % 4 == 0
        mz.rs_encode_view_dev(n, k, d_src.data_ptr() + guard + moff, 1, k, batch, d_dst.data_ptr() + guard + ooff, 1, cc, None, _stream())
        assert np.array_equal(_host(d_dst), want), name
        assert np.array_equal(_host(d_src), src), name
