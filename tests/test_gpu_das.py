"""Celestia's commitment on the device (myzkp_amd/csrc/mzk_das.hip) against tests/das_model.py, bit for bit, on the tables of
tests/das_cases.py (which tests/test_das_cases.py checks without a GPU):

  * row roots, column roots and data roots of every shape: host form; device form on strided views with guard bytes around the input
    and every output; NULL row / column outputs; workgroups that straddle squares (65 squares of small sides);
  * the same roots from mzk_merkle_commit_bytes, the path this call replaces;
  * the handle: built on the stream that produced its input with no synchronisation, roots, every position of small grids in both
    directions and 512 seeded positions of 255 x 255 x 3 -- depths, entry lengths, entries, leaves, depth-0 samples --, open against
    open_dev, two handles alive, positions out of range;
  * mzk_rs2d_encode_dev -> mzk_das_grid_build_dev on one stream.

What "verifies" means.  The reference's Merkle::verify (merkle.rs:49-66) reads left / right off the bits of the index.  That is the
shape of the tree only when every split is even: on a ragged tree it rejects the reference's own path for most leaves (n = 3: two of
the two openable leaves).  So every non-zero-depth path is checked with das_model.verify_shaped, which follows the splits of
Merkle::commit, against the returned root, and with the reference's verify wherever the leaf count is a power of two -- the only
trees whose paths the reference itself accepts, Celestia's own 16 x 16 test among them."""
import ctypes
import functools
import numpy as np
import pytest
import das_cases as C
import das_model as M

pytestmark = pytest.mark.gpu
SEED = 11
GUARD = 32          # bytes around every device buffer; keeps the 16-byte alignment of the outputs


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init_devices([0])
    yield m
    m.init_devices([0])


@functools.lru_cache(maxsize=None)
def _model(rows, cols):
    """the model's commitment of every square of the shape, computed once: (squares, [(row_roots, col_roots, data_root)])"""
    m = C.squares(rows, cols, C.max_count(rows, cols), SEED)
    return m, [M.celestia_commit(sq.tolist()) for sq in m]


def _want(rows, cols, count):
    m, commits = _model(rows, cols)
    rr = np.array([[list(x) for x in c[0]] for c in commits[:count]], dtype=np.uint8)
    cr = np.array([[list(x) for x in c[1]] for c in commits[:count]], dtype=np.uint8)
    dr = np.array([list(c[2]) for c in commits[:count]], dtype=np.uint8)
    return m[:count], rr, cr, dr


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _guarded(nbytes, fill):
    """a device buffer of nbytes between two guards: (whole tensor, pointer of the payload)"""
    import torch
    t = torch.full((nbytes + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda")
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + GUARD


def _payload(t):
    import torch
    torch.cuda.synchronize()
    a = t.cpu().numpy()
    return a[GUARD:-GUARD], np.concatenate([a[:GUARD], a[-GUARD:]])


def _ids(cases):
    return ["%dx%dx%d" % c for c in cases]


@pytest.mark.parametrize("rows,cols,count", C.commit_cases(), ids=_ids(C.commit_cases()))
def test_commit_host_form(mz, rows, cols, count):
    m, rr, cr, dr = _want(rows, cols, count)
    got = mz.das_commit(m)
    assert np.array_equal(got[2], dr) and np.array_equal(got[0], rr) and np.array_equal(got[1], cr)


@pytest.mark.parametrize("rows,cols,count", C.commit_cases(), ids=_ids(C.commit_cases()))
def test_commit_device_form_strided_between_guards(mz, rows, cols, count):
    import torch
    m, rr, cr, dr = _want(rows, cols, count)
    row_stride = cols + 3
    square_stride = (rows - 1) * row_stride + cols + 5
    view = np.full(count * square_stride, 0xA5, dtype=np.uint8)
    for q in range(count):
        for r in range(rows):
            at = q * square_stride + r * row_stride
            view[at:at + cols] = m[q, r]
    d_in, p_in = _guarded(len(view), 0xA5)
    d_in[GUARD:GUARD + len(view)] = torch.from_numpy(view).cuda()
    before = d_in.clone()
    d_r, p_r = _guarded(count * rows * 32, 0xC3)
    d_c, p_c = _guarded(count * cols * 32, 0xC3)
    d_d, p_d = _guarded(count * 32, 0xC3)
    mz.das_commit_dev(p_in, rows, cols, row_stride, square_stride, count, p_r, p_c, p_d, _stream())
    for t, want in ((d_r, rr), (d_c, cr), (d_d, dr)):
        got, guards = _payload(t)
        assert np.array_equal(got, want.reshape(-1)) and (guards == 0xC3).all()
    assert torch.equal(d_in, before)


@pytest.mark.parametrize("rows,cols,count", [(3, 5, 65), (33, 33, 2), (255, 2, 3), (128, 129, 1)], ids=_ids([(3, 5, 65), (33, 33, 2), (255, 2, 3), (128, 129, 1)]))
def test_commit_device_form_without_row_and_column_outputs(mz, rows, cols, count):
    import torch
    m = C.squares(rows, cols, count, SEED)
    want = np.array([list(M.celestia_commit(sq.tolist())[2]) for sq in m], dtype=np.uint8)
    d_in = torch.from_numpy(m).cuda()
    d_d, p_d = _guarded(count * 32, 0xC3)
    d_r, p_r = _guarded(count * rows * 32, 0xC3)
    mz.das_commit_dev(d_in.data_ptr(), rows, cols, cols, rows * cols, count, None, None, p_d, _stream())
    got, guards = _payload(d_d)
    assert np.array_equal(got, want.reshape(-1)) and (guards == 0xC3).all()
    # one of the two only
    d_d2, p_d2 = _guarded(count * 32, 0xC3)
    mz.das_commit_dev(d_in.data_ptr(), rows, cols, cols, rows * cols, count, p_r, None, p_d2, _stream())
    assert np.array_equal(_payload(d_d2)[0], want.reshape(-1))
    rr = np.array([[list(x) for x in M.celestia_commit(sq.tolist())[0]] for sq in m], dtype=np.uint8)
    got_r, guards_r = _payload(d_r)
    assert np.array_equal(got_r, rr.reshape(-1)) and (guards_r == 0xC3).all()


@pytest.mark.parametrize("rows,cols,count", C.TIE_SHAPES, ids=_ids(C.TIE_SHAPES))
def test_roots_equal_the_byte_leaf_commit_they_replace(mz, rows, cols, count):
    m = C.squares(rows, cols, count, SEED)
    rr, cr, dr = mz.das_commit(m)
    L = mz.lib()

    def old(leaves):
        leaves = np.ascontiguousarray(leaves, dtype=np.uint8)
        off = np.arange(len(leaves) + 1, dtype=np.uint64)
        root, n = np.zeros(32, dtype=np.uint8), ctypes.c_size_t(0)
        assert L.mzk_merkle_commit_bytes(leaves.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(leaves)),
                                         root.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(32), ctypes.byref(n)) == 0
        assert n.value == 32
        return root

    for q in range(count):
        for r in range(rows):
            assert np.array_equal(old(m[q, r]), rr[q, r]), (q, r)
        for c in range(cols):
            assert np.array_equal(old(m[q, :, c]), cr[q, c]), (q, c)
        roots = np.concatenate([rr[q].reshape(-1), cr[q].reshape(-1)])
        off = (32 * np.arange(rows + cols + 1)).astype(np.uint64)
        root, n = np.zeros(32, dtype=np.uint8), ctypes.c_size_t(0)
        assert L.mzk_merkle_commit_bytes(roots.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(rows + cols),
                                         root.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(32), ctypes.byref(n)) == 0
        assert np.array_equal(root, dr[q])


# ---- the handle ----------------------------------------------------------------------------------------------------------------------
def _expect_open(m, commits, pos):
    """what the model says of every position: (paths, entry_lens, depths, leaves) as the ABI lays them out"""
    n = len(pos)
    paths, lens = np.zeros((n, 8, 32), dtype=np.uint8), np.zeros((n, 8), dtype=np.uint8)
    depths, leaves = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    for s, (q, r, c, is_row) in enumerate(pos.tolist()):
        sq = m[q].tolist()
        path = M.celestia_open(sq, r, c, bool(is_row))
        leaves[s] = sq[r][c]
        if path is None:
            continue
        depths[s] = len(path)
        for k, e in enumerate(path):
            lens[s, k] = len(e)
            paths[s, k, :len(e)] = list(e)
    return paths, lens, depths, leaves


def _check_open(m, got_roots, pos, got):
    """every non-zero-depth path authenticates its leaf against the RETURNED root (see the module docstring)"""
    paths, lens, depths, leaves = got
    rr, cr, _ = got_roots
    rows, cols = m.shape[1:]
    for s, (q, r, c, is_row) in enumerate(pos.tolist()):
        d = int(depths[s])
        if d == 0:
            continue
        path = [bytes(paths[s, k, :lens[s, k]]) for k in range(d)]
        root = bytes(rr[q, r]) if is_row else bytes(cr[q, c])
        index, n = (c, cols) if is_row else (r, rows)
        leaf = bytes([leaves[s]])
        assert M.verify_shaped(root, index, n, path, leaf), (q, r, c, is_row)
        if n & (n - 1) == 0:
            assert M.verify(root, index, path, leaf), (q, r, c, is_row)


def _build_on_a_side_stream(mz, m):
    """the input is produced on a side stream and the handle built behind it with no synchronisation in between"""
    import torch
    count, rows, cols = m.shape
    side = torch.cuda.Stream()
    host = torch.from_numpy(m ^ 0xFF).pin_memory()
    with torch.cuda.stream(side):
        d = host.to("cuda", non_blocking=True)
        d = d ^ 0xFF                                        # the square itself, written by a kernel of this stream
        g = mz.DasGrid.from_device(d.data_ptr(), rows, cols, cols, rows * cols, count, side.cuda_stream)
    return g, d


@pytest.mark.parametrize("n", C.OPEN_ALL_SIDES)
def test_handle_opens_every_position_in_both_directions(mz, n):
    import torch
    count = 2
    m, rr, cr, dr = _want(n, n, count)
    g, keep = _build_on_a_side_stream(mz, m)
    roots = g.roots()
    assert np.array_equal(roots[0], rr) and np.array_equal(roots[1], cr) and np.array_equal(roots[2], dr)
    pos = C.positions_all(n, n, count)
    got = g.open(pos)
    want = _expect_open(m, None, pos)
    for a, b, what in zip(got, want, ("paths", "entry_lens", "depths", "leaves")):
        assert np.array_equal(a, b), what
    assert set(np.flatnonzero(got[2] == 0).tolist()) == {s for s, (q, r, c, d) in enumerate(pos.tolist()) if (c if d else r) in M.nonterminating(n)}
    _check_open(m, roots, pos, got)
    # the device form, on its own stream, behind the build
    d_pos = torch.from_numpy(pos.astype(np.int64)).cuda()
    k = len(pos)
    d_paths, d_lens = torch.full((k * 256,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((k * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    d_dep, d_leaf = torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda")
    g.open_dev(d_pos.data_ptr(), k, d_paths.data_ptr(), d_lens.data_ptr(), d_dep.data_ptr(), d_leaf.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert np.array_equal(d_paths.cpu().numpy().reshape(k, 8, 32), got[0]) and np.array_equal(d_lens.cpu().numpy().reshape(k, 8), got[1])
    assert np.array_equal(d_dep.cpu().numpy(), got[2]) and np.array_equal(d_leaf.cpu().numpy(), got[3])
    g.close()


def test_handle_opens_seeded_positions_of_the_largest_grid(mz):
    rows, cols, count, k = C.OPEN_SAMPLED
    m, rr, cr, dr = _want(rows, cols, count)
    g = mz.DasGrid(m)
    roots = g.roots()
    assert np.array_equal(roots[0], rr) and np.array_equal(roots[1], cr) and np.array_equal(roots[2], dr)
    pos = C.positions_sampled(rows, cols, count, k, seed=7)
    got = g.open(pos)
    want = _expect_open(m, None, pos)
    for a, b, what in zip(got, want, ("paths", "entry_lens", "depths", "leaves")):
        assert np.array_equal(a, b), what
    assert 0 < int((got[2] == 0).sum()) < k / 3
    _check_open(m, roots, pos, got)
    g.close()


def test_two_handles_alive_and_positions_out_of_range(mz):
    import torch
    ma, mb = C.squares(5, 3, 2, SEED), C.squares(16, 16, 1, SEED)
    ga, gb = mz.DasGrid(ma), mz.DasGrid(mb)
    ra, rb = ga.roots(), gb.roots()
    assert np.array_equal(ra[2], _want(5, 3, 2)[3]) and np.array_equal(rb[2], _want(16, 16, 1)[3])
    pa, pb = C.positions_all(5, 3, 2), C.positions_all(16, 16, 1)
    oa, ob = ga.open(pa), gb.open(pb)
    for a, b in zip(oa, _expect_open(ma, None, pa)):
        assert np.array_equal(a, b)
    for a, b in zip(ob, _expect_open(mb, None, pb)):
        assert np.array_equal(a, b)
    assert (ob[2] == 4).all()
    # host form: one bad position refuses the whole call and names it
    for bad in ((2, 0, 0, 1), (0, 5, 0, 0), (0, 0, 3, 1), (0, 0, 0, 2)):
        with pytest.raises(mz.MzkError) as e:
            ga.open(np.array([(0, 0, 0, 1), bad], dtype=np.uint64))
        assert e.value.code == -1 and "position 1" in e.value.message
    # device form: depths = 255 for that sample and nothing else of it; its neighbours as ever
    pos = np.array([(1, 4, 2, 0), (2, 0, 0, 1), (0, 1, 1, 1), (0, 5, 0, 0), (0, 0, 3, 1), (0, 0, 0, 2)], dtype=np.uint64)
    k = len(pos)
    d_pos = torch.from_numpy(pos.astype(np.int64)).cuda()
    d_paths, d_lens = torch.full((k * 256,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((k * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    d_dep, d_leaf = torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda"), torch.full((k,), 0xEE, dtype=torch.uint8, device="cuda")
    ga.open_dev(d_pos.data_ptr(), k, d_paths.data_ptr(), d_lens.data_ptr(), d_dep.data_ptr(), d_leaf.data_ptr(), _stream())
    torch.cuda.synchronize()
    paths, lens = d_paths.cpu().numpy().reshape(k, 8, 32), d_lens.cpu().numpy().reshape(k, 8)
    dep, leaf = d_dep.cpu().numpy(), d_leaf.cpu().numpy()
    good = ga.open(pos[[0, 2]])
    for s, j in ((0, 0), (2, 1)):
        assert np.array_equal(paths[s], good[0][j]) and np.array_equal(lens[s], good[1][j]) and dep[s] == good[2][j] and leaf[s] == good[3][j]
    for s in (1, 3, 4, 5):
        assert dep[s] == mz.DAS_OUT_OF_RANGE and (paths[s] == 0xEE).all() and (lens[s] == 0xEE).all() and leaf[s] == 0xEE
    ga.close()
    assert np.array_equal(gb.open(pb)[0], ob[0])           # the other handle lives on
    gb.close()


def test_refusals_reach_the_caller_with_their_text(mz):
    import torch
    d = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    for args, word in (((1, 8, 8, 8, 1), "rows"), ((8, 256, 256, 2048, 1), "cols"), ((8, 8, 7, 64, 1), "row_stride"), ((8, 8, 8, 63, 2), "square_stride"),
                       ((8, 8, 8, 64, 0), "squares")):
        with pytest.raises(mz.MzkError) as e:
            mz.das_commit_dev(p, *args, p + 1024, p + 2048, p + 3072, _stream())
        assert e.value.code == -1 and word in e.value.message
        with pytest.raises(mz.MzkError) as e:
            mz.DasGrid.from_device(p, *args, _stream())
        assert e.value.code == -1 and word in e.value.message
    with pytest.raises(mz.MzkError) as e:
        mz.das_commit_dev(p, 8, 8, 8, 64, 1, p + 1024 + 4, p + 2048, p + 3072, _stream())
    assert e.value.code == -1 and "aligned" in e.value.message
    torch.cuda.synchronize()
    assert not d.any()


@pytest.mark.parametrize("chunk,side,message_len", C.PIPELINE, ids=["celestia_test", "255x255"])
def test_encode_then_build_on_one_stream(mz, chunk, side, message_len):
    import torch
    import rs_model as R
    data = (np.arange(message_len) % 256).astype(np.uint8) if message_len == 64 else np.random.default_rng(5).integers(0, 256, message_len, dtype=np.uint8)
    assert chunk * chunk == message_len
    code = np.array(R.encode_rs2d(data.tolist(), R.setup_rs2d(side, side, message_len)), dtype=np.uint8)
    want = M.celestia_commit(code.tolist())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_data = torch.from_numpy(data).cuda()
        d_code = torch.zeros(side * side, dtype=torch.uint8, device="cuda")
        mz.rs2d_encode_dev(side, side, d_data.data_ptr(), message_len, d_code.data_ptr(), s.cuda_stream)
        g = mz.DasGrid.from_device(d_code.data_ptr(), side, side, side, side * side, 1, s.cuda_stream)
    rr, cr, dr = g.roots()
    assert bytes(dr[0]) == want[2]
    assert [bytes(x) for x in rr[0]] == want[0] and [bytes(x) for x in cr[0]] == want[1]
    torch.cuda.synchronize()
    assert np.array_equal(d_code.cpu().numpy().reshape(side, side), code)
    if message_len == 64:                                   # the reference's own test_celestia positions, then the malicious one
        pos = np.array([(0, i // 12, i % 12, 0) for i in range(10)], dtype=np.uint64)
        got = g.open(pos)
        _check_open(code.reshape(1, side, side), (rr, cr, dr), pos, got)
        assert (got[2] == 4).all()
        mal = np.array(R.encode_rs2d(list(range(1, 65)), R.setup_rs2d(side, side, 64)), dtype=np.uint8)
        gm = mz.DasGrid(mal)
        p, l, d, leaf = gm.open(np.array([(0, 0, 0, 0)], dtype=np.uint64))
        path = [bytes(p[0, k, :l[0, k]]) for k in range(int(d[0]))]
        assert not M.verify(bytes(cr[0, 0]), 0, path, bytes([leaf[0]]))
        gm.close()
    g.close()
