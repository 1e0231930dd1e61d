"""One constructor behind every way to an SRS handle (srs_new, mzk_srs.h): the same points through mzk_srs_upload,
mzk_srs_from_device_ex and mzk_srs_save then mzk_srs_load with the stored tables must give handles that report the same layout, commit
to the oracle's point and hand the same points back -- at every default window width, for an empty handle, and where a table budget
degrades the layout.  Direct tables attach once per width and leave with mzk_srs_drop_direct."""
import ctypes, functools
import numpy as np
import pytest
import orc
from orc import FR

pytestmark = pytest.mark.gpu
BIG = (1 << 15) + 5


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


@functools.lru_cache(maxsize=None)
def case(n):
    """points (one of them infinity), scalars and the oracle's commitment, computed once per size and never written to"""
    p = orc.synth_points(3100 + n, n)
    if n > 10:
        p[7] = 0
    s = orc.synth_vector(FR, 3101 + n, n)
    for a in (p, s):
        a.setflags(write=False)
    return p, s, (orc.msm_fast(s, p) if n else (0, 0))


def layout(L, h):
    return L.mzk_srs_window_bits(h._h), L.mzk_srs_bucket_sets(h._h), L.mzk_srs_table_bytes(h._h)


def from_device(mz, p, with_tables=1):
    import torch
    L = mz.lib()
    d = torch.from_numpy(np.ascontiguousarray(p).view(np.int64).reshape(-1).copy()).cuda() if p.size else torch.zeros(8, dtype=torch.int64, device="cuda")
    h = mz.Srs.__new__(mz.Srs)
    h._h, h.n = ctypes.c_void_p(), p.shape[0]
    rc = L.mzk_srs_from_device_ex(d.data_ptr(), h.n, with_tables, ctypes.byref(h._h), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    return h


def check_all(mz, handles, n, want_layout):
    L = mz.lib()
    p, s, want = case(n)
    for how, h in handles.items():
        assert h.n == n and L.mzk_srs_len(h._h) == n, how
        assert layout(L, h) == want_layout, how
        assert h.commit(s) == want, how
        assert np.array_equal(h.download(), p), how


@pytest.mark.parametrize("n,bits", [(0, 0), (1, 8), (300, 8), (5000, 10), (BIG, 16)])
def test_upload_from_device_and_load_give_the_same_handle(mz, tmp_path, n, bits):
    p = case(n)[0]
    path = str(tmp_path / "srs.bin")
    handles = {"upload": mz.Srs(p), "from_device_ex": from_device(mz, p)}
    handles["upload"].save(path, with_tables=True)
    handles["load"] = mz.Srs.load(path, with_tables=1)
    rows = 254 // bits + 1 if bits else 0                                # an empty handle has no tables and no bytes
    check_all(mz, handles, n, (bits, 1 if bits else 0, rows * n * 64))
    for h in handles.values():
        h.close()


def test_the_three_constructors_degrade_alike_under_a_table_budget(mz, tmp_path):
    """9 n 64 bytes: the 16 tables of 16-bit windows do not fit, every second one does.  The dump holds all 16: the loader finds them
    over the budget and builds the layout that fits from the points, as the other two do."""
    L = mz.lib()
    n = BIG
    p = case(n)[0]
    path = str(tmp_path / "full.bin")
    full = mz.Srs(p)
    full.save(path, with_tables=True)
    full.close()
    handles = {}
    try:
        L.mzk_set_table_budget(9 * n * 64)
        handles = {"upload": mz.Srs(p), "from_device_ex": from_device(mz, p), "load": mz.Srs.load(path, with_tables=1)}
        check_all(mz, handles, n, (16, 2, 8 * n * 64))
    finally:
        L.mzk_set_table_budget(0)
        for h in handles.values():
            h.close()


def test_direct_tables_attach_once_per_width_and_drop(mz):
    L = mz.lib()
    n = 5000
    p, s, _ = case(n)
    h = mz.Srs(p)
    own = 26 * n * 64
    direct = 32 * n * 128 * 64                                           # 8-bit windows: 32 of them, 2^7 multiples each
    assert layout(L, h) == (10, 1, own) and L.mzk_srs_direct_bits(h._h) == 0
    assert h.build_direct(8, 2 << 30) == 8
    assert L.mzk_srs_table_bytes(h._h) == own + direct
    rows = s[:4 * 64].reshape(4, 64, 4)
    want = [orc.msm_fast(rows[k], p[:64]) for k in range(4)]
    assert h.commit_many(rows) == want
    assert h.build_direct(8, 2 << 30) == 8                               # the same width again: nothing is rebuilt
    assert L.mzk_srs_table_bytes(h._h) == own + direct and h.commit_many(rows) == want
    h.drop_direct()
    assert layout(L, h) == (10, 1, own) and L.mzk_srs_direct_bits(h._h) == 0
    assert h.commit_many(rows) == want                                   # the window tables serve again
    h.drop_direct()                                                      # nothing to drop
    assert L.mzk_srs_table_bytes(h._h) == own
    h.close()
