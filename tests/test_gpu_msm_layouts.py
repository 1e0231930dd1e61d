"""KZG commits through every window-table layout a caller can ask for -- mzk_srs_from_device_ex at 8..22 bits, and 14..17 bits with the
two and four bucket sets a table budget degrades them to (msm_layouts.LAYOUTS: 23) -- at the coefficient counts on both sides of every
threshold between the MSM's sort and accumulate paths (msm_layouts.PREFIXES).  One handle of 2^15 points per layout, one scalar vector
for all of them (msm_layouts.scalar_vector: every edge of the signed-digit recoding at every width, repeats, P next to -P, equal
scalars, zeros) over points with repeats, negated neighbours and points at infinity; every commitment bit for bit against the oracle's
Pippenger, with the path msm_plan gives the call and the phases that ran asserted beside it.

Memory: the widest layout (22 bits) has 2^21 buckets -- 256 MiB of buckets and about 300 MiB of segment slots, the order of what
test_srs_tables_with_explicit_window_width (test_gpu_dev_api.py) already takes."""
import ctypes
import numpy as np
import pytest
import orc
import msm_layouts
from msm_layouts import N_SRS, PREFIXES, LAYOUTS, EXPECTED_PATH, PATH_ID, SCAN, SSORT, rows
from test_gpu_seg_accumulate_pipeline import mz, plan      # fixtures: the library; msm_plan at the device's own CU count

pytestmark = pytest.mark.gpu

TABLES = 2
PH_MSM_SORT, PH_MSM_COMBINE, PH_MSM_SEG_COMBINE = 1, 4, 11      # include/mzk.h
PARTIAL_AT = (4097, 32768)


def layout_points():
    """edge_points of test_gpu_seg_accumulate_pipeline.py, spread: a run of repeats, P next to -P and points at infinity inside the prefix
    of 300 and behind it, on the rows where msm_layouts.scalar_vector repeats its scalars; infinity as the last point of three prefixes"""
    p = orc.synth_points(2301, N_SRS)
    neg = lambda row: orc.to_limbs([orc.P_FQ - orc.from_limbs(row[None, 4:])[0]], 4)[0]
    p[20:36] = p[20]
    p[50] = p[51]
    p[50, 4:] = neg(p[51])
    p[90:94] = 0
    lo, hi = msm_layouts.REPEAT_POINT
    p[lo:hi] = p[lo]
    a, b = msm_layouts.NEG_PAIR
    p[a] = p[b]
    p[a, 4:] = neg(p[b])
    p[msm_layouts.EQUAL_BLOCK[0] + 7] = 0
    p[299] = 0
    p[4095] = 0
    p[N_SRS - 1] = 0
    return p


@pytest.fixture(scope="module")
def data(mz):
    """points, scalars, their device copies and the oracle's commitment of every prefix: computed once, never written again"""
    import torch
    p = layout_points()
    s = orc.to_limbs(msm_layouts.scalar_vector(orc.from_limbs(orc.synth_vector(orc.FR, 2302, N_SRS))), 4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()
    want = {m: orc.msm_fast(s[:m], p[:m]) for m in PREFIXES}
    return dev(p), dev(s), want


def phase_pairs(L, call):
    """event pairs per phase while `call` runs (pass_launches of test_gpu_ntt_splits.py)"""
    assert L.mzk_prof_select(ctypes.c_uint32(0xffffffff)) == 0
    assert L.mzk_prof_enable(1) == 0
    try:
        assert L.mzk_prof_reset() == 0
        got = call()
        out = {}
        for ph in (PH_MSM_SORT, PH_MSM_SEG_COMBINE, PH_MSM_COMBINE):
            ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
            assert L.mzk_prof_read(ph, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            out[ph] = cnt.value
        return got, out
    finally:
        L.mzk_prof_enable(0)
        L.mzk_prof_reset()


@pytest.mark.parametrize("c,sets", LAYOUTS, ids=["%d-bit-%d-set" % l for l in LAYOUTS])
def test_commit_through_the_layout_at_every_prefix(mz, plan, data, c, sets):
    import torch
    L = mz.lib()
    d_p, d_s, want = data
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ok = lambda rc: rc == 0 or pytest.fail(L.mzk_last_error().decode())
    table_bytes = rows(c, sets) * N_SRS * 64
    kind = TABLES | (c << 8) | (sets << 16)
    h = ctypes.c_void_p()
    try:
        if sets > 1:        # the s-set layout fits this budget exactly; the richer ones (19/10/5, 17/9/5, 16/8/4, 15/8/4 rows at 14..17 bits) do not
            ok(L.mzk_set_table_budget(ctypes.c_size_t(table_bytes)))
        ok(L.mzk_srs_from_device_ex(ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(N_SRS), ctypes.c_int(c), ctypes.byref(h), st))
        assert (L.mzk_srs_window_bits(h), L.mzk_srs_bucket_sets(h), L.mzk_srs_table_bytes(h)) == (c, sets, table_bytes)

        def commit(m, partial=0):
            d_o = torch.full((16,), -1, dtype=torch.int64, device="cuda")
            ok(L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_s.data_ptr()), ctypes.c_size_t(m), ctypes.c_void_p(d_o.data_ptr()), partial, st))
            if partial:     # the XYZZ record of a shard: folded like the multi-GPU path folds it
                d_f = torch.full((8,), -1, dtype=torch.int64, device="cuda")
                ok(L.mzk_g1_fold_partials_dev(ctypes.c_void_p(d_o.data_ptr()), ctypes.c_int(1), ctypes.c_void_p(d_f.data_ptr()), st))
                d_o = d_f
            torch.cuda.synchronize()
            return mz.array_to_points(d_o[:8].cpu().numpy().view(np.uint64).reshape(1, 8))[0]

        repeated = set()
        for m, path in zip(PREFIXES, EXPECTED_PATH[(c, sets)]):
            where = (c, sets, m, path)
            assert plan(m, kind, N_SRS)["path"] == PATH_ID[path], where
            got, pairs = phase_pairs(L, lambda: commit(m))
            assert got == want[m], where
            assert pairs[PH_MSM_SORT] == (0 if path == SCAN else 1), (where, pairs)
            assert pairs[PH_MSM_SEG_COMBINE] == (0 if path in (SCAN, SSORT) else 1), (where, pairs)
            assert pairs[PH_MSM_COMBINE] == (1 if sets > 1 else 0), (where, pairs)
            if path not in repeated:        # twice in a row on the same handle: every workspace slot is the one the first call sized
                repeated.add(path)
                assert commit(m) == want[m], (where, "second call")
            if m in PARTIAL_AT:
                got, pairs = phase_pairs(L, lambda: commit(m, partial=1))
                assert got == want[m] and pairs[PH_MSM_COMBINE] == (1 if sets > 1 else 0), (where, "partial", pairs)
    finally:
        L.mzk_set_table_budget(ctypes.c_size_t(0))
        if h:
            torch.cuda.synchronize()
            L.mzk_srs_free(h)
