"""The MSM's host-side plan (myzkp_amd/csrc/mzk_msm_plan.h), compiled for the host with g++ through a small shim
(tests/hostcheck/msm_plan_shim.cpp): which path a call takes, which layout, and what it asks of the workspace.  CPU only."""
import ctypes, os, random, subprocess
import pytest
import msm_layouts

HERE = os.path.dirname(os.path.abspath(__file__))
PLAIN, MONT, TABLES = 0, 1, 2
SMALL_SCAN, SMALL_SORT, TWO_LEVEL, LDS_ONE_PASS, ATOMIC = range(5)
SLOTS = ("points", "counts", "offsets", "cursor", "entries", "buckets", "scan", "slots", "wghist", "out")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("msm_plan") / "libmsmplan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "msm_plan_shim.cpp")])
    L = ctypes.CDLL(so)
    L.plan_fields.restype = ctypes.c_char_p
    L.plan.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int,
                       ctypes.POINTER(ctypes.c_uint64)]
    L.chunkable.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64]
    L.names = L.plan_fields().decode().split()
    return L


def plan(L, n, kind, stride, n_shape=None, n_alloc=None, chunks=0, num_cu=256):
    out = (ctypes.c_uint64 * len(L.names))()
    assert L.plan(n, n_shape or n, n_alloc or n, kind, stride, num_cu, chunks, out) == len(L.names)
    return dict(zip(L.names, out))


def tables(c, sets=1):
    return TABLES | (c << 8) | (sets << 16)


def layouts():
    yield PLAIN, 0
    yield MONT, 1
    for c in range(8, 23):
        for sets in (1, 2, 4):
            yield tables(c, sets), 1


def stride_for(kind, n):
    return 0 if kind == PLAIN else n


CHUNK_SIZES = (1 << 18, (1 << 18) + 1, 3 * (1 << 20) - 5, 1 << 22, 1 << 24, 1 << 27)


def test_chunkable_problems_take_the_two_level_sort(lib):
    """chunk mode stops after the segment combine of the two-level sort: msm_chunkable promises that path to every chunk"""
    for kind, _ in layouts():
        for n in CHUNK_SIZES:
            stride = stride_for(kind, n)
            if not lib.chunkable(n, kind, stride):
                continue
            whole = plan(lib, n, kind, stride)
            assert whole["err"] == 0 and whole["path"] == TWO_LEVEL and whole["sets"] == 1, (hex(kind), n)
            assert plan(lib, n, kind, stride, chunks=2)["err"] == 0
    # narrow window tables (2^(c-1) <= 2048 buckets) sort in one pass: they are not chunked; the generic layout always is
    for n in CHUNK_SIZES:
        assert lib.chunkable(n, PLAIN, 0) and lib.chunkable(n, MONT, n), n
        for c in range(8, 13):
            assert not lib.chunkable(n, tables(c), n), (c, n)
        assert not lib.chunkable(n, tables(16, 2), n)
    for c in range(13, 23):
        assert lib.chunkable(1 << 18, tables(c), 1 << 18), c
    assert not lib.chunkable((1 << 18) - 1, PLAIN, 0)


def splits(n, rng):
    """host_chunk_plan's pieces (quarters; a quarter and the rest) and ragged ones of >= 4097 pairs"""
    yield [n // 4 & ~4095, n // 2 & ~4095, 3 * n // 4 & ~4095, n]
    yield [n // 4 & ~4095, n]
    yield [4097, n]
    for _ in range(3):
        K = rng.randint(2, 8)
        cuts = sorted(rng.sample(range(4097, n - 4097), K - 1))
        if all(b - a >= 4097 for a, b in zip([0] + cuts, cuts + [n])):
            yield cuts + [n]


def test_every_chunk_asks_for_the_same_bytes(lib):
    """ws_get regrows a slot that is asked for more: every chunk of a problem must ask for the same bytes, and they must
    cover what that chunk's launches touch -- otherwise a later chunk would free an earlier chunk's buckets"""
    rng = random.Random(18)
    for kind, _ in layouts():
        for n in CHUNK_SIZES:
            stride = stride_for(kind, n)
            if not lib.chunkable(n, kind, stride):
                continue
            for ends in splits(n, rng):
                sizes = [b - a for a, b in zip([0] + ends[:-1], ends)]
                K, n_alloc = len(sizes), max(sizes)
                plans = [plan(lib, m, kind, stride, n_shape=n, n_alloc=n_alloc, chunks=K) for m in sizes]
                first = plans[0]
                for m, p in zip(sizes, plans):
                    assert p["err"] == 0 and p["path"] == TWO_LEVEL
                    for s in SLOTS:
                        assert p["ws_" + s] == first["ws_" + s], (hex(kind), n, sizes, s)
                        assert p["used_" + s] <= p["ws_" + s], (hex(kind), n, m, s)
                    for q in ("E", "T", "n_coarse", "n_fine"):
                        assert p["own_" + q] <= p["alloc_" + q], (hex(kind), n, m, q)
                    assert p["ws_out"] == 0        # the chunked call reduces once, after the last chunk


def test_one_piece_calls_ask_for_what_they_use(lib):
    for kind, stride, n in ((PLAIN, 0, 1 << 20), (MONT, 1 << 20, 5000), (tables(17), 1 << 20, 1 << 20), (tables(10), 1 << 14, 1 << 14)):
        p = plan(lib, n, kind, stride)
        assert p["err"] == 0
        for s in SLOTS:
            if s not in ("points", "out"):
                assert p["used_" + s] == p["ws_" + s], (hex(kind), s)
        assert p["ws_out"] > 0 and (p["ws_points"] > 0) == (kind == PLAIN)


def test_the_decisions_the_comments_promise(lib):
    # generic layout: 16-bit windows at 2^17 pairs (8 full windows), 19 bits from 3 x 2^21 on (7 x 2^18 buckets sorted as 2^21, 1024 bins)
    p = plan(lib, 1 << 17, PLAIN, 0)
    assert (p["c"], p["nwin"], p["NB"], p["path"]) == (16, 8, 1 << 18, TWO_LEVEL)
    assert plan(lib, 3 * (1 << 21) - 1, PLAIN, 0)["c"] == 16
    for n in (3 * (1 << 21), 1 << 24):
        p = plan(lib, n, PLAIN, 0)
        assert (p["c"], p["nwin"], p["NB"], p["NBtot"], p["cl"]) == (19, 7, 7 << 18, 1 << 21, 10), n
        assert (p["one_set"], p["red_windows"], p["horner_c"], p["coarse_c"]) == (0, 7, 19, 0)
    # 17-bit tables at 2^20 points: 512 bins buy the 4-byte records; at 2^21 points they would not: 256 bins, 8-byte records
    p = plan(lib, 1 << 20, tables(17), 1 << 20)
    assert (p["cl"], p["compact"], p["coarse_c"], p["staged"]) == (9, 1, 17, 1)
    p = plan(lib, 1 << 20, tables(17), 1 << 21)
    assert (p["cl"], p["compact"]) == (8, 0)
    p = plan(lib, 1 << 22, tables(20), 1 << 22)
    assert (p["cl"], p["coarse_c"], p["one_set"], p["red_windows"], p["horner_c"]) == (10, 20, 1, 1, 0)
    p = plan(lib, 1 << 18, tables(16), 1 << 18)
    assert (p["cl"], p["coarse_c"], p["path"]) == (8, 16, TWO_LEVEL)
    p = plan(lib, 1 << 18, tables(16, 2), 1 << 18)
    assert (p["sets"], p["NB"], p["coarse_c"], p["one_set"], p["red_windows"], p["horner_c"]) == (2, 1 << 16, 0, 0, 2, 16)
    # small inputs: below 4096 pairs the one-workgroup sort; c in {8, 10..13} with one bucket set up to 2^14 the sortless scan
    for n in (1, 100, 4095):
        assert plan(lib, n, PLAIN, 0)["path"] == SMALL_SORT and plan(lib, n, MONT, n)["path"] == SMALL_SORT
        assert plan(lib, n, tables(9), n)["path"] == SMALL_SORT and plan(lib, n, tables(14), n)["path"] == SMALL_SORT
    assert plan(lib, 4096, PLAIN, 0)["path"] != SMALL_SORT and plan(lib, 4096, tables(14), 4096)["path"] == SMALL_SORT
    for c in (8, 10, 11, 12, 13):
        for n in (1, 4097, 1 << 14):
            assert plan(lib, n, tables(c), n)["path"] == SMALL_SCAN, (c, n)
        assert plan(lib, (1 << 14) + 1, tables(c), 1 << 15)["path"] == (TWO_LEVEL if c == 13 else LDS_ONE_PASS), c   # (2^12 buckets sort in two levels)
        assert plan(lib, 100, tables(c, 2), 100)["path"] == SMALL_SORT, c
    assert plan(lib, 1 << 20, tables(8), 1 << 20)["path"] == LDS_ONE_PASS
    # below 4096 pairs the merged layout keeps the one-pass histogram as long as it fits the LDS: 2^15 buckets
    assert plan(lib, 4000, tables(16), 1 << 15)["path"] == LDS_ONE_PASS
    assert plan(lib, 4000, tables(17), 1 << 15)["path"] == TWO_LEVEL
    assert plan(lib, 1 << 13, tables(16, 2), 1 << 13)["path"] == TWO_LEVEL
    # point references are 31 bits, entry offsets 32
    assert plan(lib, 1 << 20, tables(16), 1 << 27)["err"] == 0
    assert plan(lib, 1 << 20, tables(8), 1 << 27)["err"] != 0             # 32 tables x 2^27 points
    assert plan(lib, 1 << 20, MONT, (1 << 31) - (1 << 20))["err"] == 0
    assert plan(lib, 1 << 20, MONT, (1 << 31) - (1 << 20) + 1)["err"] != 0
    assert plan(lib, 100, tables(8), 1 << 27)["err"] == 0                 # (the short paths gather nothing out of range)
    assert plan(lib, (1 << 27) + 1, PLAIN, 0)["err"] != 0
    # chunk mode needs the two-level sort
    assert plan(lib, 1 << 18, tables(10), 1 << 18, chunks=2)["err"] != 0


def test_every_layout_takes_the_tabled_path_at_every_prefix(lib):
    """msm_layouts.EXPECTED_PATH, the literal table tests/test_gpu_msm_layouts.py commits through: 23 layouts x 8 prefixes of a 2^15-point
    handle, at the CU count of an MI355X and at two others (the path, and the sort's shape, do not depend on it).  A changed threshold
    has to change that table on purpose."""
    assert set(msm_layouts.EXPECTED_PATH) == set(msm_layouts.LAYOUTS) and len(msm_layouts.LAYOUTS) == 23
    ran = set()
    for (c, sets), paths in msm_layouts.EXPECTED_PATH.items():
        assert len(paths) == len(msm_layouts.PREFIXES)
        for n, path in zip(msm_layouts.PREFIXES, paths):
            for num_cu in (256, 64, 304):
                p = plan(lib, n, tables(c, sets), msm_layouts.N_SRS, num_cu=num_cu)
                where = (c, sets, n, num_cu)
                assert p["err"] == 0 and p["path"] == msm_layouts.PATH_ID[path], where
                assert (p["c"], p["sets"], p["nwin"], p["NB"]) == (c, sets, 254 // c + 1, sets << (c - 1)), where
                assert (p["one_set"], p["red_windows"], p["horner_c"]) == (int(sets == 1), sets, 0 if sets == 1 else c), where
                if path != msm_layouts.TWO:
                    continue
                assert p["cl"] == msm_layouts.EXPECTED_CL.get((c, sets), 8), where
                assert p["F"] == (sets << (c - 1)) >> p["cl"], where
                if sets == 1:
                    assert p["F"] == msm_layouts.EXPECTED_F[c], where
                assert p["coarse_c"] == msm_layouts.EXPECTED_COARSE_C.get((c, sets), 0) and p["staged"] == int(p["coarse_c"] != 0), where
                assert p["compact"] == int((c, sets) not in msm_layouts.EXPECTED_WIDE_RECORDS), where
            ran.add(path)
    assert ran == set(msm_layouts.PATH_ID)
