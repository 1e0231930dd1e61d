"""What an SRS handle decides on the host (myzkp_amd/csrc/mzk_srs_plan.h), compiled with g++ through a small shim
(tests/hostcheck/srs_plan_shim.cpp): window width by size, the layout ladder and its budget rule, the point_kind encoding, the width of
the direct tables, when the grid-batched pass builds wide tables, and when a dump's stored tables are used.  CPU only."""
import ctypes, os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
U64 = ctypes.c_uint64
OWN, WIDE, ALLOCATE, REFUSE = range(4)          # SrsWideStep
UNTRIED, BUILT, REFUSED = range(3)              # SrsWideState
DIRECT_OK, BAD_WIDTH, OVER_BUDGET = range(3)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("srs_plan") / "libsrsplan.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "srs_plan_shim.cpp")])
    L = ctypes.CDLL(so)
    L.window_bits.argtypes = [U64]
    L.ladder.argtypes = [U64, ctypes.c_int, U64, ctypes.POINTER(U64)]
    L.point_kind.argtypes = [ctypes.c_int] * 3
    L.table_rows.argtypes = [ctypes.c_int] * 3
    L.table_rows.restype = U64
    L.direct_bytes.argtypes = [U64, ctypes.c_int]
    L.direct_bytes.restype = U64
    L.direct_plan.argtypes = [U64, ctypes.c_int, U64, ctypes.POINTER(U64)]
    L.direct_plan.restype = None
    L.wide_from.restype = U64
    L.wide_bytes.argtypes = [U64]
    L.wide_bytes.restype = U64
    L.wide_step.argtypes = [U64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, U64, U64, U64]
    L.use_stored.argtypes = [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, U64]
    return L


def ladder(L, n, with_tables, budget=0):
    """[(tables, bits, sets, rows, bytes)] in the order srs_new tries them"""
    out = (U64 * 20)()
    count = L.ladder(n, with_tables, budget, out)
    assert 1 <= count <= 4
    return [tuple(int(v) for v in out[5 * k:5 * k + 5]) for k in range(count)]


def direct(L, n, requested, budget):
    out = (U64 * 3)()
    L.direct_plan(n, requested, budget, out)
    return tuple(int(v) for v in out)


@pytest.mark.parametrize("n,bits", [(1024, 8), (1025, 10), (1 << 14, 10), ((1 << 14) + 1, 16), ((1 << 19) - 1, 16), (1 << 19, 17),
                                    ((1 << 22) - 1, 17), (1 << 22, 20), (1, 8), (1 << 27, 20)])
def test_window_bits_at_every_threshold(lib, n, bits):
    assert lib.window_bits(n) == bits


def test_the_ladder_degrades_full_tables_to_two_sets_to_four_to_the_points(lib):
    n = (1 << 16) + 37
    rungs = ladder(lib, n, 1)
    assert [(t, b, s) for t, b, s, _, _ in rungs] == [(1, 16, 1), (1, 16, 2), (1, 16, 4), (0, 16, 1)]
    assert [r[3] for r in rungs] == [16, 8, 4, 2]
    assert [r[4] for r in rungs] == [rows * n * 64 for rows in (16, 8, 4, 2)]
    assert ladder(lib, n, 16) == rungs                                    # the default width asked for by name
    assert ladder(lib, n, 0) == [(0, 16, 1, 2, 2 * n * 64)]               # prepared points: nothing to degrade


def test_a_rung_over_the_budget_is_skipped_but_for_the_last(lib):
    """the budgets of test_table_budget_degrades_the_layout_not_the_result (test_gpu_dev_api.py) and what a handle reports there"""
    n = (1 << 16) + 37
    full = 16 * n * 64
    picked = []
    for budget in (0, full, full - 1, 8 * n * 64 - 1, 4 * n * 64 - 1, 1):
        rungs = ladder(lib, n, 1, budget)
        tables, bits, sets, rows, nbytes = rungs[0]
        picked.append(sets if tables else 0)                              # mzk_srs_bucket_sets
        assert all(r[4] <= budget for r in rungs[:-1]) or budget == 0
        assert rungs[-1] == (0, 16, 1, 2, 2 * n * 64)                     # the prepared points ignore the budget
        assert rungs == [r for r in ladder(lib, n, 1) if r[4] <= budget or not budget or not r[0]]     # order kept, nothing else dropped
    assert picked == [1, 1, 2, 4, 0, 0]


def test_a_requested_width_above_17_bits_degrades_to_17(lib):
    n = (1 << 16) + 37
    assert [(t, b, s, rows) for t, b, s, rows, _ in ladder(lib, n, 20)] == [(1, 20, 1, 13), (1, 17, 2, 8), (1, 17, 4, 4), (0, 20, 1, 2)]
    assert ladder(lib, n, 20, 10 * n * 64)[0][:3] == (1, 17, 2)


@pytest.mark.parametrize("bits,rows", [(14, (19, 10, 5)), (15, (17, 9, 5)), (16, (16, 8, 4)), (17, (15, 8, 4))])
def test_table_rows_per_bucket_set_count(lib, bits, rows):
    rungs = ladder(lib, 1 << 15, bits)
    assert tuple(r[3] for r in rungs[:3]) == rows and [r[2] for r in rungs[:3]] == [1, 2, 4]
    for sets, want in zip((1, 2, 4), rows):
        assert lib.table_rows(1, bits, sets) == want == 254 // (bits * sets) + 1
    assert lib.table_rows(0, bits, 1) == 2


def test_no_multi_set_rungs_below_2_15_points_or_below_14_bits(lib):
    assert [r[:3] for r in ladder(lib, (1 << 15) - 1, 16)] == [(1, 16, 1), (0, 16, 1)]
    assert [r[:3] for r in ladder(lib, 1 << 15, 13)] == [(1, 13, 1), (0, 13, 1)]
    assert [r[:3] for r in ladder(lib, 1 << 22, 13)] == [(1, 13, 1), (0, 13, 1)]
    assert [r[:3] for r in ladder(lib, 5000, 1)] == [(1, 10, 1), (0, 10, 1)]
    assert len(ladder(lib, 1 << 15, 14)) == 4


def test_an_empty_handle(lib):
    """no points: no default tables, a requested width is kept, and nothing is ever over a budget"""
    assert ladder(lib, 0, 1) == [(0, 8, 1, 2, 0)]
    assert ladder(lib, 0, 0) == [(0, 8, 1, 2, 0)]
    for budget in (0, 1):
        assert ladder(lib, 0, 16, budget) == [(1, 16, 1, 16, 0), (0, 16, 1, 2, 0)]


def test_point_kind_encoding(lib):
    assert lib.point_kind(0, 16, 1) == 1                                   # MSM_PTS_MONT, whatever the width says
    assert lib.point_kind(1, 16, 1) == 2 | (16 << 8) | (1 << 16)
    assert lib.point_kind(1, 17, 4) == 2 | (17 << 8) | (4 << 16)


def test_direct_width_by_budget_and_the_refusal(lib):
    n = 1024
    size = {c: (254 // c + 1) * n * (1 << (c - 1)) * 64 for c in range(8, 13)}
    for c in size:
        assert lib.direct_bytes(n, c) == size[c]
    assert size[10] == 26 * 1024 * 512 * 64
    assert direct(lib, n, 0, size[12]) == (DIRECT_OK, 12, size[12])
    assert direct(lib, n, 0, size[12] - 1) == (DIRECT_OK, 11, size[11])
    assert direct(lib, n, 0, size[9] - 1) == (DIRECT_OK, 8, size[8])
    assert direct(lib, n, 0, size[8]) == (DIRECT_OK, 8, size[8])
    assert direct(lib, n, 0, size[8] - 1) == (OVER_BUDGET, 8, size[8])
    assert direct(lib, n, 10, size[10]) == (DIRECT_OK, 10, size[10])
    assert direct(lib, n, 10, 1 << 62) == (DIRECT_OK, 10, size[10])         # a requested width is not widened
    assert direct(lib, n, 10, size[10] - 1) == (OVER_BUDGET, 10, size[10])
    for bad in (-1, 1, 7, 13, 22):
        assert direct(lib, n, bad, 1 << 62)[0] == BAD_WIDTH


def test_wide_tables_every_branch(lib):
    n, frm = 1 << 14, 1 << 13
    assert lib.wide_from() == frm and lib.wide_bits() == 12
    wb = lib.wide_bytes(n)
    assert wb == 22 * n * 64
    own = 26 * n * 64

    def step(n_poly=frm, has_tables=1, sets=1, bits=10, state=UNTRIED, budget=0):
        return lib.wide_step(n_poly, has_tables, sets, bits, state, own, n, budget)
    assert step() == ALLOCATE                                               # no budget: built by the first long batch
    assert step(n_poly=frm - 1) == OWN                                      # short polynomials keep the narrow tables
    assert step(has_tables=0) == OWN and step(sets=2) == OWN
    assert step(bits=12) == OWN and step(bits=16) == OWN and step(bits=11) == ALLOCATE and step(bits=8) == ALLOCATE
    assert step(budget=own + wb) == ALLOCATE                                # own + bytes <= budget
    assert step(budget=own + wb - 1) == REFUSE
    assert step(state=BUILT) == WIDE and step(state=BUILT, budget=1) == WIDE
    assert step(state=BUILT, n_poly=frm - 1) == OWN                         # built, and still only for long polynomials
    assert step(state=REFUSED) == OWN and step(state=REFUSED, budget=0) == OWN      # a refusal is not tried again


def test_stored_tables_are_used_only_as_they_are(lib):
    n = 5000                                                                # default width 10 bits: 25 rows behind the points
    assert lib.use_stored(1, 2, 1, 10, 25, n)
    assert lib.use_stored(10, 2, 1, 10, 25, n)
    assert not lib.use_stored(1, 1, 1, 10, 25, n)                           # format 1: no table checksum
    assert not lib.use_stored(1, 2, 0, 10, 25, n)                           # no tables in the file
    assert not lib.use_stored(0, 2, 1, 10, 25, n)                           # none wanted
    assert not lib.use_stored(16, 2, 1, 10, 25, n)                          # another width wanted
    assert not lib.use_stored(1, 2, 1, 16, 15, n)                           # another width stored
    assert not lib.use_stored(1, 2, 1, 10, 24, n)                           # a row count that is not that width's
    assert not lib.use_stored(1, 2, 1, 8, 31, 0)                            # an empty dump
    assert lib.use_stored(16, 2, 1, 16, 15, (1 << 16) + 37)
