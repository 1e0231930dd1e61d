"""tests/sumcheck_product_cases.py against the sources and the model: the thresholds parse, schedule() is the host loop of
scp_prove_impl, and every table builder has, under the model alone, the property that test_gpu_sumcheck_product_matrix.py relies on --
so that none of its cases can pass without having met what it is there for.  No GPU, no library."""
import pytest
import sumcheck_product_cases as sc
import sumcheck_product_model as sm

P = sm.P


def test_the_thresholds_parse():
    assert (sc.SCP_MAX_FACTORS, sc.SCP_MAX_DEGREE) == (8, 8), "k_sc_round has eight instantiations; the matrix sweeps 1..8 x 1..8"
    assert sc.SC_TAIL_LOG >= 3 and 1 << sc.SC_TAIL_LOG <= 128, "the tail's tables are one wave's work: h <= 64"
    assert sc.SC_THREADS % 64 == 0 and sc.SC_MAX_WG >= 1
    assert sc.MLE_TILE_LOG >= 3
    assert 22 <= sc.SCP_MAX_VARS < 64
    table = sc.constexpr_ints(sc._HIP)
    assert table["SC_TAIL_M"] == 1 << sc.SC_TAIL_LOG
    assert "SC_WAVES" not in table, "a derived constant is not a decimal: the expression must not be read as one"


def host_loop(el):
    """scp_prove_impl, launch by launch: (phase, round, workgroups, index pairs)"""
    n = 1 << el
    j0 = el - sc.SC_TAIL_LOG if el > sc.SC_TAIL_LOG else 0
    out = []
    for j in range(j0):
        h = n >> (j + 1)
        need = (h + sc.SC_THREADS - 1) // sc.SC_THREADS
        nwg = need if need < sc.SC_MAX_WG else sc.SC_MAX_WG
        out.append(("round0" if j == 0 else "round", j, nwg, h))
        out.append(("round_end", j, 1, 0))
    out.append(("tail", j0, 1, n >> j0))
    return out


@pytest.mark.parametrize("el", range(1, sc.SCP_MAX_VARS + 1))
def test_schedule_is_the_host_loop(el):
    launches, trips = sc.schedule(el)
    loop = host_loop(el)
    assert launches == tuple(sum(1 for l in loop if l[0] == ph) for ph in ("round0", "round", "round_end", "tail"))
    grid = [l for l in loop if l[0] in ("round0", "round")]
    assert len(trips) == len(grid)
    for t, (_, j, nwg, h) in zip(trips, grid):
        lanes = nwg * sc.SC_THREADS
        assert (t - 1) * lanes < h <= t * lanes, (j, t)          # the last trip has work, no index is left over
    assert loop[-1][3] <= 1 << sc.SC_TAIL_LOG
    if (sc.SC_TAIL_LOG, sc.SC_THREADS, sc.SC_MAX_WG) == (7, 128, 2048):
        assert launches == (el > 7, max(el - 8, 0), max(el - 7, 0), 1)
        assert all(t == 1 << max(el - 1 - j - 18, 0) for j, t in enumerate(trips))


def test_the_stride_cases_stride():
    for el, k, d, rounds in sc.STRIDE_CASES:
        trips = sc.schedule(el)[1]
        assert all(trips[j] > 1 for j in rounds), (el, trips)
        assert 1 <= k <= sc.SCP_MAX_FACTORS and 1 <= d <= sc.SCP_MAX_DEGREE and el <= sc.SCP_MAX_VARS
    assert any(j >= 1 for el, k, d, rounds in sc.STRIDE_CASES for j in rounds), "no case strides in a round that folds and stores"
    assert any(el == 21 and k == 5 for el, k, d, _ in sc.STRIDE_CASES) and sc.schedule(21)[1][:2] == [4, 2]


def test_the_regimes_of_the_matrix():
    """el = 3, SC_TAIL_LOG, SC_TAIL_LOG + 2: tail alone with a partial wave, tail alone with a full one, two grid rounds before it"""
    assert sc.schedule(3)[0] == (0, 0, 0, 1) and (1 << 3) // 2 < 64
    assert sc.schedule(sc.SC_TAIL_LOG)[0] == (0, 0, 0, 1)
    assert sc.schedule(sc.SC_TAIL_LOG + 2)[0] == (1, 1, 2, 1)


def test_uniform_is_canonical_and_seeded():
    a, b = sc.uniform(6, 3, 5), sc.uniform(6, 3, 5)
    assert a == b and a != sc.uniform(6, 3, 6)
    assert all(0 <= v < P for t in a for v in t) and len(a) == 3 and all(len(t) == 64 for t in a)


@pytest.mark.parametrize("case", sc.CORNER_CASES, ids=lambda c: "el%d-k%d-d%d" % c[1:4])
def test_corners_reach_every_difference(case):
    kind, el, k, d, arg = case
    tables, header, want = sc.proof_of(*case)
    h = 1 << (el - 1)
    assert all(v in sc.CORNERS for t in tables for v in t)
    diffs = {(t[i + h] - t[i]) % P for t in tables for i in range(h)}
    assert {0, 1, P - 1, P - 2, 2, P - 3, 3} <= diffs, "a difference of round 0 is missing: another seed"
    assert all(v != 0 for v in want["evals"][0]), "s_0 has a zero point: the products cancel, another seed"
    assert want["sum"] == (want["evals"][0][0] + want["evals"][0][1]) % P


@pytest.mark.parametrize("c", range(sc.SCP_MAX_DEGREE + 1))
@pytest.mark.parametrize("el", [6, 9])
def test_root_at_puts_one_zero_between_full_records(el, c):
    k, d = 3, sc.SCP_MAX_DEGREE
    tables = sc.root_at(el, k, c, 7919 * el + 31 * k + c)
    s0 = sm.round_evals(tables, d)
    assert s0[c] == 0 and all(v != 0 for i, v in enumerate(s0) if i != c), s0
    assert all(0 <= v < P for t in tables for v in t)


@pytest.mark.parametrize("case", sc.ROOT_CASES, ids=lambda c: "el%d-c%d" % (c[1], c[4]))
def test_root_cases_of_the_matrix(case):
    kind, el, k, d, c = case
    tables, header, want = sc.proof_of(*case)
    assert want["evals"][0][c] == 0
    assert sc.zero_objects(want["transcript"]) == [c]
    at = sc.record_offset(want["transcript"], c)
    assert want["transcript"][at:at + 25] == sc.ZERO_RECORD
    assert sm.verify(tables, d, header, want["sum"], want["transcript"])


@pytest.mark.parametrize("case", sc.ZERO_SUM_CASES, ids=lambda c: "el%d" % c[1])
def test_zero_sum_cases_of_the_matrix(case):
    kind, el, k, d, arg = case
    tables, header, want = sc.proof_of(*case)
    assert want["sum"] == 0 and sm.claimed_sum(tables) == 0
    s0 = want["evals"][0]
    assert s0[0] != 0 and s0[1] == P - s0[0] and all(v != 0 for v in s0)
    assert sc.zero_objects(want["transcript"]) == [], "the claimed sum is not pushed: no value of the stream is zero"
    assert sm.verify(tables, d, header, 0, want["transcript"])


@pytest.mark.parametrize("k,d", [(6, 2), (4, 7), (5, 4), (3, 3), (1, 1), (3, 1)])
def test_verify_exact_is_the_verifier_where_the_verifier_is_complete(k, d):
    """d >= k: both accept the model's proof.  d < k: sm.verify rejects the honest stream -- the polynomial through d + 1 points of a
    degree-k one is another polynomial -- and verify_exact, which takes s_j(r_j) from the tables, accepts it."""
    el = 6
    tables, header, want = sc.proof_of("uniform", el, k, d, 0, "reference")
    res = sc.verify_exact(tables, d, header, want["sum"], want["transcript"], full_below=1 << el)
    assert res == {"challenges": want["challenges"], "finals": want["finals"]}
    assert sm.verify(tables, d, header, want["sum"], want["transcript"]) == (d >= k)
    assert sc.product_sum(tables) == want["sum"] == sm.claimed_sum(tables)


@pytest.mark.parametrize("k,d", [(6, 2), (4, 7)])
def test_verify_exact_rejects_what_is_wrong(k, d):
    el = 6
    tables, header, want = sc.proof_of("uniform", el, k, d, 0, "reference")
    stream, objs = want["transcript"], sm.deserialize_stream(want["transcript"])
    assert sc.verify_exact(tables, d, header, (want["sum"] + 1) % P, stream) is None
    assert sc.verify_exact(tables, d, header[:-1], want["sum"], stream) is None
    assert sc.verify_exact(tables, d, header, want["sum"], stream[:-1]) is None
    for j, c in ((0, 0), (0, 1), (2, 0), (el - 1, 1)):          # a pushed value off by one: its own round's check or the next one's
        at = len(header) + j * (d + 1) + c
        bent = objs[:at] + [[sm.fm.leaf((sm.unleaf(objs[at][0]) + 1) % P)]] + objs[at + 1:]
        assert sc.verify_exact(tables, d, header, want["sum"], sm.fm.serialize_stream(bent)) is None, (j, c)
    at = len(header) + 2 * (d + 1) + d                           # the last point of a round is pinned by full_below, and by the
    bent = objs[:at] + [[sm.fm.leaf((sm.unleaf(objs[at][0]) + 1) % P)]] + objs[at + 1:]          # interpolation where d >= k
    assert sc.verify_exact(tables, d, header, want["sum"], sm.fm.serialize_stream(bent), full_below=1 << el) is None
    other = [list(t) for t in tables]
    other[0][5] = (other[0][5] + 1) % P
    assert sc.verify_exact(other, d, header, want["sum"], stream) is None


def test_zero_objects_finds_what_is_there():
    stream = sm.fm.serialize_stream([[b"hdr"], [sm.fm.leaf(5)], [sm.fm.leaf(0)], [sm.fm.leaf(P - 1)], [sm.fm.leaf(0)]])
    assert sc.zero_objects(stream, header_objects=1) == [1, 3]
    at = sc.record_offset(stream, 1, header_objects=1)
    assert stream[at:at + 25] == sc.ZERO_RECORD and at == 8 + (16 + 3) + (16 + 13)


@pytest.mark.parametrize("el", [1, 5, 12])
def test_impulse_is_a_subset_indicator(el):
    for t in {0, 1, (1 << el) - 1, 1 << (el - 1), 5 % (1 << el)}:
        coef = sc.impulse(el, t)
        assert sum(coef) == 1 and coef[t] == 1
        assert sm.evals_over_boolean_hypercube(coef, el) == [1 if b & t == t else 0 for b in range(1 << el)]


def test_impulse_indices_touch_every_pass():
    """the bit ranges of mle_dev_impl's passes, restated: [0, T), then T - 2 bits at a time"""
    for el in (19, 22):
        passes, lo = [], 0
        while lo < el:
            cb = min(lo, 2)
            g = min(el - lo, sc.MLE_TILE_LOG - cb)
            passes.append((lo, lo + g))
            lo += g
        assert len(passes) == 3
        ts = sc.impulse_indices(el)
        assert all(0 <= t < 1 << el for t in ts) and len(set(ts)) == len(ts)
        for lo, hi in passes:          # the lowest and the highest bit of every pass, each alone
            assert 1 << lo in ts or lo == 0 and 1 in ts
            assert 1 << (hi - 1) in ts
        assert any(all(t >> lo & ((1 << (hi - lo)) - 1) for lo, hi in passes) and t != (1 << el) - 1 for t in ts)


def test_packed_round_trip():
    vals = [0, 1, P - 1, 1 << 200]
    raw = sc.packed(vals)
    assert len(raw) == 128 and [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(4)] == vals
