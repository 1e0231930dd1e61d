"""The product sum-check (mzk_sumcheck.hip) at every factor count, degree and launch schedule, against tests/sumcheck_product_model.py
bit for bit (sum, evals, challenges, finals, transcript) unless a test says otherwise.  Shapes and tables come from
tests/sumcheck_product_cases.py, whose promises test_sumcheck_product_cases.py checks without a GPU.

  a  every (k, d) in 1..8 x 1..8 with the tail on a partial wave (el = 3), the tail alone (SC_TAIL_LOG) and two grid rounds before it
  b  el = 1 .. 13 for three (k, d), host form and _dev form, the launches per phase counted and equal to schedule(el)
  c  tables at the field's edges; a zero s_0(c) between full records; a zero claimed sum over non-zero tables
  d  the reference-shaped header on factor counts that no other header test uses
  e  three _dev proofs of different shapes on one stream, one synchronize
  f  a lane of k_sc_round making several trips: el = 20 and 21 in full, el = 21 with five factors in linear time
  g  k_mle_pass with one, two and three passes, the copy path, all p - 1, and single monomials on every side of the tile split
  h  every refusal of the five entry points: the code, the message, nothing launched, nothing written"""
import ctypes, random
import numpy as np
import pytest
import sumcheck_product_cases as sc
import sumcheck_product_model as sm
from test_gpu_sumcheck_product import check, written

pytestmark = pytest.mark.gpu
P = sm.P
SZ, VP = ctypes.c_size_t, ctypes.c_void_p
PH_SCP = (13, 14, 15, 16)          # MZK_PH_SCP_ROUND0, _ROUND, _ROUND_END, _TAIL (include/mzk.h)
E_ARG, E_LENGTH, E_RANGE = -1, -5, -6


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def limbs(values):
    return np.frombuffer(sc.packed(values), dtype=np.uint64).reshape(-1, 4).copy()


def table_limbs(tables):
    return np.stack([limbs(t) for t in tables])


def to_device(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def from_device(t):
    return t.cpu().numpy().view(np.uint64)


def phase_counts(mz, call):
    """(call's result, launches of the four sum-check phases while it ran): phase_pairs of test_gpu_msm_layouts.py"""
    L = mz.lib()
    assert L.mzk_prof_select(ctypes.c_uint32(0xffffffff)) == 0
    assert L.mzk_prof_enable(1) == 0
    try:
        assert L.mzk_prof_reset() == 0
        got = call()
        out = []
        for ph in PH_SCP:
            ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
            assert L.mzk_prof_read(ph, ctypes.byref(ms), ctypes.byref(cnt)) == 0
            out.append(cnt.value)
        return got, tuple(out)
    finally:
        L.mzk_prof_enable(0)
        L.mzk_prof_reset()


def prove_dev(mz, dev_tables, el, k, d, header=(), raw=False):
    return mz.sumcheck_product_prove(None, d, header_objects=header, device_ptr=dev_tables.data_ptr(), num_vars=el, num_factors=k, raw=raw)


# ---- a. every (k, d), three regimes ------------------------------------------------------------------------------------------
REGIMES = {"partial-wave": 3, "tail-alone": sc.SC_TAIL_LOG, "two-grid-rounds": sc.SC_TAIL_LOG + 2}


@pytest.mark.parametrize("k", range(1, sc.SCP_MAX_FACTORS + 1))
@pytest.mark.parametrize("regime", list(REGIMES))
def test_every_factor_count_and_degree(mz, regime, k):
    el = REGIMES[regime]
    arr = table_limbs(sc.tables_of("uniform", el, k))
    for d in range(1, sc.SCP_MAX_DEGREE + 1):
        want = sc.proof_of("uniform", el, k, d)[2]
        got = mz.sumcheck_product_prove(arr, d)
        for key in ("sum", "evals", "challenges", "finals", "transcript"):
            assert got[key] == want[key], (key, el, k, d)


# ---- b. every schedule --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(3, 3), (5, 7), (7, 4)])
@pytest.mark.parametrize("el", range(1, 14))
def test_every_schedule_in_both_forms(mz, el, k, d):
    tables, header, want = sc.proof_of("uniform", el, k, d)
    arr = table_limbs(tables)
    launches = sc.schedule(el)[0]
    host, counts = phase_counts(mz, lambda: mz.sumcheck_product_prove(arr, d, raw=True))
    assert counts == launches, ("host form", counts)
    check(mz.sumcheck_product_unpack(el, k, d, 0, host), want)
    dev = to_device(arr)
    got, counts = phase_counts(mz, lambda: prove_dev(mz, dev, el, k, d, raw=True))
    assert counts == launches, ("_dev form", counts)
    assert written(mz, el, k, d, 0, got) == written(mz, el, k, d, 0, host)
    assert np.array_equal(from_device(dev), arr)


# ---- c. values ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CORNER_CASES, ids=lambda c: "el%d-k%d-d%d" % c[1:4])
def test_corner_values(mz, case):
    kind, el, k, d, arg = case
    tables, header, want = sc.proof_of(*case)
    check(mz.sumcheck_product_prove(table_limbs(tables), d), want)


@pytest.mark.parametrize("case", sc.ROOT_CASES, ids=lambda c: "el%d-c%d" % (c[1], c[4]))
def test_a_zero_record_between_full_ones(mz, case):
    kind, el, k, d, c = case
    tables, header, want = sc.proof_of(*case)
    got = mz.sumcheck_product_prove(table_limbs(tables), d)
    check(got, want)
    stream = got["transcript"]
    assert got["evals"][0][c] == 0 and all(v != 0 for i, v in enumerate(got["evals"][0]) if i != c)
    assert sc.zero_objects(stream) == [c]
    at = sc.record_offset(stream, c)
    assert stream[at:at + 25] == sc.ZERO_RECORD
    assert int.from_bytes(stream[:8], "little") == el * (d + 1)
    assert len(stream) == 8 + sum(16 + len(sm.fm.leaf(v)) for s in want["evals"] for v in s)


@pytest.mark.parametrize("case", sc.ZERO_SUM_CASES, ids=lambda c: "el%d" % c[1])
def test_a_zero_sum_over_non_zero_tables(mz, case):
    kind, el, k, d, arg = case
    tables, header, want = sc.proof_of(*case)
    arr = table_limbs(tables)
    raw = mz.sumcheck_product_prove(arr, d, raw=True)
    got = mz.sumcheck_product_unpack(el, k, d, 0, raw)
    check(got, want)
    at, size = mz.sumcheck_product_layout(el, k, d, 0)[0]["sum"]
    assert size == 32 and raw[at:at + 32] == bytes(32)
    assert got["evals"][0][0] != 0 and sc.zero_objects(got["transcript"]) == []


# ---- d. headers on the new shapes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,d", [(6, 2), (4, 7)])
def test_reference_shaped_header_on_new_factor_counts(mz, k, d):
    el = 9
    tables, header, want = sc.proof_of("uniform", el, k, d, 0, "reference")
    assert len(header) == 3 + k
    got = mz.sumcheck_product_prove(table_limbs(tables), d, header_objects=header)
    check(got, want)
    # (6, 2) has d < k: there the reference's verifier rejects every honest stream, the model's own included, and verify_exact
    # (sumcheck_product_cases.py) does the same checks with s_j(r_j) taken from the tables
    assert sm.verify(tables, d, header, got["sum"], got["transcript"]) == (d >= k)
    res = sc.verify_exact(tables, d, header, got["sum"], got["transcript"], full_below=1 << el)
    assert res == {"challenges": got["challenges"], "finals": got["finals"]}


# ---- e. different shapes back to back -----------------------------------------------------------------------------------------
def test_different_shapes_back_to_back_on_one_stream(mz):
    import torch
    shapes = [(12, 8, 8), (9, 1, 1), (11, 5, 7)]
    cases = [sc.proof_of("uniform", el, k, d, 0, "reference") for el, k, d in shapes]
    arrs = [table_limbs(c[0]) for c in cases]
    headers = [mz.sumcheck_frame_header(c[1]) for c in cases]
    host = []
    for (el, k, d), a, c, h in zip(shapes, arrs, cases, headers):
        raw = mz.sumcheck_product_prove(a, d, header_objects=c[1], raw=True)
        check(mz.sumcheck_product_unpack(el, k, d, len(h), raw), c[2])
        host.append(written(mz, el, k, d, len(h), raw))
    devs = [to_device(a) for a in arrs]
    totals = [mz.sumcheck_product_layout(el, k, d, len(h))[1] for (el, k, d), h in zip(shapes, headers)]
    outs = [torch.zeros(t, dtype=torch.uint8, device="cuda") for t in totals]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    for (el, k, d), t, o, h, c, total in zip(shapes, devs, outs, headers, cases, totals):          # three proofs enqueued, ONE synchronize
        rc = mz.lib().mzk_sumcheck_product_prove_dev(VP(t.data_ptr()), SZ(el), SZ(k), SZ(d), ctypes.c_char_p(h), SZ(len(h)), SZ(len(c[1])),
                                                     VP(o.data_ptr()), SZ(total), VP(s.cuda_stream))
        assert rc == 0, mz.lib().mzk_last_error()
    s.synchronize()
    for (el, k, d), o, want, h in zip(shapes, outs, host, headers):
        assert written(mz, el, k, d, len(h), o.cpu().numpy().tobytes()) == want, (el, k, d)
    for t, a in zip(devs, arrs):
        assert np.array_equal(from_device(t), a)


# ---- f. grid stride -----------------------------------------------------------------------------------------------------------
def big_tables(el, k, seed):
    """(limbs, ints) of k tables of 2^el values, built in numpy: uniform below 2^192 * (p >> 192), which is below p"""
    n = 1 << el
    rng = np.random.default_rng(seed)
    arr = rng.integers(0, 1 << 64, size=(k, n, 4), dtype=np.uint64)
    arr[:, :, 3] = rng.integers(0, P >> 192, size=(k, n), dtype=np.uint64)
    tables = []
    for f in range(k):
        cols = [arr[f, :, q].tolist() for q in range(4)]
        tables.append([a | (b << 64) | (c << 128) | (e << 192) for a, b, c, e in zip(*cols)])
    return arr, tables


@pytest.mark.parametrize("el,k,d,rounds", [c for c in sc.STRIDE_CASES if c[1] == 2], ids=["el%d" % c[0] for c in sc.STRIDE_CASES if c[1] == 2])
def test_grid_stride_against_the_full_model(mz, el, k, d, rounds):
    trips = sc.schedule(el)[1]
    assert all(trips[j] > 1 for j in rounds)
    arr, tables = big_tables(el, k, el)
    got = mz.sumcheck_product_prove(arr, d)
    check(got, sm.prove(tables, d))


def test_grid_stride_with_five_factors_in_linear_time(mz):
    """the _dev form; SUM, FINALS and the verifier in linear Python work, as test_el20_passes_the_models_verifier.  With d < k the
    reference's verifier rejects every honest stream (test_sumcheck_product_cases.py), so the verifier is verify_exact: the same
    checks with s_j(r_j) as the product sum of the folded tables, and every point of the rounds from 2^18 entries down"""
    (el, k, d, rounds), = [c for c in sc.STRIDE_CASES if c[1] != 2]
    trips = sc.schedule(el)[1]
    assert all(trips[j] > 1 for j in rounds) and max(rounds) >= 1
    arr, tables = big_tables(el, k, 100 + el)
    dev = to_device(arr)
    got = prove_dev(mz, dev, el, k, d)
    assert got["sum"] == sc.product_sum(tables)
    res = sc.verify_exact(tables, d, (), got["sum"], got["transcript"], full_below=1 << 18)
    assert res is not None, "a round's s_j(0) + s_j(1) is not the product sum of the tables folded so far"
    assert got["challenges"] == res["challenges"]
    assert got["finals"] == res["finals"]
    assert sm.verify(tables, d, (), got["sum"], got["transcript"], finals=res["finals"]) == (d >= k)
    evals = [sm.unleaf(o[0]) for o in sm.deserialize_stream(got["transcript"])]
    assert evals == [v for s in got["evals"] for v in s] and len(evals) == el * (d + 1)
    assert np.array_equal(from_device(dev), arr)


# ---- g. the subset-sum butterfly ----------------------------------------------------------------------------------------------
def mle_dev(mz, src, el, dst):
    import torch
    s = torch.cuda.current_stream()
    mz.mle_evals_from_coeffs(None, device_ptr=src.data_ptr(), num_vars=el, out_ptr=dst.data_ptr(), stream=s.cuda_stream)
    s.synchronize()


def mle_all_forms(mz, c, want, el):
    """host form, _dev out of place with the input untouched, _dev in place"""
    import torch
    assert np.array_equal(mz.mle_evals_from_coeffs(c), want), "host form"
    src = to_device(c)
    dst = torch.zeros_like(src)
    mle_dev(mz, src, el, dst)
    assert np.array_equal(from_device(dst), want), "out of place"
    assert np.array_equal(from_device(src), c), "the input of an out-of-place call"
    mle_dev(mz, src, el, src)
    assert np.array_equal(from_device(src), want), "in place"


@pytest.mark.parametrize("el", [0, 2, sc.MLE_TILE_LOG - 1, sc.MLE_TILE_LOG + 2, 2 * sc.MLE_TILE_LOG - 3, 2 * sc.MLE_TILE_LOG - 2,
                                2 * sc.MLE_TILE_LOG - 1, 2 * sc.MLE_TILE_LOG])
def test_mle_uniform_coefficients(mz, el):
    rng = random.Random(4000 + el)
    coef = [rng.randrange(P) for _ in range(1 << el)]
    mle_all_forms(mz, limbs(coef), limbs(sm.evals_over_boolean_hypercube(coef, el)), el)


@pytest.mark.parametrize("el", [sc.MLE_TILE_LOG + 2, 2 * sc.MLE_TILE_LOG - 1])
def test_mle_all_p_minus_one(mz, el):
    """evals[b] = 2^popcount(b) (p - 1): every addition of the butterfly wraps"""
    n = 1 << el
    idx = np.arange(n, dtype=np.int64)
    pop = sum((idx >> s) & 1 for s in range(el))
    by_weight = limbs([pow(2, w, P) * (P - 1) % P for w in range(el + 1)])
    mle_all_forms(mz, limbs([P - 1]).repeat(n, axis=0), by_weight[pop], el)


@pytest.mark.parametrize("el", [2 * sc.MLE_TILE_LOG - 1, 2 * sc.MLE_TILE_LOG + 2])
def test_mle_single_monomials(mz, el):
    """coefficient 1 at t alone: the table is the indicator of b containing t -- index logic only, no arithmetic"""
    import torch
    n = 1 << el
    idx = np.arange(n, dtype=np.int64)
    buf = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    want = np.zeros((n, 4), dtype=np.uint64)
    for t in sc.impulse_indices(el):
        buf.zero_()
        buf[t, 0] = 1
        mle_dev(mz, buf, el, buf)
        want[:, 0] = (idx & t) == t
        got = from_device(buf)
        if not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).any(axis=1))
            raise AssertionError("monomial %#x at el = %d: %d entries differ, the first at %#x" % (t, el, len(bad), int(bad[0])))
    # and through the host form once, the monomial that spans all three passes
    t = sc.impulse_indices(el)[-1]
    c = np.zeros((n, 4), dtype=np.uint64)
    c[t, 0] = 1
    want[:, 0] = (idx & t) == t
    assert np.array_equal(mz.mle_evals_from_coeffs(c), want)


# ---- h. errors ----------------------------------------------------------------------------------------------------------------
def refused(mz, call, code, *words):
    """`call` returns `code`, leaves a message with every one of `words`, and launches no kernel of the prover"""
    rc, counts = phase_counts(mz, call)
    msg = mz.lib().mzk_last_error().decode()
    assert rc == code, (rc, msg)
    assert counts == (0, 0, 0, 0), counts
    assert msg and all(w in msg for w in words), msg


class Prover:
    """one small valid problem, host and device copies, and both entry points with any argument replaced"""

    def __init__(self, mz, el=4, k=3, d=3):
        import torch
        self.mz, self.el, self.k, self.d = mz, el, k, d
        self.objects = sm.reference_header(d, k, el, [b"f%d" % f for f in range(k)])
        self.header = mz.sumcheck_frame_header(self.objects)
        self.tables = table_limbs(sc.tables_of("uniform", el, k))
        self.total = mz.sumcheck_product_layout(el, k, d, len(self.header))[1]
        self.dev = to_device(self.tables)
        self.pad = torch.zeros(4, dtype=torch.int64, device="cuda")          # so that dev + 8 bytes and proof + 4 stay inside allocations
        self.fill = 0xA5

    def host(self, tables="own", el=None, k=None, d=None, header="own", nobj=None, out="own", cap=None):
        a = self.tables if isinstance(tables, str) else tables
        h = self.header if isinstance(header, str) else header
        buf = (ctypes.c_uint8 * (self.total + 8))(*([self.fill] * (self.total + 8)))
        before = None if a is None else a.copy()
        rc = self.mz.lib().mzk_sumcheck_product_prove(None if a is None else a.ctypes.data_as(VP), SZ(self.el if el is None else el),
                                                      SZ(self.k if k is None else k), SZ(self.d if d is None else d),
                                                      None if h is None else ctypes.c_char_p(h), SZ(len(h or b"")), SZ(len(self.objects) if nobj is None else nobj),
                                                      buf if isinstance(out, str) else out, SZ(self.total if cap is None else cap))
        assert bytes(buf) == bytes([self.fill]) * (self.total + 8), "the proof buffer of a refused call"
        assert before is None or np.array_equal(a, before)
        return rc

    def device(self, el=None, k=None, d=None, header="own", nobj=None, cap=None, table_shift=0, proof_shift=0, null_tables=False, null_proof=False):
        import torch
        h = self.header if isinstance(header, str) else header
        out = torch.full((self.total + 16,), self.fill, dtype=torch.uint8, device="cuda")
        s = torch.cuda.current_stream()
        rc = self.mz.lib().mzk_sumcheck_product_prove_dev(None if null_tables else VP(self.dev.data_ptr() + table_shift), SZ(self.el if el is None else el),
                                                          SZ(self.k if k is None else k), SZ(self.d if d is None else d), ctypes.c_char_p(h), SZ(len(h)),
                                                          SZ(len(self.objects) if nobj is None else nobj),
                                                          None if null_proof else VP(out.data_ptr() + proof_shift), SZ(self.total if cap is None else cap),
                                                          VP(s.cuda_stream))
        s.synchronize()
        assert bool((out == self.fill).all()), "the device proof buffer of a refused call"
        assert np.array_equal(from_device(self.dev), self.tables)
        return rc


@pytest.fixture(scope="module")
def prover(mz):
    p = Prover(mz)
    # the problem itself is a valid one: both forms accept it and agree with the model
    want = sm.prove(sc.tables_of("uniform", p.el, p.k), p.d, p.objects)
    check(mz.sumcheck_product_prove(p.tables, p.d, header_objects=p.objects), want)
    check(prove_dev(mz, p.dev, p.el, p.k, p.d, header=p.objects), want)
    return p


def layout_rc(mz, el, k, d, hl):
    n = len(sm.SECTIONS)
    off, size, total = (ctypes.c_uint64 * n)(*([77] * n)), (ctypes.c_uint64 * n)(*([77] * n)), ctypes.c_uint64(77)
    rc = mz.lib().mzk_sumcheck_product_layout(SZ(el), SZ(k), SZ(d), SZ(hl), off, size, ctypes.byref(total))
    if rc != 0:
        assert list(off) == [77] * n and list(size) == [77] * n and total.value == 77
    return rc


@pytest.mark.parametrize("name,value,code,word", [("k", 0, E_ARG, "0 factors"), ("k", sc.SCP_MAX_FACTORS + 1, E_ARG, "%d factors" % (sc.SCP_MAX_FACTORS + 1)),
                                                   ("d", 0, E_ARG, "max_degree 0"), ("d", sc.SCP_MAX_DEGREE + 1, E_ARG, "max_degree %d" % (sc.SCP_MAX_DEGREE + 1)),
                                                   ("el", 0, E_LENGTH, "no variable"), ("el", sc.SCP_MAX_VARS + 1, E_LENGTH, "%d variables" % (sc.SCP_MAX_VARS + 1))])
def test_shapes_out_of_range_are_refused_by_all_three(mz, prover, name, value, code, word):
    shape = {"el": prover.el, "k": prover.k, "d": prover.d}
    shape[name] = value
    refused(mz, lambda: layout_rc(mz, shape["el"], shape["k"], shape["d"], len(prover.header)), code, word)
    refused(mz, lambda: prover.host(**{name: value}), code, word)
    refused(mz, lambda: prover.device(**{name: value}), code, word)


def test_layout_limits_the_header(mz, prover):
    assert layout_rc(mz, prover.el, prover.k, prover.d, 1 << 40) == 0
    refused(mz, lambda: layout_rc(mz, prover.el, prover.k, prover.d, (1 << 40) + 1), E_LENGTH, "header of %d bytes" % ((1 << 40) + 1))


def test_a_short_proof_buffer_is_refused(mz, prover):
    words = ("proof buffer of %d bytes" % (prover.total - 1), "needs %d" % prover.total)
    refused(mz, lambda: prover.host(cap=prover.total - 1), E_LENGTH, *words)
    refused(mz, lambda: prover.device(cap=prover.total - 1), E_LENGTH, *words)


def test_null_pointers_are_refused(mz, prover):
    refused(mz, lambda: prover.host(tables=None), E_ARG, "null pointer")
    refused(mz, lambda: prover.host(out=None), E_ARG, "null pointer")
    refused(mz, lambda: prover.device(null_tables=True), E_ARG, "null pointer")
    refused(mz, lambda: prover.device(null_proof=True), E_ARG, "null pointer")


def bad_headers(p):
    """(what, bytes, claimed objects): none parses to exactly that many objects over exactly those bytes"""
    last = p.objects[-1]
    longer = sm.frame_header(p.objects[:-1]) + (1).to_bytes(8, "little") + (len(last[0]) + 1).to_bytes(8, "little") + last[0]
    return [("one byte short", p.header[:-1], len(p.objects)),
            ("one object too few", sm.frame_header(p.objects[:-1]), len(p.objects)),
            ("one object too many", p.header, len(p.objects) - 1),
            ("a string length past the end", longer, len(p.objects)),
            ("a string length of 2^64 - 1", p.header[:8] + b"\xff" * 8 + p.header[16:], len(p.objects))]


def test_a_header_that_does_not_parse_is_refused(mz, prover):
    assert sm.frame_header(prover.objects) == prover.header
    for what, raw, nobj in bad_headers(prover):
        total = mz.sumcheck_product_layout(prover.el, prover.k, prover.d, len(raw))[1]
        assert total <= prover.total + 8, what          # the buffers of `prover` hold this layout too: the header is what is refused
        words = ("does not parse to %d objects over %d bytes" % (nobj, len(raw)),)
        refused(mz, lambda: prover.host(header=raw, nobj=nobj, cap=total), E_ARG, *words)
        refused(mz, lambda: prover.device(header=raw, nobj=nobj, cap=total), E_ARG, *words)


@pytest.mark.parametrize("value", [P, (1 << 256) - 1], ids=["p", "2^256-1"])
@pytest.mark.parametrize("factor,index", [(0, 5), (2, 15)], ids=["first-factor", "last-factor-last-entry"])
def test_a_non_canonical_table_value_is_named(mz, prover, factor, index, value):
    assert factor < prover.k and index < 1 << prover.el
    bad = prover.tables.copy()
    bad[factor, index] = limbs([value])[0]
    refused(mz, lambda: prover.host(tables=bad), E_RANGE, "table value %d of factor %d not canonical" % (index, factor))
    bad[factor, index] = limbs([P - 1])[0]          # the largest canonical value in the same place is taken
    assert mz.sumcheck_product_prove(bad, prover.d)["sum"] == sm.claimed_sum([mz.from_limbs(t) for t in bad])


def test_misaligned_device_pointers_are_refused(mz, prover):
    assert prover.dev.data_ptr() % 16 == 0
    refused(mz, lambda: prover.device(table_shift=8), E_ARG, "alignment")
    refused(mz, lambda: prover.device(proof_shift=4), E_ARG, "alignment")


def test_mle_refusals(mz):
    import torch
    L = mz.lib()
    el = 3
    coef = limbs(sc.uniform(el, 1, 9)[0])
    out = np.full((1 << el, 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    src = to_device(np.concatenate([coef, coef]))          # twice the size: a shifted pointer stays inside the allocation
    dst = torch.full((2 << el, 4), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()

    def host(c, o, n=el):
        return L.mzk_mle_evals_from_coeffs(None if c is None else c.ctypes.data_as(VP), SZ(n), None if o is None else o.ctypes.data_as(VP))

    def device(a, b, n=el):
        return L.mzk_mle_evals_from_coeffs_dev(None if a is None else VP(a), SZ(n), None if b is None else VP(b), VP(s.cuda_stream))

    too_many = ("%d variables" % (sc.SCP_MAX_VARS + 1),)
    bad = coef.copy()
    bad[5] = limbs([P])[0]
    top = coef.copy()
    top[(1 << el) - 1] = limbs([(1 << 256) - 1])[0]
    for call, code, words in [(lambda: host(coef, out, sc.SCP_MAX_VARS + 1), E_LENGTH, too_many),
                              (lambda: device(src.data_ptr(), dst.data_ptr(), sc.SCP_MAX_VARS + 1), E_LENGTH, too_many),
                              (lambda: host(None, out), E_ARG, ("null pointer",)),
                              (lambda: host(coef, None), E_ARG, ("null pointer",)),
                              (lambda: device(None, dst.data_ptr()), E_ARG, ("null pointer",)),
                              (lambda: device(src.data_ptr(), None), E_ARG, ("null pointer",)),
                              (lambda: host(bad, out), E_RANGE, ("coefficient 5 not canonical",)),
                              (lambda: host(top, out), E_RANGE, ("coefficient %d not canonical" % ((1 << el) - 1),)),
                              (lambda: device(src.data_ptr() + 8, dst.data_ptr()), E_ARG, ("alignment",)),
                              (lambda: device(src.data_ptr(), dst.data_ptr() + 8), E_ARG, ("alignment",))]:
        rc = call()
        msg = L.mzk_last_error().decode()
        assert rc == code and all(w in msg for w in words), (rc, msg)
        s.synchronize()
        assert bool((out == 0xA5A5A5A5A5A5A5A5).all()) and bool((dst == 0x5A5A5A5A).all())
        assert np.array_equal(from_device(src)[:1 << el], coef)
    assert np.array_equal(mz.mle_evals_from_coeffs(coef), limbs(sm.evals_over_boolean_hypercube(sc.uniform(el, 1, 9)[0], el)))
