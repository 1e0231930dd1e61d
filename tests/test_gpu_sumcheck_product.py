"""mzk_sumcheck_product_prove / _dev and mzk_mle_evals_from_coeffs / _dev: the product sum-check of examples/sumcheck over evaluation
tables in one enqueue, transcript included, against tests/sumcheck_product_model.py (Python integers and hashlib), bit for bit.

  shapes    el = 1, 2, the largest el the tail kernel takes alone (7) and the hand-over from grid rounds (8), several workgroups with
            partials (13) for k = d = 1, 3, 8 and d != k both ways, and 16 as the largest full comparison
  values    all zero, all p - 1, the demo's 0..256, uniform random
  framing   no header; the reference-shaped header; filler lengths that put a hashed stream length on both SHAKE256 padding edges
  forms     _dev == host form, inputs untouched, two proofs back to back on one stream
  el = 20   the model's verifier accepts the library's proof; SUM and FINALS against linear-time Python
  mle       the subset-sum butterfly in and out of place, and coefficients -> tables -> proof end to end

These are the spot shapes of the change that introduced the prover.  The sweep -- all 64 (k, d), every el from 1 to 13 with the
launches counted, el = 21 where a lane of k_sc_round strides, values at the field's edges, three passes of k_mle_pass and the error
paths -- is test_gpu_sumcheck_product_matrix.py, over the shapes and tables of sumcheck_product_cases.py."""
import ctypes, functools, random
import numpy as np
import pytest
import sumcheck_product_model as sm

pytestmark = pytest.mark.gpu
P = sm.P
TAIL_EL = 7               # SC_TAIL_LOG of mzk_sumcheck.hip: 2^7 entries per factor fit the tail's LDS tables


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


@functools.lru_cache(maxsize=None)
def case(el, k, d, kind="random", header_kind="none"):
    """(tables as ints, header objects, the model's proof) -- computed once, shared and never modified"""
    rng = random.Random(1000 * el + 10 * k + d)
    n = 1 << el
    if kind == "zero":
        tables = [[0] * n for _ in range(k)]
    elif kind == "pm1":
        tables = [[P - 1] * n for _ in range(k)]
    elif kind == "demo":
        tables = [[rng.randrange(256) for _ in range(n)] for _ in range(k)]
    else:
        tables = [[rng.randrange(P) for _ in range(n)] for _ in range(k)]
    header = ()
    if header_kind == "reference":
        header = sm.reference_header(d, k, el, [bytes(rng.randrange(256) for _ in range(5 + 8 * f + (f % 3))) for f in range(k)])
    header = tuple(tuple(o) for o in header)
    return tables, header, sm.prove(tables, d, header)


def limbs_of(mz, tables):
    return np.stack([mz.to_limbs(t, 4) for t in tables])


def check(got, want):
    for key in ("sum", "evals", "challenges", "finals", "transcript"):
        assert got[key] == want[key], key


@pytest.mark.parametrize("el,k,d", [(1, 1, 1), (1, 3, 3), (2, 3, 3), (2, 2, 5), (TAIL_EL, 3, 3), (TAIL_EL, 8, 8), (TAIL_EL + 1, 3, 3),
                                    (TAIL_EL + 1, 8, 8), (TAIL_EL + 2, 3, 3), (13, 1, 1), (13, 3, 3), (13, 8, 8), (13, 3, 1), (13, 2, 5),
                                    (16, 3, 3)])
def test_shapes_against_the_model(mz, el, k, d):
    tables, header, want = case(el, k, d)
    check(mz.sumcheck_product_prove(limbs_of(mz, tables), d), want)


@pytest.mark.parametrize("kind", ["zero", "pm1", "demo", "random"])
@pytest.mark.parametrize("el", [2, TAIL_EL + 2])
def test_values(mz, kind, el):
    tables, header, want = case(el, 3, 3, kind)
    got = mz.sumcheck_product_prove(limbs_of(mz, tables), 3)
    check(got, want)
    if kind == "zero":          # every s serializes as the 9-byte zero record: u64 1 | u64 9 | NoSign | u64 0
        zero = (1).to_bytes(8, "little") + (9).to_bytes(8, "little") + bytes(9)
        assert got["transcript"] == (4 * el).to_bytes(8, "little") + zero * (4 * el)
    if kind == "demo" and el > 2:          # short digit counts in round 0, full ones once a 64-bit challenge has been folded in
        objs = sm.deserialize_stream(got["transcript"])
        assert len(objs[0][0]) < 9 + 32 and any(len(o[0]) == 9 + 32 for o in objs[4:])


@pytest.mark.parametrize("el", [3, TAIL_EL + 2])
def test_reference_shaped_header(mz, el):
    tables, header, want = case(el, 3, 3, "random", "reference")
    assert len(header) == 6 and all(len(o[0]) % 8 for o in header[3:])
    got = mz.sumcheck_product_prove(limbs_of(mz, tables), 3, header_objects=header)
    check(got, want)
    assert sm.verify(tables, 3, header, got["sum"], got["transcript"])


@functools.lru_cache(maxsize=None)
def padding_edge_case(el, residue):
    """a header whose last object's length puts the hashed stream length of some round on `residue` mod 136 (from the model)"""
    tables = case(el, 2, 2)[0]
    for filler in range(1, 2 * 136):
        header = tuple(tuple(o) for o in sm.reference_header(2, 2, el, [b"\x07" * 11, bytes(i & 255 for i in range(filler))]))
        want = sm.prove(tables, 2, header)
        if any(ln % 136 == residue for ln in want["hashed_lengths"]):
            return tables, header, want
    return None


@pytest.mark.parametrize("el", [4, TAIL_EL + 2])
@pytest.mark.parametrize("residue", [0, 135])
def test_shake_padding_edges(mz, el, residue):
    found = padding_edge_case(el, residue)
    assert found is not None, "no filler length puts a round's stream length on residue %d: did the record sizes change?" % residue
    tables, header, want = found
    assert any(ln % 136 == residue for ln in want["hashed_lengths"])
    check(mz.sumcheck_product_prove(limbs_of(mz, tables), 2, header_objects=header), want)


def written(mz, el, k, d, header_len, raw):
    """the bytes of a packed proof that the prover defines: everything up to the end of the serialized stream"""
    sec, _ = mz.sumcheck_product_layout(el, k, d, header_len)
    at = sec["transcript_len"][0]
    return raw[:sec["transcript"][0] + int.from_bytes(raw[at:at + 8], "little")]


def test_dev_form_inputs_untouched_and_back_to_back(mz):
    import torch
    el, k, d = TAIL_EL + 3, 3, 3
    cases = [case(el, k, d, "random", "reference"), case(el, k, d, "demo", "reference")]
    arrs = [limbs_of(mz, c[0]) for c in cases]
    headers = [mz.sumcheck_frame_header(c[1]) for c in cases]
    host = [written(mz, el, k, d, len(h), mz.sumcheck_product_prove(a, d, header_objects=c[1], raw=True)) for a, c, h in zip(arrs, cases, headers)]
    ts = [torch.from_numpy(a.view(np.int64)).cuda() for a in arrs]
    for t, a, c, h in zip(ts, arrs, cases, host):          # the Python _dev path: same packed bytes as the host form
        got = mz.sumcheck_product_prove(None, d, header_objects=c[1], device_ptr=t.data_ptr(), num_vars=el, num_factors=k, raw=True)
        assert written(mz, el, k, d, len(mz.sumcheck_frame_header(c[1])), got) == h
        assert np.array_equal(t.cpu().numpy().view(np.uint64), a)
        check(mz.sumcheck_product_unpack(el, k, d, len(mz.sumcheck_frame_header(c[1])), got), c[2])
    totals = [mz.sumcheck_product_layout(el, k, d, len(h))[1] for h in headers]
    outs = [torch.zeros(t, dtype=torch.uint8, device="cuda") for t in totals]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    SZ = ctypes.c_size_t
    for t, o, h, c, total in zip(ts, outs, headers, cases, totals):            # two proofs enqueued, then ONE synchronize
        rc = mz.lib().mzk_sumcheck_product_prove_dev(ctypes.c_void_p(t.data_ptr()), SZ(el), SZ(k), SZ(d), ctypes.c_char_p(h), SZ(len(h)), SZ(len(c[1])),
                                                     ctypes.c_void_p(o.data_ptr()), SZ(total), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0
    s.synchronize()
    for o, h, hd in zip(outs, host, headers):
        assert written(mz, el, k, d, len(hd), o.cpu().numpy().tobytes()) == h


def test_el20_passes_the_models_verifier(mz):
    """linear work in Python: the full model prover is not run at this size"""
    el, k, d = 20, 3, 3
    n = 1 << el
    rng = np.random.default_rng(20)
    arr = np.zeros((k, n, 4), dtype=np.uint64)
    arr[:, :, 0] = rng.integers(0, 1 << 63, size=(k, n), dtype=np.uint64)
    arr[:, :, 1] = rng.integers(0, 1 << 63, size=(k, n), dtype=np.uint64)
    tables = [[int(a) | (int(b) << 64) for a, b in zip(arr[f, :, 0].tolist(), arr[f, :, 1].tolist())] for f in range(k)]
    got = mz.sumcheck_product_prove(arr, d)
    assert got["sum"] == sum(a * b * c for a, b, c in zip(*tables)) % P
    cur = tables
    for r in got["challenges"]:
        cur = [sm.fold(t, r) for t in cur]
    finals = [t[0] for t in cur]
    assert got["finals"] == finals
    assert sm.verify(tables, d, (), got["sum"], got["transcript"], finals=finals)
    evals = [sm.unleaf(o[0]) for o in sm.deserialize_stream(got["transcript"])]
    assert evals == [v for s in got["evals"] for v in s]


MLE_TILE_EL = 10          # MLE_TILE_LOG of mzk_sumcheck.hip: one LDS pass


@pytest.mark.parametrize("el", [1, MLE_TILE_EL, MLE_TILE_EL + 1, 14])
def test_mle_evals_in_place_and_out_of_place(mz, el):
    import torch
    rng = random.Random(el)
    coef = [rng.randrange(P) for _ in range(1 << el)]
    want = mz.to_limbs(sm.evals_over_boolean_hypercube(coef, el), 4)
    c = mz.to_limbs(coef, 4)
    assert np.array_equal(mz.mle_evals_from_coeffs(c), want)                       # host form
    s = torch.cuda.current_stream()
    src = torch.from_numpy(c.view(np.int64)).cuda()
    dst = torch.zeros_like(src)
    mz.mle_evals_from_coeffs(None, device_ptr=src.data_ptr(), num_vars=el, out_ptr=dst.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(dst.cpu().numpy().view(np.uint64), want)
    assert np.array_equal(src.cpu().numpy().view(np.uint64), c)
    mz.mle_evals_from_coeffs(None, device_ptr=src.data_ptr(), num_vars=el, out_ptr=src.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(src.cpu().numpy().view(np.uint64), want)


def test_coefficients_to_proof_end_to_end(mz):
    el, k, d = 8, 3, 3
    rng = random.Random(88)
    coefs = [[rng.randrange(P) for _ in range(1 << el)] for _ in range(k)]
    tables = [sm.evals_over_boolean_hypercube(c, el) for c in coefs]
    header = sm.reference_header(d, k, el, [b"f%d" % f for f in range(k)])
    want = sm.prove(tables, d, header)
    arr = np.stack([mz.mle_evals_from_coeffs(mz.to_limbs(c, 4)) for c in coefs])
    got = mz.sumcheck_product_prove(arr, d, header_objects=header)
    check(got, want)
    assert sm.verify(tables, d, header, got["sum"], got["transcript"])
