"""mzk_fri_prove_gl / mzk_fri_prove_gl_dev: FRI::prove (zkstark/fri.rs:99-143) over MZK_FIELD_M64 and MZK_FIELD_M64X3 in one call, the
proof stream, F::sample mod p, sample_indices and the query phase on the device.  Every case is compared bit for bit with
tests/goldilocks_model.py: the four fields of the unpacked proof, and the packed bytes section by section against a Python packing of
the model's proof (zero padding of every 64-byte path slot, all-zero signs, status 0; the alignment gaps between sections are not
compared)."""
import ctypes
import numpy as np
import pytest
import fri_prove_model as fpm
import goldilocks_model as gm
import fri_prove_gl_cases as cases
from test_fri_prove_gl_model import layout_gl, PATH_STRIDE_GL

pytestmark = pytest.mark.gpu

P = gm.P
E_ARG, E_NOT_POW2, E_LENGTH, E_RANGE = -1, -2, -5, -6
FIELDS = [gm.M64, gm.M64X3]
IDS = [F.name for F in FIELDS]
SZ = ctypes.c_size_t


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def arr(F, elems):
    return np.array([F.words(e) for e in elems], dtype=np.uint64).reshape(len(elems), F.limbs)


def elems(F, a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, F.limbs)
    assert (a < np.uint64(P)).all(), "non-canonical coefficient in an output"
    return [F.from_words(row) for row in a.tolist()]


def pack(F, proof, n, expansion, tests):
    """the model's proof in mzk_fri_prove_gl's packed form: {section: bytes}"""
    words = lambda es: arr(F, es).tobytes()
    out = {"status": bytes(8), "top_indices": np.array(proof["top_level_indices"], dtype=np.uint64).tobytes(),
           "roots": b"".join(proof["merkle_roots"]), "last_codeword": words(proof["last_codeword"])}
    values, paths, lens = [], [], []
    for layer in proof["revealed_layers"]:
        for k in "abc":
            values.append(words(layer[k][0]))
            for path in layer[k][1]:
                for entry in path:
                    assert len(entry) <= PATH_STRIDE_GL
                    paths.append(entry + bytes(PATH_STRIDE_GL - len(entry)))
                    lens.append(len(entry))
    out["values"] = b"".join(values)
    out["signs"] = bytes(3 * tests * len(proof["revealed_layers"]))
    out["paths"] = b"".join(paths)
    out["path_lens"] = np.array(lens, dtype=np.uint64).tobytes()
    return out


def raw_prove(mz, F, cw, omega, offset, expansion, tests):
    """the C entry point itself: the packed bytes"""
    n = len(cw)
    _, _, total = mz.fri_proof_layout_gl(F.fid, n, expansion, tests)
    c, w, o = arr(F, cw), arr(F, [omega]), arr(F, [offset])
    buf = (ctypes.c_uint8 * total)()
    rc = mz.lib().mzk_fri_prove_gl(F.fid, c.ctypes.data_as(ctypes.c_void_p), SZ(n), w.ctypes.data_as(ctypes.c_void_p), o.ctypes.data_as(ctypes.c_void_p),
                                   SZ(expansion), SZ(tests), buf, SZ(total))
    assert rc == 0, mz.lib().mzk_last_error()
    return bytes(buf)


def as_model(F, proof):
    """fri_unpack_proof_gl's dict (rows of words) -> the model's shape (elements)"""
    layers = [{k: (elems(F, L[k][0]), L[k][1]) for k in "abc"} for L in proof["revealed_layers"]]
    return {"top_level_indices": proof["top_level_indices"], "last_codeword": elems(F, proof["last_codeword"]),
            "merkle_roots": proof["merkle_roots"], "revealed_layers": layers}


def same_proof(got, want):
    for k in ("top_level_indices", "last_codeword", "merkle_roots", "revealed_layers"):
        assert got[k] == want[k], k


def check_sections(F, raw, want, n, expansion, tests):
    R, sec, total = layout_gl(F.limbs, n, expansion, tests)
    assert len(raw) == total
    packed = pack(F, want, n, expansion, tests)
    for k in fpm.SECTIONS:
        o, s = sec[k]
        assert len(packed[k]) == s, k
        assert raw[o:o + s] == packed[k], k


def prove_and_compare(mz, F, cw, omega, offset, expansion, tests, want=None):
    """one proof through the C entry point against the model: packed sections, then the four proof fields; returns (unpacked, model)"""
    n = len(cw)
    want = want or gm.prove(F, cw, omega, offset, expansion, tests)
    raw = raw_prove(mz, F, cw, omega, offset, expansion, tests)
    check_sections(F, raw, want, n, expansion, tests)
    got = as_model(F, mz.fri_unpack_proof_gl(F.fid, n, expansion, tests, raw))
    same_proof(got, want)
    return got, want


def scalar(F, e):
    return sum(int(w) << (64 * i) for i, w in enumerate(F.words(e)))


# ---- 1. test_fri_efield (fri.rs:546-594) ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def efield_case():
    F = gm.M64X3
    omega, offset = gm.root_of_unity(F, 10), F.from_int(7)
    coef = [F.from_int(i) for i in range(64)]
    return omega, offset, coef, gm.ntt(F, omega, coef + [F.zero] * (1024 - 64))


def test_fri_efield_matches_the_model_and_verifies(mz, efield_case):
    F = gm.M64X3
    omega, offset, coef, cw = efield_case
    got, want = prove_and_compare(mz, F, cw, omega, offset, 16, 17)
    # the Python wrapper gives the same proof
    same_proof(as_model(F, mz.fri_prove_gl(F.fid, arr(F, cw), scalar(F, omega), scalar(F, offset), 16, 17)), want)
    points = []
    assert gm.verify(F, got, omega, offset, 1024, 16, 17, points)
    assert len(points) == 2 * 17
    for x, y in points:
        assert gm.poly_eval(F, coef, gm.fpow(F, omega, x)) == y


def test_fri_efield_corrupted_codeword_is_rejected(mz, efield_case):
    F = gm.M64X3
    omega, offset, coef, cw = efield_case
    bad = [F.one] * 21 + cw[21:]
    got, _ = prove_and_compare(mz, F, bad, omega, offset, 16, 17)
    assert not gm.verify(F, got, omega, offset, 1024, 16, 17, [])


# ---- 2. every leaf length in every tree: the edge vectors through a periodic codeword ----------------------------------------------------
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n,expansion,tests,rounds,m", [(64, 4, 4, 2, 32), (64, 2, 3, 3, 16), (1024, 16, 17, 4, 128), (2048, 4, 17, 5, 128)])
def test_edge_vectors_through_a_periodic_codeword(mz, F, n, expansion, tests, rounds, m):
    assert fpm.num_rounds(n, expansion, tests) == rounds and n >> (rounds - 1) == m
    v = cases.edge_vector(F, m)
    cw = cases.periodic(v, n)
    lg = n.bit_length() - 1
    omega, offset = gm.root_of_unity(F, lg), F.from_int(7)
    want = gm.prove(F, cw, omega, offset, expansion, tests)
    assert want["last_codeword"] == v                       # every fold had a = b: v's leaf shapes sit in every round's tree
    prove_and_compare(mz, F, cw, omega, offset, expansion, tests, want)
    if F is gm.M64X3 and (n, expansion, tests) in ((64, 4, 4), (1024, 16, 17)):
        # the slots that need the 64-byte stride: a sibling leaf of 59 bytes is revealed
        assert any(len(path[0]) == 59 for L in want["revealed_layers"] for k in "abc" for path in L[k][1])


# ---- 3. a last codeword longer than one scan batch; 4. several fold workgroups and multi-step Merkle levels ----------------------------
@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("n,expansion,tests,rounds,m", [(4096, 4, 100, 4, 512), (1 << 14, 4, 17, 8, 128)])
def test_random_codewords(mz, F, n, expansion, tests, rounds, m):
    assert fpm.num_rounds(n, expansion, tests) == rounds and n >> (rounds - 1) == m
    cw = cases.rand_elems(F, 31 * n + F.fid, n)
    cw[n // 2], cw[n - 1] = F.zero, F.from_words([P - 1] * F.limbs)
    lg = n.bit_length() - 1
    prove_and_compare(mz, F, cw, gm.root_of_unity(F, lg), F.from_int(7), expansion, tests)


# ---- 5. the _dev form --------------------------------------------------------------------------------------------------------------
def test_dev_form_from_a_coset_lde_on_the_device(mz, efield_case):
    import torch
    F = gm.M64X3
    omega, _, coef, _ = efield_case
    offset = F.from_int(7)
    n, expansion, tests = 1024, 16, 17
    want_cw = gm.fast_coset_evaluate(F, coef, offset, omega, n)
    host_raw = raw_prove(mz, F, want_cw, omega, offset, expansion, tests)
    d_coef = torch.from_numpy(arr(F, coef).view(np.int64)).cuda()
    d_cw = torch.empty((n, F.limbs), dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream()
    w, o = arr(F, [omega]), arr(F, [offset])
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = mz.lib().mzk_coset_lde_dev(F.fid, ctypes.c_void_p(d_coef.data_ptr()), SZ(len(coef)), vp(o), vp(w), ctypes.c_void_p(d_cw.data_ptr()), SZ(n),
                                    ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, mz.lib().mzk_last_error()
    got = mz.fri_prove_gl(F.fid, None, scalar(F, omega), scalar(F, offset), expansion, tests, device_ptr=d_cw.data_ptr(), n=n)
    assert elems(F, d_cw.cpu().numpy().view(np.uint64)) == want_cw
    host = mz.fri_unpack_proof_gl(F.fid, n, expansion, tests, host_raw)
    same_proof(as_model(F, got), as_model(F, host))
    # and the packed bytes of the device form, section by section, against the host form's
    _, sec, total = mz.fri_proof_layout_gl(F.fid, n, expansion, tests)
    proof = torch.zeros(total, dtype=torch.uint8, device="cuda")
    rc = mz.lib().mzk_fri_prove_gl_dev(F.fid, ctypes.c_void_p(d_cw.data_ptr()), SZ(n), vp(w), vp(o), SZ(expansion), SZ(tests), ctypes.c_void_p(proof.data_ptr()),
                                       SZ(total), ctypes.c_void_p(s.cuda_stream))
    assert rc == 0, mz.lib().mzk_last_error()
    s.synchronize()
    dev_raw = proof.cpu().numpy().tobytes()
    for k, (off, size) in sec.items():
        assert dev_raw[off:off + size] == host_raw[off:off + size], k


# ---- 6. argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_enqueue_nothing(mz):
    L = mz.lib()
    F = gm.M64X3
    n = 1 << 10
    cw = arr(F, cases.rand_elems(F, 3, n))
    w, o = arr(F, [gm.root_of_unity(F, 10)]), arr(F, [F.from_int(7)])
    _, _, total = mz.fri_proof_layout_gl(F.fid, n, 4, 17)
    buf = (ctypes.c_uint8 * total)()
    sentinel = bytes([0xA5]) * total
    ctypes.memmove(buf, sentinel, total)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)

    def call(fid=F.fid, c=cw, n=n, ww=w, oo=o, exp=4, tests=17, cap=total):
        return L.mzk_fri_prove_gl(fid, vp(c), SZ(n), vp(ww), vp(oo), SZ(exp), SZ(tests), buf, SZ(cap))
    outside = arr(F, [(7, 0, 1)])                        # not in the base field
    big = np.array([[P, 0, 0]], dtype=np.uint64)         # not canonical
    checks = [(dict(fid=0), E_ARG), (dict(fid=1), E_ARG), (dict(fid=2), E_ARG), (dict(c=None), E_ARG), (dict(ww=None), E_ARG),
              (dict(n=0), E_LENGTH), (dict(n=1000), E_NOT_POW2), (dict(exp=512), E_LENGTH), (dict(n=64, exp=2, tests=20), E_LENGTH),
              (dict(cap=total - 1), E_LENGTH), (dict(ww=outside), E_ARG), (dict(oo=outside), E_ARG), (dict(ww=big), E_RANGE), (dict(oo=big), E_RANGE)]
    for kw, code in checks:
        assert call(**kw) == code, kw
        if "fid" in kw:
            assert L.mzk_last_error().decode() == "fri_prove_gl: bad field id %d" % kw["fid"]
        assert bytes(buf) == sentinel, kw
    assert call(fid=gm.FIELD_M64, ww=np.array([P], dtype=np.uint64)) == E_RANGE
    # tests > the last codeword's length cannot pass FRI::num_rounds' own rule with two rounds or more (4 tests < the length before
    # the last halving): the check is the layout's, exercised by the shapes above
    # mzk_fri_prove keeps refusing the Goldilocks ids
    for fid in (gm.FIELD_M64, gm.FIELD_M64X3):
        rc = L.mzk_fri_prove(fid, vp(cw), None, SZ(n), vp(w), vp(o), SZ(4), SZ(17), buf, SZ(total))
        assert rc == E_ARG and L.mzk_last_error().decode() == "fri_prove: bad field id %d" % fid
        assert bytes(buf) == sentinel


def test_ids_of_other_fields_are_refused_by_all_three_entry_points(mz):
    """what tests/test_gpu_field_ids.py checks for the entry points of the other fields: every id but 3 and 4 -- the Montgomery fields
    and ids that name no field -- is MZK_E_ARG in the call's own words, before anything else is looked at (null pointers here)"""
    import torch
    L = mz.lib()
    N = None
    H = np.array([1, 0, 0, 0], dtype=np.uint64).ctypes.data_as(ctypes.c_void_p)
    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    D = ctypes.c_void_p(d.data_ptr())
    out = (ctypes.c_uint8 * 512)()
    for fid in (0, 1, 2, 5, 7, -1):
        calls = [("mzk_fri_proof_layout_gl", (SZ(4), SZ(2), SZ(1), N, N, N, N)),
                 ("mzk_fri_prove_gl", (H, SZ(4), H, H, SZ(2), SZ(1), out, SZ(512))),
                 ("mzk_fri_prove_gl_dev", (D, SZ(4), H, H, SZ(2), SZ(1), D, SZ(512), N))]
        for fn, rest in calls:
            rc = getattr(L, fn)(ctypes.c_int(fid), *rest)
            assert rc == E_ARG and L.mzk_last_error().decode() == "fri_prove_gl: bad field id %d" % fid, (fn, fid, rc, L.mzk_last_error())
    torch.cuda.synchronize()
    assert not d.any().item()
