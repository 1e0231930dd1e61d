"""The deterministic pieces of mzk_fri_prove_gl (FRI::prove over M64 and ExtendedFieldElement<M64, Ip3>, zkstark/fri.rs:99-143,
546-594) on the CPU: the Goldilocks functions of myzkp_amd/csrc/mzk_transcript.h compiled for the host
(tests/hostcheck/transcript_gl_shim.cpp) against tests/goldilocks_model.py and tests/fri_prove_model.py -- F::sample mod p, the
packed layout (64-byte path entries, 1 or 3 words per element), the last-codeword writer and the transcript capacity --, the
host-only layout entry point of the built library, and the golden file.  CPU only."""
import ctypes, hashlib, json, os, random, subprocess
import numpy as np
import pytest
import fri_prove_model as fpm
import goldilocks_model as gm
import fri_prove_gl_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
P = gm.P
U64 = ctypes.c_uint64
PATH_STRIDE_GL = 64
FIELDS = [gm.M64, gm.M64X3]
IDS = [F.name for F in FIELDS]
SHAPES = [(64, 4, 4), (64, 2, 3), (1024, 16, 17), (4096, 4, 100), (1 << 20, 4, 17), (1024, 4, 0)]


def layout_gl(limbs, n, expansion_factor, tests):
    """(num_rounds, {section: (offset, size)}, total) of mzk_fri_prove_gl's packed proof: fri_prove_model.layout's sections with
    `limbs` = 1 or 3 words per element and 64 bytes per path entry; every section 8-byte aligned"""
    R = fpm.num_rounds(n, expansion_factor, tests)
    m, L = n >> (R - 1), R - 1
    d = [(n >> r).bit_length() - 1 for r in range(R)]
    entries = sum(tests * (2 * d[i] + d[i + 1]) for i in range(L))
    sizes = [8, 8 * tests, 32 * R, 8 * limbs * m, 8 * limbs * 3 * tests * L, 3 * tests * L, PATH_STRIDE_GL * entries, 8 * entries]
    out, at = {}, 0
    for k, s in zip(fpm.SECTIONS, sizes):
        out[k] = (at, s)
        at += (s + 7) & ~7
    return R, out, at


@pytest.fixture(scope="module")
def txg(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("transcript_gl") / "libtranscript_gl.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "transcript_gl_shim.cpp")])
    L = ctypes.CDLL(so)
    L.txg_sample_gl.restype = U64
    L.txg_sample_gl.argtypes = [U64]
    L.txg_layout.argtypes = [U64, U64, U64, ctypes.c_int, ctypes.POINTER(U64)]
    L.txg_transcript_cap.restype = U64
    L.txg_transcript_cap.argtypes = [U64, U64, U64, ctypes.c_int]
    L.txg_record_len.restype = U64
    L.txg_record_len.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.txg_push_last.restype = U64
    L.txg_push_last.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, U64]
    return L


def test_sample_gl_reduces_the_accumulator_once(txg):
    """digests whose last eight bytes, big-endian, sit on both sides of p: a real transcript reaches the >= p branch with probability
    2^-32, so it is covered here and nowhere else"""
    rng = random.Random(9)
    tails = [0, P - 1, P, P + 1, (1 << 64) - 1]
    digests = [bytes(rng.randrange(256) for _ in range(24)) + t.to_bytes(8, "big") for t in tails]
    digests += [bytes(rng.randrange(256) for _ in range(32)) for _ in range(300)]
    for F in FIELDS:
        for d in digests:
            got = txg.txg_sample_gl(int.from_bytes(d[24:], "little"))
            assert F.from_int(got) == gm.sample(F, d) and got < P, d.hex()
    assert [txg.txg_sample_gl(int.from_bytes(t.to_bytes(8, "big"), "little")) for t in tails] == [0, P - 1, 0, 1, (1 << 32) - 2]


def _shim_layout(txg, n, e, t, limbs):
    out = (U64 * 18)()
    txg.txg_layout(n, e, t, limbs, out)
    return int(out[0]), {k: (int(out[1 + i]), int(out[9 + i])) for i, k in enumerate(fpm.SECTIONS)}, int(out[17])


@pytest.mark.parametrize("n,e,t", SHAPES)
@pytest.mark.parametrize("limbs", [1, 3])
def test_layout_matches_python(txg, n, e, t, limbs):
    want = layout_gl(limbs, n, e, t)
    assert _shim_layout(txg, n, e, t, limbs) == want
    R, sec, total = want
    assert sec["paths"][1] == PATH_STRIDE_GL * sec["path_lens"][1] // 8
    assert all(o % 8 == 0 for o, _ in sec.values()) and total >= sum(s for _, s in sec.values())


def test_library_layout_entry_point():
    """mzk_fri_proof_layout_gl of the built library: host only, no device needed"""
    import myzkp_amd as mz
    for n, e, t in SHAPES:
        for F in FIELDS:
            assert mz.fri_proof_layout_gl(F.fid, n, e, t) == layout_gl(F.limbs, n, e, t)
    bad = [((fid, 256, 4, 17), -1) for fid in (0, 1, 2)]
    bad += [((3, 0, 4, 17), -5), ((4, 1000, 4, 17), -2), ((3, 1024, 512, 17), -5), ((4, 64, 2, 20), -5)]
    for args, code in bad:
        with pytest.raises(mz.MzkError) as ei:
            mz.fri_proof_layout_gl(*args)
        assert ei.value.code == code, args
        if args[0] < 3:
            assert ei.value.message == "fri_prove_gl: bad field id %d" % args[0]
    # the other layout keeps refusing the Goldilocks ids, and the ABI version stays
    for fid in (3, 4):
        with pytest.raises(mz.MzkError) as ei:
            mz.fri_proof_layout(fid, 256, 4, 17)
        assert ei.value.code == -1
    assert mz.lib().mzk_abi_version() == 2


def _words(F, elems):
    return np.array([F.words(e) for e in elems], dtype=np.uint64).reshape(len(elems), F.limbs)


@pytest.mark.parametrize("F", FIELDS, ids=IDS)
@pytest.mark.parametrize("m,rounds", [(16, 3), (32, 2), (128, 4), (512, 4), (2, 2)])
def test_last_codeword_writer_against_the_stream_model(txg, F, m, rounds):
    """the serial writer of mzk_transcript.h over the edge vectors: byte for byte fpm.serialize_stream, every record length, and the
    capacity the driver reserves"""
    v = cases.edge_vector(F, m)
    lens = {len(F.leaf(e)) for e in v}
    if m >= 16:
        assert lens >= ({8, 21, 25, 30, 34, 39, 47, 59} if F.limbs == 3 else {9, 13, 17})
    roots = [hashlib.sha3_256(bytes([r, m & 255])).digest() for r in range(rounds)]
    want = fpm.serialize_stream([[r] for r in roots] + [[F.leaf(e) for e in v]])
    w = _words(F, v)
    for e, row in zip(v, w):
        assert txg.txg_record_len(F.limbs, row.ctypes.data) == 8 + len(F.leaf(e))
    n, expansion, tests = m << (rounds - 1), m // 2, 0                 # a shape with this many rounds and this last length
    assert fpm.num_rounds(n, expansion, tests) == rounds
    cap = txg.txg_transcript_cap(n, expansion, tests, F.limbs)
    assert cap == 8 + 48 * rounds + 8 + m * (8 + (59 if F.limbs == 3 else 17)) and len(want) <= cap
    buf = ctypes.create_string_buffer(b"\xA5" * (cap + 16), cap + 16)
    head = fpm.serialize_stream([[r] for r in roots])
    ctypes.memmove(buf, head, len(head))
    assert txg.txg_push_last(F.limbs, buf, rounds, w.ctypes.data, m) == len(want)
    assert buf.raw[:len(want)] == want
    assert buf.raw[len(want):] == b"\xA5" * (cap + 16 - len(want))
    # all-maximal leaves fill the capacity exactly
    full = [F.from_words([P - 1] * F.limbs)] * m
    assert txg.txg_push_last(F.limbs, buf, rounds, _words(F, full).ctypes.data, m) == cap


def test_golden_vectors_reproduce():
    """tests/golden/fri_prove_gl_vectors.json is what goldilocks_model.prove computes; only test_fri_efield's proof verifies"""
    golden = json.load(open(os.path.join(HERE, "golden", "fri_prove_gl_vectors.json")))
    assert [c["name"] for c in golden] == ["test_fri_efield", "m64_random_64", "m64x3_edge_64"]
    for c in golden:
        F = gm.FIELDS[c["field"]]
        cw = [F.from_words([int(x) for x in e]) for e in c["codeword"]]
        om, off = F.from_int(int(c["omega"])), F.from_int(int(c["offset"]))
        e, t = c["expansion_factor"], c["num_colinearity_tests"]
        proof = gm.prove(F, cw, om, off, e, t)
        assert proof["top_level_indices"] == c["top_level_indices"]
        assert [r.hex() for r in proof["merkle_roots"]] == c["merkle_roots"]
        assert hashlib.sha256(cases.stream_of(F, proof)).hexdigest() == c["stream_sha256"]
        assert gm.verify(F, proof, om, off, len(cw), e, t) == (c["name"] == "test_fri_efield")
    edge = golden[2]
    assert edge["field"] == gm.FIELD_M64X3 and [tuple(int(x) for x in e) for e in edge["codeword"][:10]] == cases.EDGE[gm.FIELD_M64X3]
