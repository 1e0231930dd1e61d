"""The deterministic pieces of FRI::prove (zkstark/fri.rs:19-143, algebra/fiat_shamir.rs) on the CPU: the Python model of
tests/fri_prove_model.py against hand-built bincode bytes and literal restatements, and the device header
myzkp_amd/csrc/mzk_transcript.h compiled for the host (tests/hostcheck/transcript_shim.cpp) against hashlib -- the SHAKE256
framing, Blake2b-256, F::sample and the packed proof layout that the kernels of mzk_fri_prove run -- and against the model's leaves
the record writers of M128 and Fr (fri_record_len, fri_record_put, the serial last-codeword push), once more as a stand-alone
program under the sanitizers.  CPU only."""
import ctypes, hashlib, json, os, random, subprocess
import numpy as np
import pytest
import fri_prove_model as fm
import fri_prove_cases as fc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def tx(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("transcript") / "libtranscript.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "transcript_shim.cpp")])
    L = ctypes.CDLL(so)
    L.tx_sample_bytes.restype = ctypes.c_uint64
    L.tx_sample_bytes.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    L.tx_sample_digest_word3.restype = ctypes.c_uint64
    L.tx_sample_digest_word3.argtypes = [ctypes.c_uint64]
    L.tx_num_rounds.argtypes = [ctypes.c_uint64] * 3
    L.tx_blake2b256_seed_counter.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.tx_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
    L.tx_transcript_cap.restype = ctypes.c_uint64
    L.tx_transcript_cap.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    L.tx_record_len.restype = ctypes.c_uint64
    L.tx_record_len.argtypes = [ctypes.c_int, ctypes.c_void_p]
    L.tx_record_put.restype = ctypes.c_uint64
    L.tx_record_put.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_char_p]
    L.tx_push_last.restype = ctypes.c_uint64
    L.tx_push_last.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64]
    return L


def test_stream_bincode_by_hand():
    """Vec<Vec<Vec<u8>>> with two objects: [root] and a codeword of two leaves, bincode 1.x default (u64 LE lengths)"""
    root = bytes(range(32))
    l0, l1 = fm.leaf(5), fm.leaf(0)
    assert l0 == bytes([1]) + (1).to_bytes(8, "little") + (5).to_bytes(4, "little")
    assert l1 == bytes([0]) + bytes(8)                                    # NoSign, no digits
    assert fm.leaf(-(1 << 32)) == bytes([0xFF]) + (2).to_bytes(8, "little") + bytes(4) + (1).to_bytes(4, "little")
    want = ((2).to_bytes(8, "little") + (1).to_bytes(8, "little") + (32).to_bytes(8, "little") + root
            + (2).to_bytes(8, "little") + len(l0).to_bytes(8, "little") + l0 + len(l1).to_bytes(8, "little") + l1)
    assert fm.serialize_stream([[root], [l0, l1]]) == want
    assert fm.fiat_shamir([[root], [l0, l1]]) == hashlib.shake_256(want).digest(32)
    assert fm.serialize_stream([]) == bytes(8)


def test_sample_is_the_wrapping_loop(tx):
    rng = random.Random(3)
    for _ in range(300):
        b = bytes(rng.randrange(256) for _ in range(rng.randrange(0, 48)))
        acc = 0
        for x in b:                                   # usize arithmetic of field.rs:272-278 / fri.rs:19-25
            acc = ((acc << 8) % (1 << 64)) ^ x
        assert fm.sample(b) == acc == int.from_bytes(b[-8:], "big")
        assert tx.tx_sample_bytes(b, len(b)) == acc
        if len(b) == 32:
            assert tx.tx_sample_digest_word3(int.from_bytes(b[24:], "little")) == acc
    assert tx.tx_sample_digest_word3(0x0807060504030201) == 0x0102030405060708


def test_num_rounds_rule_and_boundaries(tx):
    for n in [1 << k for k in range(0, 21)]:
        for e in (1, 2, 4, 8, 64, 1 << 12):
            for t in (0, 1, 4, 17, 100, 1 << 20):
                r = fm.num_rounds(n, e, t)
                assert tx.tx_num_rounds(n, e, t) == r
                if r >= 1:
                    # the loop's last step had 4 t < len, so the reference's `number <= reduced_size` assertion always holds
                    assert t <= n >> (r - 1)
    assert fm.num_rounds(256, 4, 17) == 2 and fm.num_rounds(16384, 4, 17) == 8 and fm.num_rounds(8192, 8, 10) == 8
    assert fm.num_rounds(1024, 512, 17) == 1 and fm.num_rounds(64, 2, 20) == 0           # < 2: MZK_E_LENGTH
    with pytest.raises(AssertionError, match="cannot sample more indices"):
        fm.sample_indices(bytes(32), 64, 4, 5)
    assert len(fm.sample_indices(bytes(32), 64, 4, 4)) == 4


@pytest.mark.parametrize("length", list(range(0, 300)) + [407, 408, 543, 544, 600])
def test_device_shake256_and_blake2b(tx, length):
    msg = bytes((7 * i + length) & 255 for i in range(length))
    out = ctypes.create_string_buffer(32)
    tx.tx_shake256_32(msg, ctypes.c_size_t(length), out)
    assert out.raw == hashlib.shake_256(msg).digest(32)
    tx.tx_blake2b256(msg, ctypes.c_size_t(length), out)
    assert out.raw == hashlib.blake2b(msg, digest_size=32).digest()


def test_device_shake256_long_lengths(tx):
    out = ctypes.create_string_buffer(32)
    for length in range(300, 601):
        msg = os.urandom(length)
        tx.tx_shake256_32(msg, ctypes.c_size_t(length), out)
        assert out.raw == hashlib.shake_256(msg).digest(32), length
        tx.tx_blake2b256(msg, ctypes.c_size_t(length), out)
        assert out.raw == hashlib.blake2b(msg, digest_size=32).digest(), length


def test_sampler_message(tx):
    out = ctypes.create_string_buffer(32)
    seed = hashlib.sha256(b"seed").digest()
    for c in (0, 1, 255, 256, 1 << 20, (1 << 64) - 1):
        tx.tx_blake2b256_seed_counter(seed, c, out)
        assert out.raw == hashlib.blake2b(seed + c.to_bytes(8, "little"), digest_size=32).digest()


def _shim_layout(tx, n, e, t, limbs):
    out = (ctypes.c_uint64 * 18)()
    tx.tx_layout(n, e, t, limbs, out)
    return int(out[0]), {k: (int(out[1 + i]), int(out[9 + i])) for i, k in enumerate(fm.SECTIONS)}, int(out[17])


SHAPES = [(256, 4, 17), (1 << 14, 4, 17), (1 << 16, 4, 17), (1 << 20, 4, 17), (8192, 8, 10), (64, 2, 3), (64, 4, 4), (1 << 10, 4, 0)]


@pytest.mark.parametrize("n,e,t", SHAPES)
@pytest.mark.parametrize("limbs", [2, 4])
def test_layout_matches_python(tx, n, e, t, limbs):
    want = fm.layout(limbs, n, e, t)
    assert _shim_layout(tx, n, e, t, limbs) == want
    R, sec, total = want
    assert sec["paths"][1] == fm.PATH_STRIDE * sec["path_lens"][1] // 8
    assert all(o % 8 == 0 for o, _ in sec.values()) and total >= sum(s for _, s in sec.values())


FIELD_WORDS = [(4, fm.P_M128), (8, fm.P_FR)]              # 32-bit words per element: M128, and Fr (Fq has Fr's form)
LAST_SHAPES = [(2, 2), (16, 3), (128, 4), (512, 4)]        # (last codeword's length m, rounds)


def _u32(vals, nw):
    return np.array([fc.words(v, nw) for v in vals], dtype=np.uint32).reshape(len(vals), nw)


def _record(v):
    return fm.u64le(len(fm.leaf(v))) + fm.leaf(v)


@pytest.mark.parametrize("nw,p", FIELD_WORDS, ids=["M128", "Fr"])
def test_leaf_records_against_the_model(tx, nw, p):
    """fri_record_len / fri_record_put over the edge values with both signs: every trimmed word count 0 .. nw, the zero element
    (NoSign whatever the flag says) and Sign::Minus; nothing written past the record"""
    edge = fc.edge_values(p, nw)
    assert {len(fm.leaf(v)) for v in edge} == {9 + 4 * k for k in range(nw + 1)}
    for v in edge + [-v for v in edge]:
        for negative in ((1,) if v < 0 else (0, 1) if v == 0 else (0,)):
            w = _u32([v], nw)
            want = _record(v)
            assert tx.tx_record_len(nw, w.ctypes.data) == len(want), v
            buf = ctypes.create_string_buffer(b"\xA5" * (len(want) + 16), len(want) + 16)
            assert tx.tx_record_put(nw, w.ctypes.data, negative, buf) == len(want), v
            assert buf.raw == want + b"\xA5" * 16, v


@pytest.mark.parametrize("nw,p", FIELD_WORDS, ids=["M128", "Fr"])
@pytest.mark.parametrize("m,rounds", LAST_SHAPES)
def test_last_codeword_writer_against_the_stream_model(tx, nw, p, m, rounds):
    """the serial writer of mzk_transcript.h over the edge vector: byte for byte fm.serialize_stream, and the capacity the driver
    reserves"""
    v = fc.edge_vector(p, nw, m)
    roots = [hashlib.sha3_256(bytes([r, m & 255])).digest() for r in range(rounds)]
    want = fm.serialize_stream([[r] for r in roots] + [[fm.leaf(e) for e in v]])
    n, expansion, tests = m << (rounds - 1), m // 2, 0                 # a shape with this many rounds and this last length
    assert fm.num_rounds(n, expansion, tests) == rounds
    cap = tx.tx_transcript_cap(n, expansion, tests, nw)
    assert cap == 8 + 48 * rounds + 8 + m * (8 + 9 + 4 * nw) and len(want) <= cap
    buf = ctypes.create_string_buffer(b"\xA5" * (cap + 16), cap + 16)
    head = fm.serialize_stream([[r] for r in roots])
    ctypes.memmove(buf, head, len(head))
    assert tx.tx_push_last(nw, buf, rounds, _u32(v, nw).ctypes.data, m) == len(want)
    assert buf.raw[:len(want)] == want
    assert buf.raw[len(want):] == b"\xA5" * (cap + 16 - len(want))
    # all-maximal leaves fill the capacity exactly
    assert tx.tx_push_last(nw, buf, rounds, _u32([p - 1] * m, nw).ctypes.data, m) == cap


def test_record_writers_stand_alone_under_the_sanitizers(tmp_path):
    """the same writers in a program of their own, built with -fsanitize=address,undefined: every record and every stream goes into a
    heap block of exactly its length"""
    exe, inp = str(tmp_path / "transcript_shim_san"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "transcript_shim.cpp")])
    cases = [(nw, rounds, fc.edge_vector(p, nw, m)) for nw, p in FIELD_WORDS for m, rounds in LAST_SHAPES]
    with open(inp, "w") as f:
        for nw, rounds, v in cases:
            f.write("%d %d %d %s\n" % (nw, rounds, len(v), " ".join("%x" % w for e in v for w in fc.words(e, nw))))
    r = subprocess.run([exe, inp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines.pop() == "ok %d" % len(cases)
    for nw, rounds, v in cases:
        for e in v:
            kind, plus, minus = lines.pop(0).split()
            assert kind == "R" and bytes.fromhex(plus) == _record(e) and bytes.fromhex(minus) == _record(-e), (nw, e)
        kind, stream = lines.pop(0).split()
        assert kind == "S" and bytes.fromhex(stream) == fm.serialize_stream([[bytes(32)]] * rounds + [[fm.leaf(e) for e in v]]), (nw, len(v))
    assert not lines


def test_library_layout_entry_point():
    """mzk_fri_proof_layout of the built library: host only, no device needed"""
    import myzkp_amd as mz
    for n, e, t in SHAPES:
        for fid, limbs in ((mz.FIELD_M128, 2), (mz.FIELD_FR, 4)):
            assert mz.fri_proof_layout(fid, n, e, t) == fm.layout(limbs, n, e, t)
    for args, code in (((7, 256, 4, 17), -1), ((1, 0, 4, 17), -5), ((1, 1000, 4, 17), -2), ((1, 1024, 512, 17), -5), ((1, 64, 2, 20), -5)):
        with pytest.raises(mz.MzkError) as ei:
            mz.fri_proof_layout(*args)
        assert ei.value.code == code


def test_golden_vectors_reproduce():
    """tests/golden/fri_prove_vectors.json is what the model computes (and its proofs verify)"""
    cases = json.load(open(os.path.join(HERE, "golden", "fri_prove_vectors.json")))
    assert [c["name"] for c in cases] == ["test_fri_field_m128", "fr_random_64", "m128_signed_64"]
    for c in cases:
        p = fm.P_FR if c["field"] == 0 else fm.P_M128
        cw = [int(v) for v in c["codeword"]]
        om, off, e, t = int(c["omega"]), int(c["offset"]), c["expansion_factor"], c["num_colinearity_tests"]
        proof, stream = fm.prove(p, cw, om, off, e, t)
        assert proof["top_level_indices"] == c["top_level_indices"]
        assert [r.hex() for r in proof["merkle_roots"]] == c["merkle_roots"]
        assert hashlib.sha256(stream).hexdigest() == c["stream_sha256"]
        # only the low-degree codeword of test_fri_field verifies; the random ones fail the last codeword's degree check
        assert fm.verify(p, proof, om, off, len(cw), e, t) == (c["name"] == "test_fri_field_m128")
    assert any(int(v) < 0 for v in cases[2]["codeword"])
