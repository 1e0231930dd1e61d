"""The deterministic pieces of FRI::prove (zkstark/fri.rs:19-143, algebra/fiat_shamir.rs) on the CPU: the Python model of
tests/fri_prove_model.py against hand-built bincode bytes and literal restatements, and the device header
myzkp_amd/csrc/mzk_transcript.h compiled for the host (tests/hostcheck/transcript_shim.cpp) against hashlib -- the SHAKE256
framing, Blake2b-256, F::sample and the packed proof layout that the kernels of mzk_fri_prove run.  CPU only."""
import ctypes, hashlib, json, os, random, subprocess
import pytest
import fri_prove_model as fm

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
