"""The product sum-check (examples/sumcheck) on the CPU: the Python model of tests/sumcheck_product_model.py against itself (prover
against verifier), against brute force and against hand-built bytes; the device header myzkp_amd/csrc/mzk_sumcheck_tx.h compiled for
the host (tests/hostcheck/sumcheck_tx_shim.cpp) against the model; and what the library's entry points decide before any device
work.  CPU only."""
import ctypes, os, random, subprocess
import numpy as np
import pytest
import fri_prove_model as fm
import sumcheck_product_model as sm

HERE = os.path.dirname(os.path.abspath(__file__))
P = sm.P


def tables_for(el, k, seed):
    rng = random.Random(seed)
    return [[rng.randrange(P) for _ in range(1 << el)] for _ in range(k)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("sumcheck_tx") / "libsumcheck_tx.so")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC", "-shared", "-o", so,
                           os.path.join(HERE, "hostcheck", "sumcheck_tx_shim.cpp")])
    L = ctypes.CDLL(so)
    L.sctx_write_record.restype = ctypes.c_size_t
    L.sctx_write_record.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    L.sctx_header_ok.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t]
    L.sctx_layout.argtypes = [ctypes.c_uint64] * 4 + [ctypes.POINTER(ctypes.c_uint64)]
    return L


@pytest.mark.parametrize("el", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("d", [1, 3])
def test_prover_passes_verifier_and_tampering_is_rejected(el, k, d):
    tables = tables_for(el, k, 100 * el + 10 * k + d)
    header = sm.reference_header(d, k, el, [b"factor-%d" % f for f in range(k)])
    pr = sm.prove(tables, d, header)
    assert pr["sum"] == sm.claimed_sum(tables)
    # s_j has degree k in its variable, so d + 1 points determine it only when d >= k: the reference's verifier (verifier.rs:53-73)
    # interpolates through them and accepts exactly then.  The prover runs either way (max_degree is an input of its own).
    assert sm.verify(tables, d, header, pr["sum"], pr["transcript"]) == (d >= k)
    assert len(pr["evals"]) == el and all(len(s) == d + 1 for s in pr["evals"]) and len(pr["finals"]) == k
    assert all(r < 1 << 64 for r in pr["challenges"])
    # a flipped s value: the record of s_0(0) starts right after the header; flip the lowest bit of its sign / first digit
    raw = bytearray(pr["transcript"])
    at = 8 + len(sm.frame_header(header)) + 16
    raw[at + (9 if raw[at] else 0)] ^= 1
    assert not sm.verify(tables, d, header, pr["sum"], bytes(raw))
    assert not sm.verify(tables, d, header, (pr["sum"] + 1) % P, pr["transcript"])
    # a flipped challenge byte: bytes that only the hash sees (the last factor object) change r_0 and with it every later check
    if d >= k and el > 1:
        bad_header = [list(o) for o in header]
        bad_header[-1] = [bytes([bad_header[-1][0][0] ^ 1]) + bad_header[-1][0][1:]]
        forged = fm.serialize_stream(bad_header + sm.deserialize_stream(pr["transcript"])[len(header):])
        assert not sm.verify(tables, d, bad_header, pr["sum"], forged)


def test_verifier_accepts_exactly_when_the_degree_bound_holds():
    tables = tables_for(4, 3, 5)
    assert sm.verify(tables, 3, (), sm.claimed_sum(tables), sm.prove(tables, 3)["transcript"])
    assert sm.verify(tables, 5, (), sm.claimed_sum(tables), sm.prove(tables, 5)["transcript"])
    assert not sm.verify(tables, 1, (), sm.claimed_sum(tables), sm.prove(tables, 1)["transcript"])


def test_flipped_challenge_is_rejected():
    """the verifier re-derives r_j from the stream: a proof whose later rounds were made with another r_0 fails"""
    tables = tables_for(3, 2, 9)
    pr = sm.prove(tables, 2)
    objs = sm.deserialize_stream(pr["transcript"])
    r0 = pr["challenges"][0] ^ (1 << 8)                         # one flipped challenge byte
    cur = [sm.fold(t, r0) for t in tables]
    forged = objs[:3]
    for _ in range(2):
        s = sm.round_evals(cur, 2)
        forged += [[fm.leaf(v)] for v in s]
        cur = [sm.fold(t, sm.challenge(forged)) for t in cur]
    assert not sm.verify(tables, 2, (), pr["sum"], fm.serialize_stream(forged))


def test_sum_and_rounds_against_brute_force():
    el, k, d = 3, 2, 2
    tables = tables_for(el, k, 1)
    pr = sm.prove(tables, d)
    n = 1 << el
    assert pr["sum"] == sum(tables[0][x] * tables[1][x] for x in range(n)) % P

    def mle(t, point):            # multilinear extension, variable 0 = the most significant index bit
        total = 0
        for x in range(n):
            w = 1
            for i, r in enumerate(point):
                bit = (x >> (el - 1 - i)) & 1
                w = w * (r if bit else 1 - r) % P
            total += t[x] * w
        return total % P
    r = pr["challenges"]
    assert pr["finals"] == [mle(t, r) for t in tables]
    for c in range(d + 1):        # s_1(c) = sum over the last variable of the product at (r_0, c, x_2)
        assert pr["evals"][1][c] == sum(mle(tables[0], [r[0], c, b]) * mle(tables[1], [r[0], c, b]) for b in (0, 1)) % P


def test_hypercube_tables_from_monomial_coefficients():
    el = 3
    rng = random.Random(4)
    coef = [rng.randrange(P) for _ in range(1 << el)]
    assert sm.evals_over_boolean_hypercube(coef, el) == [sm.eval_monomials_direct(coef, el, b) for b in range(1 << el)]
    assert sm.evals_over_boolean_hypercube([5], 0) == [5]
    # x_0 alone (the most significant bit of the index) is 1 on the upper half of the table
    assert sm.evals_over_boolean_hypercube([0, 0, 0, 0, 1, 0, 0, 0], 3) == [0, 0, 0, 0, 1, 1, 1, 1]


def test_stream_by_hand():
    """header of three 8-byte objects, one round, d = 1: tables [3], [2^32] -> s_0(0) = 3, s_0(1) = 2^32"""
    u = lambda x: x.to_bytes(8, "little")
    header = sm.reference_header(1, 1, 1, [])
    framed = u(1) + u(8) + u(1) + u(1) + u(8) + u(1) + u(1) + u(8) + u(1)
    assert sm.frame_header(header) == framed
    pr = sm.prove([[3, 1 << 32]], 1, header)
    rec0 = u(1) + u(13) + bytes([1]) + u(1) + (3).to_bytes(4, "little")
    rec1 = u(1) + u(17) + bytes([1]) + u(2) + bytes(4) + (1).to_bytes(4, "little")
    want = u(5) + framed + rec0 + rec1
    assert pr["transcript"] == want and pr["hashed_lengths"] == [len(want)]
    assert pr["evals"] == [[3, 1 << 32]] and pr["sum"] == 3 + (1 << 32)
    import hashlib
    r = int.from_bytes(hashlib.shake_256(want).digest(32)[24:], "big")
    assert pr["challenges"] == [r] and pr["finals"] == [(3 + r * ((1 << 32) - 3)) % P]


def _words(v):
    return (ctypes.c_uint32 * 8)(*[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)])


@pytest.mark.parametrize("v", [0, 1, (1 << 32) - 1, 1 << 32, 1 << 224, P - 1])
def test_record_writer_matches_the_model(shim, v):
    out = ctypes.create_string_buffer(shim.sctx_record_max())
    n = shim.sctx_write_record(_words(v), out)
    assert out.raw[:n] == fm.serialize_stream([[fm.leaf(v)]])[8:]
    assert n <= sm.RECORD_MAX == shim.sctx_record_max()


def test_header_parser(shim):
    header = sm.frame_header(sm.reference_header(3, 3, 5, [b"abc", b"", b"0123456789abc"]))
    assert shim.sctx_header_ok(header, len(header), 6) == 1
    assert shim.sctx_header_ok(b"", 0, 0) == 1
    assert shim.sctx_header_ok(header, len(header), 5) == 0 and shim.sctx_header_ok(header, len(header), 7) == 0
    for cut in (1, 7, 8, 13, len(header) - 1):
        assert shim.sctx_header_ok(header[:len(header) - cut], len(header) - cut, 6) == 0          # truncated
    assert shim.sctx_header_ok(header + b"\0", len(header) + 1, 6) == 0                              # over-long
    assert shim.sctx_header_ok(header + bytes(8), len(header) + 8, 6) == 0
    assert shim.sctx_header_ok(header + bytes(8), len(header) + 8, 7) == 1                           # an object of no strings
    huge = (1).to_bytes(8, "little") + ((1 << 64) - 1).to_bytes(8, "little") + b"x"
    assert shim.sctx_header_ok(huge, len(huge), 1) == 0
    assert shim.sctx_header_ok(((1 << 63)).to_bytes(8, "little"), 8, 1) == 0
    assert shim.sctx_header_ok(b"", 0, 1) == 0


GRID = [(el, k, d, hl) for el in (1, 2, 7, 8, 13, 30) for k in (1, 3, 8) for d in (1, 3, 8) for hl in (0, 24, 77, 1000)]


def test_layout_shim_and_library_agree_with_the_model(shim):
    import myzkp_amd as mz
    for el, k, d, hl in GRID:
        want = sm.layout(el, k, d, hl)
        out = (ctypes.c_uint64 * 15)()
        shim.sctx_layout(el, k, d, hl, out)
        assert ({s: (int(out[i]), int(out[7 + i])) for i, s in enumerate(sm.SECTIONS)}, int(out[14])) == want
        assert mz.sumcheck_product_layout(el, k, d, hl) == want
        sec, total = want
        assert all(o % 8 == 0 for o, _ in sec.values()) and total % 8 == 0
        assert sec["transcript"][1] == 8 + hl + el * (d + 1) * (16 + 41)


def test_entry_point_argument_errors():
    """everything the three entry points decide before device work (no GPU needed)"""
    import myzkp_amd as mz
    L = mz.lib()
    SZ = ctypes.c_size_t
    for args, code in (((0, 3, 3, 0), -5), ((31, 3, 3, 0), -5), ((4, 0, 3, 0), -1), ((4, 9, 3, 0), -1), ((4, 3, 0, 0), -1), ((4, 3, 9, 0), -1),
                       ((4, 3, 3, (1 << 40) + 1), -5), ((4, 3, 3, (1 << 64) - 8), -5)):
        with pytest.raises(mz.MzkError) as ei:
            mz.sumcheck_product_layout(*args)
        assert ei.value.code == code
    el, k, d = 2, 2, 2
    tables = mz.to_limbs([1, 2, 3, 4, 5, 6, 7, 8], 4)
    header = mz.sumcheck_frame_header(sm.reference_header(d, k, el, [b"a", b"b"]))
    _, total = mz.sumcheck_product_layout(el, k, d, len(header))
    buf = (ctypes.c_uint8 * total)()
    hb = ctypes.c_char_p(header)
    tp = tables.ctypes.data_as(ctypes.c_void_p)

    def host(t=tp, el=el, k=k, d=d, h=hb, hl=len(header), ho=5, out=buf, cap=total):
        return L.mzk_sumcheck_product_prove(t, SZ(el), SZ(k), SZ(d), h, SZ(hl), SZ(ho), out, SZ(cap))

    def dev(t=ctypes.c_void_p(4096), el=el, k=k, d=d, h=hb, hl=len(header), ho=5, out=ctypes.c_void_p(8192), cap=total):
        return L.mzk_sumcheck_product_prove_dev(t, SZ(el), SZ(k), SZ(d), h, SZ(hl), SZ(ho), out, SZ(cap), None)
    for call in (host, dev):
        assert call(t=None) == -1 and call(out=None) == -1 and call(h=None) == -1
        assert call(k=0) == -1 and call(k=9) == -1 and call(d=0) == -1 and call(d=9) == -1
        assert call(el=0) == -5 and call(el=31) == -5
        assert call(cap=total - 1) == -5
        assert call(ho=4) == -1 and call(ho=6) == -1 and call(hl=len(header) - 1) == -1
        assert b"header" in L.mzk_last_error()
    bad = tables.copy()
    bad[5] = mz.to_limbs([sm.P], 4)[0]
    assert host(t=bad.ctypes.data_as(ctypes.c_void_p)) == -6
    assert b"not canonical" in L.mzk_last_error()
    coef = mz.to_limbs([1, 2, 3, 4], 4)
    out = np.zeros_like(coef)
    cp, op = coef.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)
    assert L.mzk_mle_evals_from_coeffs(None, SZ(2), op) == -1 and L.mzk_mle_evals_from_coeffs(cp, SZ(2), None) == -1
    assert L.mzk_mle_evals_from_coeffs(cp, SZ(31), op) == -5
    assert L.mzk_mle_evals_from_coeffs(bad.ctypes.data_as(ctypes.c_void_p), SZ(3), op) == -6
    assert L.mzk_mle_evals_from_coeffs_dev(None, SZ(2), ctypes.c_void_p(4096), None) == -1
    assert L.mzk_mle_evals_from_coeffs_dev(ctypes.c_void_p(4096), SZ(31), ctypes.c_void_p(4096), None) == -5
