"""tests/rs_model.py -- the Python restatement of algebra/reedsolomon.rs that the device codec is compared with -- pinned on values
computed once from the reference's definitions, on the outcome of the reference's nine tests (reedsolomon.rs:461-570), and on the
properties a Reed-Solomon code has.  CPU only."""
import itertools, random
import pytest
import rs_model as m


def test_field_is_gf256_mod_0x11d():
    assert m.gf_mul(2, 0x80) == 0x1D                      # x * x^7 = x^8 = x^4 + x^3 + x^2 + 1
    assert m.gf_pow(2, 255) == 1 and all(m.gf_pow(2, e) != 1 for e in (1, 3, 5, 15, 17, 51, 85))      # x has order 255
    for a in range(256):
        for b in range(256):
            assert m.gf_mul(a, b) == m.gf_mul_bits(a, b)
    for a in range(1, 256):
        assert m.gf_mul(a, m.gf_inv(a)) == 1
        assert m.gf_pow(a, 0) == 1 and m.gf_pow(a, 3) == m.gf_mul(a, m.gf_mul(a, a))
    assert m.gf_pow(0, 0) == 1 and m.gf_pow(0, 5) == 0
    rnd = random.Random(1)
    for _ in range(500):
        a, b, c = (rnd.randrange(256) for _ in range(3))
        assert m.gf_mul(a, b) == m.gf_mul(b, a)
        assert m.gf_mul(a, b ^ c) == m.gf_mul(a, b) ^ m.gf_mul(a, c)
        assert m.gf_mul(m.gf_mul(a, b), c) == m.gf_mul(a, m.gf_mul(b, c))


def test_pinned_values():
    rs = m.setup_rs1d(7, 3)
    assert rs.generator_polynomial() == [64, 120, 54, 15, 1]
    assert m.encode_rs1d([9, 1, 7], rs) == [28, 87, 217, 157, 9, 1, 7]
    assert m.encode_rs1d([1, 2, 3], rs) == [161, 29, 145, 45, 1, 2, 3]
    assert m.encode_rs1d([4, 8, 15], rs) == [140, 168, 119, 80, 4, 8, 15]
    assert m.encode_rs1d([2, 4, 6], rs) == [95, 58, 63, 90, 2, 4, 6]
    assert m.encode_rs1d([6, 0, 0], rs) == [157, 13, 180, 34, 6]          # the reference's form: trailing zeros trimmed
    assert m.encode_rs1d([0, 0, 0], rs) == []
    assert rs.encode_fixed([6, 0, 0]) == [157, 13, 180, 34, 6, 0, 0]
    assert rs.encode_fixed([0, 0, 0]) == [0] * 7
    assert m.encode_rs2d([2, 4, 6], m.setup_rs2d(4, 4, 3)) == [[16, 8, 16, 8], [0, 24, 20, 12], [28, 26, 2, 4], [12, 10, 6, 0]]


def _add(code, pos, v):
    code[pos] = (code[pos] + v) & 0xFF          # the reference's tests add in u8 (`code[i] += v`), they do not xor


def test_the_references_five_1d_tests():
    rs = m.setup_rs1d(7, 3)
    code = rs.encode([9, 1, 7])                                            # test_syndrome_computation_no_error
    assert rs.compute_syndromes(code) == [0, 0, 0, 0]
    assert code[4:7] == [9, 1, 7] and m.decode_rs1d(code, rs) == [9, 1, 7]   # test_no_errors
    code = m.encode_rs1d([1, 2, 3], rs)                                    # test_single_error_correction
    _add(code, 3, 10)
    assert m.decode_rs1d(code, rs) == [1, 2, 3]
    code = m.encode_rs1d([4, 8, 15], rs)                                   # test_multiple_error_correction
    _add(code, 1, 7); _add(code, 5, 12)
    assert m.decode_rs1d(code, rs) == [4, 8, 15]
    code = m.encode_rs1d([2, 4, 6], rs)                                    # test_too_many_errors
    _add(code, 0, 3); _add(code, 3, 5); _add(code, 6, 7)
    assert m.decode_rs1d(code, rs) is None


@pytest.mark.parametrize("message, errors", [
    ([2, 4, 6], []),                                                       # test_no_errors_2d
    ([2, 8, 3], [(1, 1, 10)]),                                             # test_single_error_correction_2d
    ([5, 4, 16], [(1, 0, 6), (1, 1, 5)]),                                  # test_multiple_error_correction_2d
    ([8, 2, 3], [(1, 0, 6), (0, 1, 5)]),                                   # test_too_many_errors_2d (which expects success)
])
def test_the_references_four_2d_tests(message, errors):
    rs = m.setup_rs2d(4, 4, 3)
    code = m.encode_rs2d(message, rs)
    assert [code[2][2], code[2][3], code[3][2]] == message
    for r, c, v in errors:
        code[r][c] = (code[r][c] + v) & 0xFF
    assert m.decode_rs2d(code, m.setup_rs2d(4, 4, 3)) == message


def test_every_codeword_has_zero_syndromes():
    rnd = random.Random(2)
    for n in range(1, 21):
        for k in range(1, n + 1):
            rs = m.ReedSolomon(n, k)
            g = rs.generator_polynomial()
            assert len(g) == n - k + 1 and g[-1] == 1
            for msg in ([rnd.randrange(256) for _ in range(k)], [0xFF] * k, [rnd.randrange(256) for _ in range(k - 1)] + [0]):
                cw = rs.encode_fixed(msg)
                assert cw[n - k:] == msg
                assert rs.compute_syndromes(cw) == [0] * (n - k), (n, k, msg)


def test_trimmed_is_fixed_under_zero_extension():
    rnd = random.Random(3)
    for n, k in ((7, 3), (16, 8), (12, 11), (20, 1), (9, 9)):
        rs = m.ReedSolomon(n, k)
        for zeros in range(k + 1):
            msg = [rnd.randrange(1, 256) for _ in range(k - zeros)] + [0] * zeros
            trimmed, fixed = rs.encode(msg), rs.encode_fixed(msg)
            assert len(fixed) == n and fixed[:len(trimmed)] == trimmed and not any(fixed[len(trimmed):])
            assert not trimmed or trimmed[-1] != 0
            assert rs.encode(msg[:k - zeros]) == trimmed                   # a shorter message is the zero-padded one


def test_corrects_every_single_error_at_7_3():
    rs = m.ReedSolomon(7, 3)
    cw = rs.encode_fixed([9, 1, 7])
    for pos in range(7):
        for v in range(1, 256):
            r = list(cw)
            r[pos] ^= v
            assert rs.decode_status(r) == (cw, cw[4:], 1)


@pytest.mark.parametrize("n, k", [(7, 3), (8, 3), (16, 8), (12, 11), (20, 5), (255, 223), (255, 127)])
def test_corrects_up_to_t_errors(n, k):
    rnd = random.Random(n * 256 + k)
    rs = m.ReedSolomon(n, k)
    t = (n - k) // 2
    for e in range(t + 1):
        for _ in range(1 if n == 255 else 6):
            cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
            r = list(cw)
            for pos in rnd.sample(range(n), e):
                r[pos] ^= rnd.randrange(1, 256)
            assert rs.decode_status(r) == (cw, cw[n - k:], e)


def test_exhaustive_pairs_at_7_3():
    rs = m.ReedSolomon(7, 3)
    cw = rs.encode_fixed([4, 8, 15])
    for p, q in itertools.combinations(range(7), 2):
        for v, w in ((1, 1), (0xFF, 1), (7, 0xFF), (0x80, 0x1D)):
            r = list(cw)
            r[p] ^= v
            r[q] ^= w
            assert rs.decode_status(r) == (cw, cw[4:], 2)


def test_beyond_t_is_none_or_another_codeword():
    rnd = random.Random(5)
    seen = set()
    for n, k in ((7, 3), (8, 3), (16, 8)):
        rs = m.ReedSolomon(n, k)
        t = (n - k) // 2
        for _ in range(40):
            cw = rs.encode_fixed([rnd.randrange(256) for _ in range(k)])
            r = list(cw)
            for pos in rnd.sample(range(n), t + 1 + rnd.randrange(2)):
                r[pos] ^= rnd.randrange(1, 256)
            corrected, msg, status = rs.decode_status(r)
            if status == 255:
                assert corrected == r
                seen.add("none")
            else:
                assert corrected != cw and msg == corrected[n - k:]
                seen.add("other")
    assert "none" in seen


def test_2d_round_trips_and_fails_as_a_whole():
    rnd = random.Random(6)
    for col_n, row_n, ml in ((6, 5, 7), (8, 8, 16), (4, 4, 3)):
        rs = m.ReedSolomon2D(col_n, row_n, ml)
        data = [rnd.randrange(256) for _ in range(ml)]
        code = rs.encode(data)
        size = rs.size
        assert [code[col_n - size + i // size][row_n - size + i % size] for i in range(ml)] == data
        assert rs.decode(code) == data
        if (col_n - size) // 2 >= 1:
            hit = [list(r) for r in code]
            for c in range(row_n):
                hit[rnd.randrange(col_n)][c] ^= rnd.randrange(1, 256)
            got, cs, _ = rs.decode_status(hit)
            assert got == data and cs == [1] * row_n
