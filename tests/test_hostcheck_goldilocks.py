"""myzkp_amd/csrc/mzk_gl.h -- the Goldilocks base and cubic-extension arithmetic and the leaf serialisation that the HIP kernels
execute -- compiled for the host with g++ (tests/hostcheck/goldilocks_shim.cpp) and checked operation by operation against Python
integers.  CPU only."""
import ctypes, os, random, subprocess
import pytest
import goldilocks_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
P = gm.P
EDGE = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P - 2, (P - 1) // 2]
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def hc():
    src = os.path.join(HERE, "hostcheck", "goldilocks_shim.cpp")
    so = os.path.join(HERE, "hostcheck", "libgoldilocks_shim.so")
    hdr = os.path.join(os.path.dirname(HERE), "myzkp_amd", "csrc", "mzk_gl.h")
    if not os.path.exists(so) or any(os.path.getmtime(f) > os.path.getmtime(so) for f in (src, hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.gl_base_op.argtypes = [ctypes.c_int, U64, U64, ctypes.POINTER(U64)]
    return lib


@pytest.fixture(scope="module")
def base_values():
    rng = random.Random(64)
    return EDGE + [rng.randrange(P) for _ in range(200)]


def bop(hc, op, a, b=0):
    out = U64()
    assert hc.gl_base_op(op, a, b, ctypes.byref(out)) == 0
    return out.value


def eop(hc, op, a, b=(0, 0, 0)):
    aa, bb, out = (U64 * 3)(*a), (U64 * 3)(*b), (U64 * 3)()
    assert hc.gl_ext_op(op, aa, bb, out) == 0
    return tuple(out)


def test_base_operations_against_python(hc, base_values):
    vals = base_values
    for i, a in enumerate(vals):
        for b in EDGE + [vals[(7 * i + 3) % len(vals)]]:
            assert bop(hc, 0, a, b) == (a + b) % P, ("add", a, b)
            assert bop(hc, 1, a, b) == (a - b) % P, ("sub", a, b)
            assert bop(hc, 3, a, b) == a * b % P, ("mul", a, b)
        assert bop(hc, 2, a) == (-a) % P
        assert bop(hc, 4, a) == a * a % P
        assert bop(hc, 6, a) == (pow(a, -1, P) if a else 0)
        e = vals[(3 * i + 1) % len(vals)]
        assert bop(hc, 5, a, e) == pow(a, e, P)
    assert bop(hc, 5, gm.ROOT_2_32, 1 << 32) == 1 and bop(hc, 5, gm.ROOT_2_32, 1 << 31) == P - 1


def test_reduction_of_any_128_bit_value(hc):
    """reduce128 takes every (lo, hi), not only products of canonical operands: all-ones words, the borrow and the carry path"""
    rng = random.Random(65)
    m = (1 << 64) - 1
    words = [0, 1, (1 << 32) - 1, 1 << 32, m, m - 1, P, P - 1, P + 1, 0xFFFFFFFF00000000]
    cases = [(lo, hi) for lo in words for hi in words] + [(rng.getrandbits(64), rng.getrandbits(64)) for _ in range(2000)]
    for lo, hi in cases:
        assert bop(hc, 7, lo, hi) == (lo + (hi << 64)) % P, (lo, hi)


def test_extension_operations_against_python(hc, base_values):
    rng = random.Random(66)
    F = gm.M64X3
    elems = [(a, b, c) for a in EDGE[:4] + [P - 1] for b in (0, 1 << 32, P - 1) for c in (0, 1, P - 2)]
    elems += [tuple(rng.choice(base_values) for _ in range(3)) for _ in range(200)]
    for i, a in enumerate(elems):
        b = elems[(5 * i + 2) % len(elems)]
        assert eop(hc, 0, a, b) == F.add(a, b) == eop(hc, 5, a, b)
        assert eop(hc, 1, a, b) == F.sub(a, b) == eop(hc, 6, a, b)
        assert eop(hc, 2, a) == F.neg(a)
        assert eop(hc, 3, a, b) == F.mul(a, b) == eop(hc, 8, a, b), (a, b)
        assert eop(hc, 4, a, b) == tuple(x * b[0] % P for x in a) == eop(hc, 7, a, b)
    x = (0, 1, 0)
    assert eop(hc, 3, eop(hc, 3, x, x), x) == (P - 1, 1, 0)            # x^3 = x - 1


def test_leaf_bytes_against_the_model(hc, base_values):
    rng = random.Random(67)
    buf = (ctypes.c_uint8 * 64)()
    for v in base_values:
        n = hc.gl_leaf(1, (U64 * 1)(v), buf)
        assert bytes(buf[:n]) == gm.M64.leaf(v)
    elems = [(0, 0, 0), (5, 0, 0), (0, 5, 0), (0, 0, 5), (P - 1, P - 1, P - 1), (1 << 32, 0, (1 << 32) - 1)]
    elems += [tuple(rng.choice(base_values) for _ in range(3)) for _ in range(200)]
    for e in elems:
        n = hc.gl_leaf(3, (U64 * 3)(*e), buf)
        assert bytes(buf[:n]) == gm.M64X3.leaf(e), e
