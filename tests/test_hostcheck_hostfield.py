"""The host field arithmetic every translation unit shares (myzkp_amd/csrc/mzk_hostfield.h) run by tests/hostcheck/hostfield_shim.cpp, a
stand-alone program built with -fsanitize=address,undefined, against Python integers: Fr, Fq and M128 over the edge values
0, 1, 2, p-1, p-2, (p-1)/2, 2^64-1, 2^64 and 300 seeded random values -- add, sub, neg (0 -> 0), the Montgomery product and the bit-serial
one, powers with 64-bit exponents, inverses (0 -> 0), (2^k)^-1 for every k the field admits, and h_mont_words against a 2^(29 L) mod p.
Then the two decisions built on it: the reference's pair of assertions on a root and its order (ntt.rs:75-76 and its siblings) on the
field's own roots, and the Shoup table entries of the transforms (limbs of w^j and of floor(w^j 2^261 / p); Fr, the one field whose
transforms take them).  CPU only; mzk_host_field_op (test_abi_load.py) checks the same arithmetic as the library carries it."""
import os, random, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FR, M128, FQ = 0, 1, 2
P = {FR: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
     FQ: 21888242871839275222246405745257275088696311157297823662689037894645226208583,
     M128: 1 + 407 * (1 << 119)}
LIMBS64 = {FR: 4, FQ: 4, M128: 2}
LIMBS29 = {FR: 9, FQ: 9, M128: 5}
TWO_ADICITY = {FR: 28, FQ: 1, M128: 119}
E_ROOT_ORDER, E_ROOT_PRIM = -3, -4
SAID_ORDER = "assertion failed: primitive_root.pow(root_order).is_one()"
SAID_PRIM = "assertion failed: !primitive_root.pow(root_order / 2).is_one()"


def root(fid, lg):
    """the field's root of unity of order 2^lg"""
    p = P[fid]
    top = {FR: pow(5, (p - 1) >> 28, p), FQ: p - 1, M128: 85408008396924667383611388730472331217}[fid]
    return pow(top, 1 << (TWO_ADICITY[fid] - lg), p)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostfield")
    exe = str(d / "hostfield_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "hostfield_shim.cpp")])

    def run(fid, ops):
        """ops: tuples (name, int ...) -> one output line each"""
        path = str(d / ("ops_%d.txt" % fid))
        with open(path, "w") as f:
            for op in ops:
                f.write(" ".join([op[0]] + ["%x" % v for v in op[1:]]) + "\n")
        r = subprocess.run([exe, str(fid), path], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "ok" and len(lines) == len(ops) + 1, r.stdout[-3000:]
        return lines[:-1]
    return run


def values(fid):
    p = P[fid]
    rnd = random.Random(4400 + fid)
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (1 << 64) - 1, 1 << 64] + [rnd.randrange(p) for _ in range(300)]


@pytest.mark.parametrize("fid", [FR, FQ, M128])
def test_arithmetic_against_python_integers(shim, fid):
    p = P[fid]
    vals = values(fid)
    rnd = random.Random(4500 + fid)
    ops, want = [], []
    for i, a in enumerate(vals):
        # every edge value meets every edge value, a random value two partners
        for b in (vals[:8] if i < 8 else [vals[(7 * i + 3) % len(vals)], vals[i % 8]]):
            ops += [("add", a, b), ("sub", a, b), ("mul", a, b), ("slow", a, b)]
            want += [(a + b) % p, (a - b) % p, a * b % p, a * b % p]
        e = rnd.getrandbits(64)
        ops += [("neg", a), ("inv", a), ("pow", a, e), ("pow", a, i % 3), ("mont", a)]
        want += [-a % p, pow(a, -1, p) if a else 0, pow(a, e, p), pow(a, i % 3, p), (a << (29 * LIMBS29[fid])) % p]
    for k in range(TWO_ADICITY[fid] + 1):
        ops.append(("ninv", k))
        want.append(pow(1 << k, -1, p))
    got = shim(fid, ops)
    for op, w, g in zip(ops, want, got):
        width = 64 if op[0] == "mont" else 16 * LIMBS64[fid]          # the eight words: the upper ones zero for M128
        assert g == "%0*x" % (width, w), (fid, op, g, "%x" % w)


@pytest.mark.parametrize("fid", [FR, FQ, M128])
def test_the_two_assertions_on_a_root_and_its_order(shim, fid):
    top = min(TWO_ADICITY[fid], 63)                                   # root_order is a 64-bit count
    ops, want = [], []
    for k in sorted({1, 2, 3, 5, 14, 20, 28, top} & set(range(1, top + 1))):
        ops.append(("root", root(fid, k), 1 << k))
        want.append("0 ")
        ops.append(("root", pow(root(fid, k), 2, P[fid]), 1 << k))    # of order 2^(k-1): the first assertion holds, the second fails
        want.append("%d %s" % (E_ROOT_PRIM, SAID_PRIM))
        if k < TWO_ADICITY[fid]:
            ops.append(("root", root(fid, k + 1), 1 << k))            # of order 2^(k+1)
            want.append("%d %s" % (E_ROOT_ORDER, SAID_ORDER))
    # an order that is no power of two, T = 8 q for an odd prime q | p - 1 (Fr: 3; M128: 11, as 407 = 11 * 37): its maximal proper
    # divisors are T / 2 and T / q
    if fid != FQ:
        p, q = P[fid], {FR: 3, M128: 11}[fid]
        T = 8 * q
        assert (p - 1) % T == 0
        w = next(w for w in (pow(c, (p - 1) // T, p) for c in range(2, 200)) if pow(w, T // 2, p) != 1 and pow(w, T // q, p) != 1)
        ops += [("root", w, T), ("root", w, 2 * T), ("root", w, T // 2), ("root", 1, T), ("root", 0, T)]
        want += ["0 ", "%d %s" % (E_ROOT_PRIM, SAID_PRIM), "%d %s" % (E_ROOT_ORDER, SAID_ORDER), "%d %s" % (E_ROOT_PRIM, SAID_PRIM),
                 "%d %s" % (E_ROOT_ORDER, SAID_ORDER)]
    assert shim(fid, ops) == want


def test_shoup_entries_of_the_transform_twiddles(shim):
    p = P[FR]
    vs = [pow(root(FR, lg), j, p) for lg in (28, 14, 7) for j in range(64)] + [0, 1, p - 1]
    got = shim(FR, [("shoup", v) for v in vs])
    for v, line in zip(vs, got):
        words = [int(w, 16) for w in line.split()]
        q = (v << 261) // p
        assert len(words) == 32
        assert words[:9] == [(v >> (29 * i)) & 0x1fffffff for i in range(9)], v
        assert words[16:25] == [(q >> (29 * i)) & 0x1fffffff for i in range(9)], v
        assert q < 1 << 261 and set(words[9:16] + words[25:]) == {0xdeadbeef}, v
