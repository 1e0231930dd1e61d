"""Builds and runs tests/cpp/test_hypercube_mirror.cpp: SumCheckProverGPU::prove(max_degree, factors, header) of the C++ mirror
(myzkp_amd/host/myzkp.hpp) on MPolynomial factors (el = 9, k = 3, d = 3, one factor not multilinear, one with short keys) equals the
table overload on tables from evals_over_boolean_hypercube(factor, el), and both equal tests/sumcheck_product_model.py on the tables
of tests/hypercube_model.py: the claimed sum and the SHA-256 of the proof stream."""
import hashlib, os, subprocess
import pytest
import orc
import hypercube_model as hm
import sumcheck_product_model as sm

ROOT = orc.ROOT
NAME = "test_hypercube_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)
SEED = (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xA0761D6478BD642F)
M64 = (1 << 64) - 1


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def factors_of(el, k):
    """the factors of the C++ program as dictionaries (a later assignment to a key replaces the earlier one, as there)"""
    out = []
    for f in range(k):
        d = {}
        for t in range(11 + 7 * f):
            mask = ((t + 1) * (2 * f + 3) * 37) & ((1 << el) - 1)
            key = [((1 + (t + i) % 3) if f == 1 else 1) if (mask >> (el - 1 - i)) & 1 else 0 for i in range(el)]
            if f == 2:
                while key and key[-1] == 0:
                    key.pop()
            d[tuple(key)] = ((t + 1) * SEED[f]) & M64
        out.append(d)
    out[1][(2,) + (0,) * (el - 1)] = 1002
    out[1][(5,) + (0,) * (el - 1)] = 1005
    return out


def test_hypercube_mirror_compiles():
    """CPU: the mirror's MPolynomial overloads compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_hypercube_mirror_matches_the_model():
    el, k, d = 9, 3, 3
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "hypercube mirror tests passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if len(f) >= 2 and f[0].endswith(".sum"):
            got[f[0]] = sum(int(w, 16) << (64 * i) for i, w in enumerate(f[1:]))
        elif len(f) == 2 and f[0].endswith(".proof"):
            got[f[0]] = hashlib.sha256(bytes.fromhex(f[1])).hexdigest()
    factors = factors_of(el, k)
    assert any(max(key, default=0) > 1 for key in factors[1]) and any(len(key) < el for key in factors[2])
    tables = [hm.evals([(c, key) for key, c in f.items()], el) for f in factors]
    header = sm.reference_header(d, k, el, [bytes([0xA0 + f]) * (f + 2) for f in range(k)])
    want = sm.prove(tables, d, header)
    for tag in ("terms", "tables"):
        assert got[tag + ".sum"] == want["sum"], tag
        assert got[tag + ".proof"] == hashlib.sha256(want["transcript"]).hexdigest(), tag
