"""Builds and runs tests/cpp/test_sumcheck_product_mirror.cpp: SumCheckProverGPU of the C++ mirror (myzkp_amd/host/myzkp.hpp) proves
el = 8, k = 3, d = 3 with the reference-shaped header; the claimed sum and the SHA-256 of the proof stream are compared with
tests/sumcheck_product_model.py, for given tables and for tables made from coefficients by evals_over_boolean_hypercube."""
import hashlib, os, subprocess
import pytest
import orc
import sumcheck_product_model as sm

ROOT = orc.ROOT
NAME = "test_sumcheck_product_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)
SEED = (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xA0761D6478BD642F)
M64 = (1 << 64) - 1


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_sumcheck_product_mirror_compiles():
    """CPU: the mirror's SumCheckProverGPU compiles and links against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_sumcheck_product_mirror_matches_the_model():
    el, k, d = 8, 3, 3
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "sumcheck product mirror tests passed" in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if len(f) >= 2 and f[0].endswith(".sum"):
            got[f[0]] = sum(int(w, 16) << (64 * i) for i, w in enumerate(f[1:]))
        elif len(f) == 2 and f[0].endswith(".proof"):
            got[f[0]] = hashlib.sha256(bytes.fromhex(f[1])).hexdigest()
    tables = [[(((x + 1) * s) & M64) | ((((x + 7) * s) & M64) << 64) for x in range(1 << el)] for s in SEED]
    header = sm.reference_header(d, k, el, [bytes([0xA0 + f]) * (f + 2) for f in range(k)])
    for tag, tabs in (("tables", tables), ("coefs", [sm.evals_over_boolean_hypercube(t, el) for t in tables])):
        want = sm.prove(tabs, d, header)
        assert got[tag + ".sum"] == want["sum"], tag
        assert got[tag + ".proof"] == hashlib.sha256(want["transcript"]).hexdigest(), tag
