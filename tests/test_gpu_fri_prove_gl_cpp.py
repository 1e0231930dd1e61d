"""Builds and runs tests/cpp/test_fri_prove_gl_mirror.cpp: fri_prove<F> of the C++ mirror (myzkp_amd/host/myzkp.hpp) for the tags M64
and <M64, Ip3> at (64, 4, 4) and (1024, 16, 17) -- roots, top-level indices, last codeword, revealed values and path bytes as printed,
compared with tests/goldilocks_model.py."""
import os, subprocess
import pytest
import orc
import goldilocks_model as gm

ROOT = orc.ROOT
NAME = "test_fri_prove_gl_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)
P = gm.P
SEED = 0x9E3779B97F4A7C15


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_fri_prove_gl_mirror_compiles():
    """CPU: fri_prove<F> instantiated for the two Goldilocks tags compiles and links against mzk_fri_prove_gl."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


def _synth(F, n):
    def word(i):
        v = (i + 1) * SEED % (1 << 64)
        return v - P if v >= P else v
    return [F.from_words([word(i * F.limbs + k) for k in range(F.limbs)]) for i in range(n)]


def _parse(stdout):
    out = {}
    for line in stdout.splitlines():
        f = line.split()
        if len(f) >= 2 and f[0].count(".") >= 2 and f[1].isdigit():
            out.setdefault(f[0], {})[int(f[1])] = f[2:]
    return {k: [d[i] for i in range(len(d))] for k, d in out.items()}


@pytest.mark.gpu
def test_fri_prove_gl_mirror_matches_the_model():
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "fri_prove_gl mirror tests passed" in out.stdout
    got = _parse(out.stdout)
    hexes = lambda es, F: [["%x" % w for w in F.words(e)] for e in es]
    for tag, F in (("m64", gm.M64), ("m64x3", gm.M64X3)):
        for lg, expansion, tests in ((6, 4, 4), (10, 16, 17)):
            n = 1 << lg
            want = gm.prove(F, _synth(F, n), gm.root_of_unity(F, lg), F.from_int(7), expansion, tests)
            pre = "%s.%d." % (tag, lg)
            assert got[pre + "root"] == [[r.hex()] for r in want["merkle_roots"]], pre
            assert got[pre + "top"] == [["%x" % i] for i in want["top_level_indices"]], pre
            assert got[pre + "last"] == hexes(want["last_codeword"], F), pre
            for i, L in enumerate(want["revealed_layers"]):
                for k in "abc":
                    assert got["%svalue.%d.%s" % (pre, i, k)] == hexes(L[k][0], F), (pre, i, k)
                    assert got["%spath.%d.%s" % (pre, i, k)] == [[e.hex() for e in path] for path in L[k][1]], (pre, i, k)
            assert len([key for key in got if key.startswith(pre + "value.")]) == 3 * len(want["revealed_layers"])
