"""Builds and runs tests/cpp/test_goldilocks_mirror.cpp: ntt / intt, fast_coset_evaluate and one FRI fold through the C++ mirror
(myzkp_amd/host/myzkp.hpp) for the tags M64 and <M64, Ip3>, every printed output compared with tests/goldilocks_model.py."""
import os, subprocess
import pytest
import orc
import goldilocks_model as gm

ROOT = orc.ROOT
NAME = "test_goldilocks_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)
P = gm.P


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_goldilocks_mirror_compiles():
    """CPU: the mirror's templates instantiated for the two Goldilocks tags compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


def _synth(F, n, seed):
    def word(i):
        v = (i + 1) * seed % (1 << 64)
        return v - P if v >= P else v
    return [F.from_words([word(i * F.limbs + k) for k in range(F.limbs)]) for i in range(n)]


def _parse(stdout):
    out = {}
    for line in stdout.splitlines():
        f = line.split()
        if len(f) >= 3 and "." in f[0] and f[1].isdigit():
            out.setdefault(f[0], {})[int(f[1])] = [int(x, 16) for x in f[2:]]
    return {k: [d[i] for i in range(len(d))] for k, d in out.items()}


@pytest.mark.gpu
def test_goldilocks_mirror_matches_the_model():
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "goldilocks mirror tests passed" in out.stdout
    got = _parse(out.stdout)
    for tag, F in (("m64", gm.M64), ("m64x3", gm.M64X3)):
        omega, offset = gm.root_of_unity(F, 6), F.from_int(7)
        v = _synth(F, 64, 0x9E3779B97F4A7C15)
        assert [F.from_words(w) for w in got[tag + ".ntt"]] == gm.ntt(F, omega, v), tag
        cw = gm.fast_coset_evaluate(F, _synth(F, 24, 0xD1B54A32D192ED03), offset, omega, 64)
        assert [F.from_words(w) for w in got[tag + ".lde"]] == cw, tag
        alpha = _synth(F, 1, 0xA0761D6478BD642F)[0]
        assert [F.from_words(w) for w in got[tag + ".fold"]] == gm.fold(F, cw, alpha, offset, omega), tag
