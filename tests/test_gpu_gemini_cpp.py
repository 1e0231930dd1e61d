"""Builds and runs tests/cpp/test_gemini_mirror.cpp: the Gemini / sum-check functions of the C++ mirror (myzkp_amd/host/myzkp.hpp)
on the reference's test_gemini and test_sumcheck_pipeline cases, every value and point compared with tests/golden/gemini_vectors.json."""
import json, os, subprocess
import pytest
import orc

ROOT = orc.ROOT
NAME = "test_gemini_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_gemini_mirror_compiles():
    """CPU: the mirror's Gemini / sum-check functions (the prove_sumcheck template instantiated) compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


def _parse(stdout):
    out = {}
    for line in stdout.splitlines():
        f = line.split()
        if len(f) < 6 or "." not in f[0]:
            continue
        limbs = [int(x, 16) for x in f[2:]]
        v = sum(l << (64 * k) for k, l in enumerate(limbs[:4]))
        val = v if len(limbs) == 4 else [v, sum(l << (64 * k) for k, l in enumerate(limbs[4:]))]
        out.setdefault(f[0], {})[int(f[1])] = val
    return {k: [d[i] for i in range(len(d))] for k, d in out.items()}


@pytest.mark.gpu
def test_gemini_mirror_matches_golden():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "gemini_vectors.json")))
    s = d["sumcheck"]
    build_exe()
    args = [EXE, str(d["alpha"]), str(d["max_d"])] + [str(r) for r in s["rs"]] + [str(s["beta"])]
    out = subprocess.run(args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "gemini mirror tests passed" in out.stdout
    got = _parse(out.stdout)
    for tag in ("gemini", "sumcheck"):
        g = d[tag]
        assert got[tag + ".commit"] == g["commits"], tag
        assert got[tag + ".y"] == [y for ys in g["ys"] for y in ys], tag
        assert got[tag + ".w"] == g["ws"], tag
        assert got[tag + ".deg"] == g["deg"], tag
    assert [list(x) for x in zip(got["sumcheck.a"], got["sumcheck.b"])] == s["gs"]
    assert got["sumcheck.r"] == s["rs"] and got["sumcheck.beta"] == [s["beta"]]
