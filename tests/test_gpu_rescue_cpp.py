"""Builds and runs tests/cpp/test_rescue_mirror.cpp: the reference's test_rescue_prime (zkstark/rescueprime.rs:602-654) line for line
through the C++ mirror (myzkp_amd/host/myzkp.hpp: struct RescuePrime) with the parameters dumped from
tests/golden/rescue_prime_m128.json -- both hashes, the first and the last row of the trace, the boundary constraints on the trace --
and the ten-link chain of test_fast_stark; every printed element compared with the model of tests/rescue_cases.py."""
import os, subprocess
import pytest
import rescue_cases as rc

ROOT = os.path.dirname(rc.HERE)
NAME = "test_rescue_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_rescue_mirror_compiles():
    """CPU: the mirror's RescuePrime compiles and links against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_rescue_mirror_runs_the_references_test(tmp_path):
    build_exe()
    g = rc.golden()
    c = rc.BY_NAME["reference"]
    kats = [(int(k["input"]), int(k["hash"])) for k in g["kats"]]
    par = tmp_path / "rescue_parameters.txt"
    vals = [v for row in c["mds"] for v in row] + c["rc"] + [v for k in kats for v in k] + [rc.CHAIN_INPUT]
    par.write_text("%d %d %x %x\n%s\n" % (c["m"], c["n"], c["alpha"], c["alphainv"], "\n".join("%x" % v for v in vals)))
    out = subprocess.run([EXE, str(par)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rescue mirror tests passed" in out.stdout and "FAIL" not in out.stdout
    got = {f[0]: int(f[1], 16) for f in (ln.split() for ln in out.stdout.splitlines()) if len(f) == 2 and "." in f[0]}
    a = kats[1][0]
    t = rc.model_trace(c, a)
    assert [got["hash.0"], got["hash.1"]] == [kats[0][1], kats[1][1]] == [rc.model_hash(c, kats[0][0]), t[-1][0]]
    assert [got["trace.first.%d" % i] for i in range(c["m"])] == t[0] == [a, 0]
    assert [got["trace.last.%d" % i] for i in range(c["m"])] == t[-1]
    assert [got["chain.%d" % l] for l in range(10)] == [o for _, o in rc.model_chain(c, rc.CHAIN_INPUT, 10)]
