"""Builds and runs tests/cpp/test_rs_mirror.cpp: the reference's nine Reed-Solomon tests (algebra/reedsolomon.rs:461-570) through the
C++ mirror (myzkp_amd/host/myzkp.hpp), every printed code compared with tests/rs_model.py."""
import os, subprocess
import pytest
import orc
import rs_model as M

ROOT = orc.ROOT
NAME = "test_rs_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_rs_mirror_compiles():
    """CPU: the mirror's Reed-Solomon items compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_rs_mirror_runs_the_references_nine_tests():
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "rs mirror tests passed" in out.stdout and "FAIL" not in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f and "." in f[0] or f and f[0] == "generator":
            got[f[0]] = [int(x, 16) for x in f[1:]]
    rs = M.setup_rs1d(7, 3)
    assert got["generator"] == rs.generator_polynomial() == [64, 120, 54, 15, 1]
    for msg in ([9, 1, 7], [1, 2, 3], [4, 8, 15], [2, 4, 6]):
        assert got["code." + ".".join(map(str, msg))] == M.encode_rs1d(msg, rs)
    assert got["trimmed.6.0.0"] == M.encode_rs1d([6, 0, 0], rs) == [157, 13, 180, 34, 6]
    assert got["fixed.6.0.0"] == rs.encode_fixed([6, 0, 0])
    for name, msg in (("no_errors_2d", [2, 4, 6]), ("single_error_correction_2d", [2, 8, 3]), ("multiple_error_correction_2d", [5, 4, 16]),
                      ("too_many_errors_2d", [8, 2, 3])):
        want = M.encode_rs2d(msg, M.setup_rs2d(4, 4, 3))
        assert [got["%s.row%d" % (name, r)] for r in range(4)] == want
