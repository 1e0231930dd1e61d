"""Builds and runs tests/cpp/test_celestia_mirror.cpp: the reference's test_celestia (das/celestia.rs:196-231) line for line through the
C++ mirror (myzkp_amd/host/myzkp.hpp: struct Celestia), then the celestia arm of examples/da.rs for data sizes 16, 64, 256, 1024;
every printed commitment compared with tests/das_model.py over the code of tests/rs_model.py."""
import os, subprocess
import pytest
import orc
import das_model as M
import rs_model as R

ROOT = orc.ROOT
NAME = "test_celestia_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_celestia_mirror_compiles():
    """CPU: the mirror's Celestia compiles and links against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_celestia_mirror_runs_the_references_test_and_example():
    build_exe()
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "celestia mirror tests passed" in out.stdout and "FAIL" not in out.stdout
    got = {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f and "." in f[0]:
            got[f[0]] = bytes(int(x, 16) for x in f[1:])
    cases = [("test_celestia", list(range(64)), 16)] + [("da%d" % n, [i % 256 for i in range(n)], 2 * s) for n, s in ((16, 4), (64, 8), (256, 16), (1024, 32))]
    for name, data, side in cases:
        code = R.encode_rs2d(data, R.setup_rs2d(side, side, len(data)))
        rr, cr, dr = M.celestia_commit(code)
        assert [got["%s.row.%d" % (name, i)] for i in range(side)] == rr, name
        assert [got["%s.col.%d" % (name, i)] for i in range(side)] == cr, name
        assert got["%s.data.0" % name] == dr, name
