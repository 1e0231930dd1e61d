"""Builds and runs tests/cpp/test_mpoly_mirror.cpp: MPolynomial::evaluate_symbolic and the weighted combination of the C++ mirror
(myzkp_amd/host/myzkp.hpp) on the reference's known answers and on every case of tests/golden/mpoly_vectors.json."""
import json, os, subprocess
import pytest
import orc

ROOT = orc.ROOT
NAME = "test_mpoly_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_mpoly_mirror_compiles():
    """CPU: the mirror's MPolynomial and weighted_combination templates, instantiated over both fields, compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


def _cases():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "mpoly_vectors.json")))
    cases = []
    for c in d["compose"]:
        cases.append({"field": c["field"], "point": c["point"], "constraints": c["constraints"], "polys": [], "want": ("compose", c["expected"])})
    for c in d["lincomb"]:
        cases.append({"field": c["field"], "point": [], "constraints": [], "polys": list(zip(c["weights"], c["shifts"], c["polys"])),
                      "want": ("lincomb", [c["expected"]])})
    return cases


@pytest.mark.gpu
def test_mpoly_mirror_matches_golden(tmp_path):
    cases = _cases()
    lines = []
    for c in cases:
        tok = [str(c["field"]), str(len(c["point"]))]
        for q in c["point"]:
            tok += [str(len(q))] + list(q)
        tok.append(str(len(c["constraints"])))
        for terms in c["constraints"]:
            tok.append(str(len(terms)))
            for coef, k in terms:
                tok += [coef] + [str(e) for e in k]
        tok.append(str(len(c["polys"])))
        for w, s, q in c["polys"]:
            tok += [w, str(s), str(len(q))] + list(q)
        lines.append(" ".join(tok))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    build_exe()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "mpoly mirror tests passed" in out.stdout
    got, lens = {}, {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f and f[0] in ("compose.len", "lincomb.len"):
            lens[(f[0][:-4], int(f[1]), int(f[2]))] = int(f[3])
        elif f and f[0] in ("compose", "lincomb"):
            got.setdefault((f[0], int(f[1]), int(f[2])), {})[int(f[3])] = sum(int(x, 16) << (64 * k) for k, x in enumerate(f[4:]))
    checked = 0
    for index, c in enumerate(cases):
        kind, want = c["want"]
        if kind == "compose" and any(len({tuple(k) for _, k in terms}) != len(terms) for terms in c["constraints"]):
            continue                                        # duplicate exponent rows: not expressible as a dictionary
        for a, w in enumerate(want):
            key = (kind, index, a)
            assert lens[key] == len(w), key
            assert [got.get(key, {})[i] for i in range(len(w))] == [int(v) for v in w], key
            checked += 1
    assert checked >= len(cases) - 2
