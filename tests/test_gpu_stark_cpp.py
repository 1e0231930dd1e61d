"""Builds and runs tests/cpp/test_stark_mirror.cpp: boundary_quotients, fast_stark_dims and FastStark (preprocess, prove) of the C++
mirror (myzkp_amd/host/myzkp.hpp) on known answers, on the boundary quotients of a real FastStark proof of the model
(tests/stark_model.py), true and false output, and on one whole proof, piece by piece against the model's."""
import json, os, random, subprocess
import pytest
import orc
import mpoly_model as mm
import stark_model as sm

ROOT = orc.ROOT
NAME = "test_stark_mirror"
EXE = os.path.join(ROOT, "tests", "cpp", NAME)
P = mm.M128_P


def build_exe():
    src = os.path.join(ROOT, "tests", "cpp", NAME + ".cpp")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", src, "-o", EXE, "-L" + os.path.join(ROOT, "myzkp_amd"), "-lmzk_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "myzkp_amd"), "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib"])


def test_stark_mirror_compiles():
    """CPU: the mirror's FastStark templates, instantiated over both fields, compile and link against the ABI."""
    import myzkp_amd.build as b
    b.build()
    build_exe()
    assert os.path.exists(EXE)


def _cases():
    """(field, [(polynomial, roots)], expected quotients): the boundary stage of two model proofs, and random rows over Fr"""
    with open(os.path.join(ROOT, "tests", "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    st = sm.FastStark(P, mm.M128_GEN, mm.m128_root(9), mm.m128_root(7), 4, 2, rp.m, rp.n + 1, 2)
    air = rp.transition_constraints(st.omicron)
    rnd = random.Random(12)
    tr = rp.trace(123456789)
    cases = []
    for claimed in (tr[-1][0], (tr[-1][0] + 1) % P):
        boundary = [(0, 1, 0), (rp.n, 0, claimed)]
        pr = st.prove([list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(st.nr)], boundary, air,
                      [rnd.randrange(P) for _ in range(128)])
        dbg = pr["_debug"]
        cases.append((orc.M128, list(zip(dbg["trace_polynomials"], dbg["boundary_roots"])), dbg["boundary_quotients"]))
    p = mm.FR_P
    rows = [([rnd.randrange(p) for _ in range(n)] + [1], [rnd.randrange(p) for _ in range(k)]) for n, k in ((40, 3), (9000, 2), (5, 9), (17, 0))]
    cases.append((orc.FR, rows, [sm.pdivmod(f, sm.from_monomials(r, p), p)[0] for f, r in rows]))
    return cases


_PROOF = {}


def _proof_line():
    """a FastStark<M128>::prove case at the reference's parameters, and the model's proof of it"""
    with open(os.path.join(ROOT, "tests", "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    st = sm.FastStark(P, mm.M128_GEN, mm.m128_root(9), mm.m128_root(7), 4, 2, rp.m, rp.n + 1, 2)
    air = rp.transition_constraints(st.omicron)
    rnd = random.Random(31)
    tr = rp.trace(42)
    boundary = [(0, 1, 0), (rp.n, 0, tr[-1][0])]
    trace = [list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(st.nr)]
    randomizer = [rnd.randrange(P) for _ in range(128)]
    _PROOF["want"] = st.prove(trace, boundary, air, randomizer)
    tok = [str(100 + orc.M128), "4", "2", str(rp.m), str(rp.n + 1), "2", str(mm.M128_GEN), str(len(air))]
    for a in air:
        tok.append(str(len(a)))
        for k, c in a.items():
            tok += [str(c)] + [str(e) for e in k]
    tok.append(str(len(trace)))
    tok += [str(v) for row in trace for v in row]
    tok.append(str(len(boundary)))
    for c, r, v in boundary:
        tok += [str(c), str(r), str(v)]
    tok.append(str(len(randomizer)))
    tok += [str(v) for v in randomizer]
    return " ".join(tok)


@pytest.mark.gpu
def test_stark_mirror_matches_the_model(tmp_path):
    cases = _cases()
    lines = []
    for fid, rows, _ in cases:
        tok = [str(fid), str(len(rows))]
        for f, r in rows:
            tok += [str(len(f))] + [str(v) for v in f] + [str(len(r))] + [str(v) for v in r]
        lines.append(" ".join(tok))
    lines.append(_proof_line())
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    build_exe()
    out = subprocess.run([EXE, str(path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stark mirror tests passed" in out.stdout
    got, lens = {}, {}
    for line in out.stdout.splitlines():
        f = line.split()
        if f and f[0] == "quotient.len":
            lens[(int(f[1]), int(f[2]))] = int(f[3])
        elif f and f[0] == "quotient":
            got.setdefault((int(f[1]), int(f[2])), {})[int(f[3])] = sum(int(x, 16) << (64 * k) for k, x in enumerate(f[4:]))
    # a whole proof through FastStark<F>::prove: every printed piece against the model's proof
    w = _PROOF["want"]
    idx = len(cases)
    lines_of = lambda key: [l.split()[2:] for l in out.stdout.splitlines() if l.split() and l.split()[0] == key and int(l.split()[1]) == idx]
    assert [l[0] for l in lines_of("bqcroot")] == [r.hex() for r in w["bqc_roots"]] and lines_of("rdcroot")[0][0] == w["rdc_root"].hex()
    assert lines_of("tzroot")[0][0] == w["_debug"]["transition_zerofier_root"].hex()
    assert [int(x) for x in lines_of("indices")[0]] == w["_debug"]["indices"]
    val = lambda l: sum(int(x, 16) << (64 * k) for k, x in enumerate(l[1:]))
    for key, name in (("bqcpoint", "bqc_points"), ("rdcpoint", "rdc_points"), ("tzcpoint", "tzc_points")):
        assert [val(l) for l in lines_of(key)] == w[name], key
    for key, name in (("bqcpath", "bqc_paths"), ("rdcpath", "rdc_paths"), ("tzcpath", "tzc_paths")):
        assert [[bytes.fromhex(h) for h in l[1:]] for l in lines_of(key)] == w[name], key
    for index, (_, rows, want) in enumerate(cases):
        for s, w in enumerate(want):
            assert lens[(index, s)] == len(w), (index, s)
            assert [got.get((index, s), {})[i] for i in range(len(w))] == w, (index, s)
