"""myzkp_amd/csrc/mzk_gf256.h (GF(2^8) products, inverses, the packed forms) and mzk_rs_plan.h (which kernel form encodes and decodes
a Reed-Solomon code, with how many lanes, registers, workgroups and LDS bytes, and the tables the kernels read) run on the host by
tests/hostcheck/rs_shim.cpp, a stand-alone program with its own main: built once plain and once with -fsanitize=address,undefined,
both outputs equal.  Checked here against tests/rs_model.py and in integers, for EVERY admitted (n, k) and the batches
1, 63, 64, 65, 2^20, 2^31.  CPU only."""
import os, subprocess
import pytest
import rs_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
BATCHES = (1, 63, 64, 65, 1 << 20, 1 << 31)
COPY, LANE, WAVE = 0, 1, 2
MAX_GRID, BLOCK, MAX_LDS = 1 << 20, 256, 160 * 1024


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("rs_shim")
    src = os.path.join(HERE, "hostcheck", "rs_shim.cpp")
    common = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    plain, san = str(d / "rs_shim"), str(d / "rs_shim_san")
    subprocess.check_call(common + ["-O2", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    outs = []
    for exe in (plain, san):
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the sanitized build computes something else"
    out = {"M": {}, "K": {}, "R": []}
    key = None
    for ln in outs[0].splitlines():
        f = ln.split()
        if f[0] == "M":
            out["M"][int(f[1])] = bytes.fromhex(f[2])
        elif f[0] == "I":
            out["I"] = bytes.fromhex(f[1])
        elif f[0] == "X":
            out["X"] = int(f[1])
        elif f[0] == "T":
            out["T"] = (bytes.fromhex(f[1]), bytes.fromhex(f[2]))
        elif f[0] == "K":
            key = (int(f[1]), int(f[2]))
            names = ("d", "t", "form", "lanes", "pw", "pad", "w", "spl", "ppl", "npad", "dpad")
            out["K"][key] = dict(zip(names, map(int, f[3:14])), gen=bytes.fromhex(f[14]), launches={})
        elif f[0] == "B":
            v = list(map(int, f[1:]))
            out["K"][key]["launches"][v[0]] = [dict(zip(("grid", "block", "per_block", "iters", "lds"), v[1 + 5 * i: 6 + 5 * i])) for i in range(3)]
        elif f[0] == "R":
            out["R"].append((int(f[1]), int(f[2]), int(f[3]), int(f[4]), ln.split(None, 5)[5] if len(f) > 5 else ""))
        else:
            assert f[0] == "ok" and int(f[1]) == 255 * 256 // 2
    return out


def test_all_products_and_inverses_equal_the_model(shim):
    for a in range(256):
        assert shim["M"][a] == bytes(M.gf_mul_bits(a, b) for b in range(256)), a
    assert shim["I"][0] == 0
    for a in range(1, 256):
        assert shim["I"][a] == M.gf_inv(a) and M.gf_mul_bits(a, shim["I"][a]) == 1, a


def test_packed_forms_equal_the_scalar_product(shim):
    assert shim["X"] == 0


def test_points_equal_the_model(shim):
    pts, inv = shim["T"]
    assert list(pts[:255]) == M.ReedSolomon(255, 1).evaluation_points(255)
    assert all(M.gf_mul(p, q) == 1 for p, q in zip(pts, inv))


def test_every_admitted_code_has_a_plan_that_covers_it(shim):
    gens = {d: bytes(M.ReedSolomon(d + 1, 1).generator_polynomial()) for d in range(255)}
    assert len(shim["K"]) == 255 * 256 // 2
    for n in range(1, 256):
        for k in range(1, n + 1):
            p = shim["K"][(n, k)]
            where = (n, k, p)
            d = n - k
            assert p["d"] == d and p["t"] == d // 2, where
            assert p["gen"] == gens[d], where                                   # the generator polynomial is the model's
            # encode: the form by d, lanes x parity words x 4 bytes cover d with the padding the kernels rely on
            assert p["form"] == (COPY if d == 0 else LANE if d <= 32 else WAVE), where
            if d == 0:
                assert p["pw"] == 0 and p["pad"] == 0, where
            else:
                assert (p["lanes"], p["pw"]) == ((1, 1 if d <= 4 else 2 if d <= 8 else 4 if d <= 16 else 8) if d <= 32 else (64, 1)), where
                assert 4 * p["lanes"] * p["pw"] == d + p["pad"] and 0 <= p["pad"], where
            # decode: a power-of-two group inside one wave; syndromes, coefficients and positions all owned by some lane
            w = p["w"]
            assert w in (8, 16, 32, 64) and (w >= d or w == 64) and (w == 8 or w // 2 < d), where
            assert p["spl"] * w >= d and p["ppl"] * w >= n and (p["ppl"] - 1) * w < n, where
            assert p["npad"] >= n and p["dpad"] >= d + 1 and p["npad"] % 4 == 0 and p["dpad"] % 4 == 0, where
            for batch in BATCHES:
                enc, syn, dec = p["launches"][batch]
                per = {COPY: BLOCK, LANE: BLOCK, WAVE: BLOCK // 64}[p["form"]]
                groups = BLOCK // w
                for L, per_block in ((enc, per), (syn, groups), (dec, groups)):
                    assert L["block"] == BLOCK and L["per_block"] == per_block, where
                    assert 1 <= L["grid"] <= MAX_GRID and L["iters"] >= 1, where
                    assert L["grid"] * L["iters"] * per_block >= batch, where                         # the grid covers the batch
                    assert (L["grid"] * L["iters"] - 1) * per_block < batch or L["grid"] == MAX_GRID, where      # without an idle workgroup
                    assert L["grid"] * L["block"] < 1 << 32, where
                assert enc["lds"] == 0 and syn["lds"] == 0, where
                assert dec["lds"] == groups * (2 * p["npad"] + 5 * p["dpad"]) <= MAX_LDS, where
                assert dec["lds"] <= 64 * 1024, where                                                # no opt-in for large dynamic LDS is needed


def test_every_refusal_and_its_text(shim):
    got = {(n, k, b): (err, msg) for n, k, b, err, msg in shim["R"]}
    nk = "rs: (n, k) = (%d, %d) is outside 1 <= k <= n <= 255 (the evaluation points 2^i repeat from n = 256 on)"
    bt = "rs: a batch of %d codewords is outside 1 .. 2^31"
    assert got == {
        (256, 8, 1): (-1, nk % (256, 8)), (256, 256, 1): (-1, nk % (256, 256)), (16, 0, 1): (-1, nk % (16, 0)), (0, 0, 1): (-1, nk % (0, 0)),
        (8, 9, 1): (-1, nk % (8, 9)), (1000, 1000, 5): (-1, nk % (1000, 1000)),
        (16, 8, 0): (-1, bt % 0), (16, 8, (1 << 31) + 1): (-1, bt % ((1 << 31) + 1)), (255, 1, 1 << 40): (-1, bt % (1 << 40)),
    }
