"""myzkp_amd/csrc/mzk_rescue_plan.h (the program every S-box exponent becomes, the grid of a batch, the constants of a handle) and
myzkp_amd/csrc/mzk_rescue.h (one hash chain as the work of one lane, here with the portable products) run on the host by
tests/hostcheck/rescue_shim.cpp, a stand-alone program with its own main: built once plain and once with
-fsanitize=address,undefined, both with the products' limb-bound assertions on, both outputs equal.
(a) every program, run on integers, raises to exactly its exponent, reads at most four slots, costs what a Python restatement of the
planner says and never more than the binary method; 163 products for the reference's exponent; every refusal with its text; the grid.
(b) hashes and full traces of every case of tests/rescue_cases.py equal the model, both fields.  CPU only."""
import os, random, subprocess
import pytest
import rescue_cases as rc

HERE = os.path.dirname(os.path.abspath(__file__))
CAP, BLOCK = 8192, 64
REF_ALPHAINV = 0x87aaaaaaaaaaaaaaaaaaaaaaaaaaaaab
BATCHES = (0, 1, 63, 64, 65, CAP * 64 - 1, CAP * 64, CAP * 64 + 1, 1 << 32)


def exponents():
    out = [0, 1, 2, 3, 5, 7, REF_ALPHAINV]
    for k in (1, 2, 3, 4, 127, 128, 253, 254):
        out += [1 << k, (1 << k) - 1]
    out += [rc.M128_P - 2, rc.FR_P - 2]
    out += [rc.inv_exp(a, "m128") for a in (3, 5, 7, 9, 13)] + [rc.inv_exp(a, "fr") for a in (5, 7)]
    out += [0b1000111, 0b10001110000001]                 # a lone 111 behind zeros: the table of width 3 costs more than it saves
    rng = random.Random(20260)
    out += [rng.getrandbits(128) | 1 << 127 for _ in range(100)] + [rng.getrandbits(254) | 1 << 253 for _ in range(100)]
    return out


# ---- the planner once more, in Python ----------------------------------------------------------------------------------------------------
def plan_width(e, w):
    """(products, squarings, multiplies, table, slots, steps) of the left-to-right sliding window of width w"""
    if e == 0:
        return (0, 0, 0, 0, 0, [(0, 0)])
    bits = bin(e)[2:]
    i, sq, first, maxu, squarings, mults, steps = 0, 0, True, 1, 0, 0, []
    while i < len(bits):
        if bits[i] == "0":
            sq += 1
            i += 1
            continue
        ln = min(w, len(bits) - i)
        while bits[i + ln - 1] == "0":
            ln -= 1
        u = int(bits[i:i + ln], 2)
        if first:
            steps.append((2, (u - 1) // 2))
            first = False
        else:
            sq += ln
            steps += [(3, sq), (4, (u - 1) // 2)]
            squarings += sq
            mults += 1
        sq = 0
        maxu = max(maxu, u)
        i += ln
    if sq:
        steps.append((3, sq))
        squarings += sq
    k = (maxu - 1) // 2
    table = k + 1 if k else 0
    if k:
        steps.insert(0, (1, k))
    return (squarings + mults + table, squarings, mults, table, k + 1, steps)


def plan(e):
    best, width = plan_width(e, 1), 1 if e else 0
    binary = best[0]
    for w in (2, 3):
        c = plan_width(e, w)
        if c[0] < best[0]:
            best, width = c, w
    return best, width, binary


def run_program(steps):
    """the exponent a program raises to, and the slots it reads"""
    acc, built, used = None, 0, {0}
    for op, arg in steps:
        if op == 0:
            acc = 0
        elif op == 1:
            built = arg
        elif op == 2:
            assert arg <= built
            acc = 2 * arg + 1
            used.add(arg)
        elif op == 3:
            acc <<= arg
        elif op == 4:
            assert arg <= built
            acc += 2 * arg + 1
            used.add(arg)
        else:
            raise AssertionError(op)
    return acc, used, built


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescue_shim")
    src = os.path.join(HERE, "hostcheck", "rescue_shim.cpp")
    inp = str(d / "input.txt")
    exps = exponents()
    with open(inp, "w") as f:
        f.write("%d\n%s\n" % (len(exps), "\n".join("%x" % e for e in exps)))
        f.write("%d\n%s\n" % (len(BATCHES), "\n".join(str(b) for b in BATCHES)))
        f.write(rc.dump(rc.CASES))
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-misleading-indentation", "-DMZK_CHECK_BOUNDS"]
    plain, san = str(d / "rescue_shim"), str(d / "rescue_shim_san")
    subprocess.check_call(common + ["-O2", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    outs = []
    for exe in (plain, san):
        r = subprocess.run([exe, inp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the sanitized build computes something else"
    out = {"X": {}, "G": {}, "R": [], "P": None, "H": {}, "O": {}, "T": {}, "exps": exps}
    lines = outs[0].splitlines()
    assert lines[-1] == "ok"
    for ln in lines[:-1]:
        f = ln.split()
        if f[0] == "X":
            out["X"][int(f[1], 16)] = (tuple(map(int, f[2:10])), int(f[10], 16), [tuple(map(int, s.split(":"))) for s in f[11:]])
        elif f[0] == "G":
            out["G"][int(f[1])] = tuple(map(int, f[2:]))
        elif f[0] == "R":
            out["R"].append((tuple(map(int, f[1:5])), int(f[5]), ln.split(None, 6)[6]))
        elif f[0] == "P":
            out["P"] = list(map(int, f[1:]))
        elif f[0] in "HO":
            out[f[0]][(f[1], int(f[2]), int(f[3]))] = int(f[4], 16)
        else:
            assert f[0] == "T", ln
            out["T"][(f[1], int(f[2]), int(f[3]), int(f[4]))] = [int(v, 16) for v in f[5:]]
    return out


def test_every_program_raises_to_exactly_its_exponent(shim):
    assert set(shim["X"]) == set(shim["exps"]) and len(shim["exps"]) >= 6 + 16 + 2 + 7 + 200
    for e, (k, reached, steps) in shim["X"].items():
        window, slots, nsteps, squarings, mults, table, products, binary = k
        assert reached == e, hex(e)                                  # the shim's own integer run
        got, used, built = run_program(steps)                        # and one in Python, from the steps it printed
        assert got == e and len(steps) == nsteps <= 520, hex(e)
        assert max(used) == built and built + 1 == max(slots, 1) <= 4, hex(e)      # the table ends at the largest slot read
        assert all(pow(x, e, p) == eval_program(steps, x, p) for p in (rc.M128_P, rc.FR_P) for x in (0, 1, 2, p - 1, 0x123456789abcdef)), hex(e)


def eval_program(steps, x, p):
    """the program on field elements, as the lane runs it"""
    acc, slot = None, {0: x}
    for op, arg in steps:
        if op == 0:
            acc = 1
        elif op == 1:
            x2 = x * x % p
            for j in range(1, arg + 1):
                slot[j] = slot[j - 1] * x2 % p
        elif op == 2:
            acc = slot[arg]
        elif op == 3:
            for _ in range(arg):
                acc = acc * acc % p
        else:
            acc = acc * slot[arg] % p
    return acc


def test_product_counts_equal_the_python_planner_and_never_exceed_the_binary_method(shim):
    for e, (k, _, steps) in shim["X"].items():
        window, slots, nsteps, squarings, mults, table, products, binary = k
        (w_products, w_sq, w_mul, w_table, w_slots, w_steps), w_width, w_binary = plan(e)
        assert (products, squarings, mults, table, slots, window, binary) == (w_products, w_sq, w_mul, w_table, w_slots, w_width, w_binary), hex(e)
        assert steps == w_steps, hex(e)
        assert products == squarings + mults + table <= binary, hex(e)
        assert binary == (max(e.bit_length() - 1, 0) + max(bin(e).count("1") - 1, 0)), hex(e)
    k = shim["X"][REF_ALPHAINV][0]
    assert k == (3, 4, k[2], 127, 32, 4, 163, 191)
    assert shim["X"][0][2] == [(0, 0)] and shim["X"][1][2] == [(2, 0)] and shim["X"][2][2] == [(2, 0), (3, 1)]
    assert shim["X"][0b1000111][0][6] == 9                           # the binary method: a table for one 111 would make it 11


def test_grid_and_rounds(shim):
    assert sorted(shim["G"]) == sorted(BATCHES)
    for batch, (wgs, grid, iters, block, cap) in shim["G"].items():
        assert (block, cap) == (BLOCK, CAP)
        assert wgs == -(-batch // BLOCK) and grid == min(wgs, CAP)
        if batch == 0:
            assert (grid, iters) == (0, 0)
            continue
        assert grid * iters >= wgs > grid * (iters - 1) and grid * block < 1 << 32
    assert shim["G"][CAP * 64][1:3] == (CAP, 1) and shim["G"][CAP * 64 + 1][1:3] == (CAP, 2) and shim["G"][1 << 32][1:3] == (CAP, (1 << 26) // CAP)


def test_every_refusal_and_its_text(shim):
    got = {k: (err, msg) for k, err, msg in shim["R"]}
    fld = "rescue: field id %d is neither MZK_FIELD_M128 nor MZK_FIELD_FR"
    assert got == {
        (2, 2, 27, 1): (-1, fld % 2), (3, 2, 27, 1): (-1, fld % 3), (4, 2, 27, 1): (-1, fld % 4), (99, 2, 27, 1): (-1, fld % 99),
        (1, 0, 27, 1): (-1, "rescue: m = 0 is outside 1 .. 4"), (1, 5, 27, 1): (-1, "rescue: m = 5 is outside 1 .. 4"),
        (0, 2, 0, 1): (-1, "rescue: n_rounds = 0 is outside 1 .. 64"), (0, 2, 65, 1): (-1, "rescue: n_rounds = 65 is outside 1 .. 64"),
        (1, 4, 64, (1 << 40) + 1): (-5, "rescue: batch = %d is beyond 2^40" % ((1 << 40) + 1)),
    }


def test_exported_plan_of_the_reference_parameters(shim):
    P = shim["P"]
    words = []
    for e in (3, REF_ALPHAINV):
        (products, sq, mul, table, slots, steps), width, binary = plan(e)
        words.append([width, slots, len(steps), sq, mul, table, products, binary])
    assert words[0] == [1, 1, 3, 1, 1, 0, 2, 2] and words[1][0:2] + words[1][3:] == [3, 4, 127, 32, 4, 163, 191]
    const_words = ((words[0][2] + words[1][2] + 3) & ~3) + 5 * (4 + 108)
    assert P == [1, 2, 27, 4099] + words[0] + words[1] + [27 * (2 * 165 + 8) + 2, 28, 56, 64, 65, 65, 1, CAP, 4 * const_words]


def test_per_lane_code_equals_the_model_on_every_case(shim):
    hashes = traces = 0
    for c in rc.CASES:
        rows = c["n"] + 1
        for k, x in enumerate(c["inputs"]):
            for l, (t, o) in enumerate(rc.model_chain(c, x, c["links"])):
                where = (c["name"], k, l)
                assert shim["H"][where] == o == shim["O"][where], where
                assert [shim["T"][where + (r,)] for r in range(rows)] == t, where
                hashes += 1
                traces += rows
    assert hashes == len(shim["H"]) == len(shim["O"]) and traces == len(shim["T"])


def test_the_library_reports_the_same_plan_without_a_gpu(shim):
    import myzkp_amd.build as b
    b.build()
    import myzkp_amd as mz
    p = mz.rescue_plan(mz.FIELD_M128, 2, 27, 3, REF_ALPHAINV, 4099)
    assert [p[k] for k in mz._lib.RESCUE_PLAN_FIELDS] == shim["P"]
    assert (p["alphainv_products"], p["alphainv_binary"], p["alphainv_slots"], p["grid_cap"]) == (163, 191, 4, CAP)
    assert (mz.RESCUE_MAX_M, mz.RESCUE_MAX_ROUNDS) == (4, 64)
    for bad, code, name in (((2, 2, 27, 3, 5, 1), -1, "field"), ((1, 0, 27, 3, 5, 1), -1, "m = 0"), ((1, 5, 27, 3, 5, 1), -1, "m = 5"), ((0, 2, 0, 3, 5, 1), -1, "n_rounds = 0"),
                            ((0, 2, 65, 3, 5, 1), -1, "n_rounds = 65"), ((1, 2, 2, 3, 5, (1 << 40) + 1), -5, "batch")):
        with pytest.raises(mz.MzkError) as e:
            mz.rescue_plan(*bad)
        assert e.value.code == code and name in e.value.message
    # a handle's constants are checked before any device work: these refusals need no GPU
    for mds, rcs, what in (([[rc.M128_P]], [0, 0], "mds[0]"), ([[1]], [0, rc.M128_P], "round_constants[1]")):
        with pytest.raises(mz.MzkError) as e:
            mz.RescuePrime(mz.FIELD_M128, 1, 1, 3, 5, mds, rcs)
        assert e.value.code == -6 and what in e.value.message
    with pytest.raises(mz.MzkError) as e:
        mz.RescuePrime(mz.FIELD_M128, 5, 1, 3, 5, [[1]], [0, 0])
    assert e.value.code == -1 and "m = 5" in e.value.message


def test_no_instantiation_of_the_kernel_spills_or_uses_scratch():
    """one kernel template over <field, m, with_trace>: 16 instantiations in the shipped library, read with tools/kernel_resources.py"""
    import sys
    import myzkp_amd.build as b
    so = b.build()
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import kernel_resources
    res = {k: v for k, v in kernel_resources.kernel_resources(so).items() if "k_rescue<" in k}
    assert len(res) == 16, sorted(res)
    for k, v in res.items():
        assert (v["vgpr_spill"], v["sgpr_spill"], v["scratch"]) == (0, 0, 0), (k, v)
