"""myzkp_amd/csrc/mzk_hypercube_plan.h run on the host by tests/hostcheck/hypercube_plan_shim.cpp, a stand-alone program with its own
main: built once plain and once with -fsanitize=address,undefined, both outputs equal.  For every el in 0..30, over random and
adversarial term tables (all-equal masks, all-distinct masks, only high bits, only low bits, empty factors between full ones, more
groups and more masks than the tile form's limits and exactly as many) and each of the three forms, every field of the plan equals
tests/hypercube_model.py: the distinct masks in order, the merged segments, the groups, the form that runs, grids, launch and byte counts, and the coefficients merged on the
host.  Every refusal with its code.  CPU only."""
import os, random, subprocess
import pytest
import hypercube_model as hm

HERE = os.path.dirname(os.path.abspath(__file__))
P = hm.P
E_ARG, E_LENGTH = -1, -5


def exps_with_mask(m, el, rng):
    return tuple(rng.choice((1, 1, 2, 7, 0xFFFFFFFF)) if (m >> (el - 1 - i)) & 1 else 0 for i in range(el))


def tables():
    """[(el, form, t0, factors)]: factors = lists of (coef, exps)"""
    out = []
    for el in range(31):
        rng = random.Random(4100 + el)
        n = 1 << el
        g = min(el, hm.TILE_LOG)
        low, high = n - 1 & ((1 << g) - 1), (n - 1) >> g << g
        term = lambda m: (rng.choice((0, 1, P - 1, rng.randrange(P))), exps_with_mask(m, el, rng))
        rand = lambda cnt, keep=n - 1: [term(rng.randrange(n) & keep) for _ in range(cnt)]
        one = rng.randrange(n)
        distinct = rng.sample(range(n), min(n, 70))
        sets = {"random": [rand(50), rand(3), rand(120)],
                "all_equal_masks": [[term(one) for _ in range(40)]],
                "all_distinct_masks": [[term(m) for m in distinct]],
                "only_high_bits": [rand(60, high), rand(5, high)],
                "only_low_bits": [rand(60, low)],
                "empty_between_full": [[], rand(30), [], [], rand(31), []],
                "no_factor": [],
                "nine_factors": [rand(2 + f) for f in range(9)]}
        if el >= 19:            # more groups than HC_TILE_MAX_GROUPS in one factor, and exactly the limit in another table
            his = rng.sample(range(n >> g), hm.TILE_MAX_GROUPS + 1)
            sets["groups_above_limit"] = [rand(4), [term(h << g | rng.randrange(1 << g)) for h in his]]
            sets["groups_at_limit"] = [[term(h << g | rng.randrange(1 << g)) for h in his[:-1]]]
        if el in (13, 20, 30):  # more distinct masks than HC_TILE_MAX_MASKS in one group, and exactly the limit
            lows = rng.sample(range(1 << 13), hm.TILE_MAX_MASKS + 1)
            at = lambda m: (m & 1023) | (m >> 10) << (el - 3)            # three high bits: eight groups at most
            sets["masks_above_limit"] = [[term(at(m)) for m in lows], rand(3)]
            sets["masks_at_limit"] = [[term(at(m)) for m in lows[:-1]]]
        for i, (name, factors) in enumerate(sets.items()):
            forms = (0, 1, 2) if name in ("random", "groups_above_limit", "masks_above_limit", "empty_between_full", "no_factor") else ((el + i) % 3,)
            for form in forms:
                out.append((name, el, form, 5 * (i % 2), factors))
    return out


def write_table(lines, el, k, form, offsets, rows):
    lines.append("%d %d %d %d %d" % (el, k, form, len(offsets), len(rows)))
    lines.append(" ".join(str(o) for o in offsets))
    for c, exps in rows:
        lines.append("%064x %s" % (c, " ".join(str(e) for e in exps)))


REFUSALS = [("form 3", 4, 1, 3, [0, 1], 1, E_ARG), ("form -1", 4, 1, -1, [0, 1], 1, E_ARG), ("31 variables", 31, 1, 0, [0, 0], 0, E_LENGTH),
            ("decreasing offsets", 4, 2, 0, [2, 3, 1], 3, E_LENGTH), ("2^28 terms", 4, 1, 1, [0, 1 << 28], 0, E_LENGTH),
            ("2^28 terms over two factors", 0, 2, 2, [7, 7 + (1 << 27), 7 + (1 << 28)], 0, E_LENGTH), ("null offsets", 4, 1, 0, [], 0, E_ARG),
            ("65536 factors", 2, 65536, 0, [0] * 65537, 0, E_LENGTH)]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("hypercube_plan_shim")
    src = os.path.join(HERE, "hostcheck", "hypercube_plan_shim.cpp")
    tabs = tables()
    lines = [str(len(tabs) + len(REFUSALS))]
    for name, el, form, t0, factors in tabs:
        offsets = [t0]
        for f in factors:
            offsets.append(offsets[-1] + len(f))
        rows = [(0, (0,) * el)] * t0 + [t for f in factors for t in f]
        write_table(lines, el, len(factors), form, offsets, rows)
    for what, el, k, form, offsets, n_rows, code in REFUSALS:
        write_table(lines, el, k, form, offsets, [(1, (1,) * el)] * n_rows)
    inp = str(d / "input.txt")
    open(inp, "w").write("\n".join(lines) + "\n")
    common = ["g++", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-misleading-indentation"]
    plain, san = str(d / "shim"), str(d / "shim_san")
    subprocess.check_call(common + ["-O2", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    outs = []
    for exe in (plain, san):
        r = subprocess.run([exe, inp], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    return tabs, outs[0].split("\n")


def test_every_plan_field_equals_the_model(shim):
    tabs, lines = shim
    at = 0
    seen_forms = set()
    for name, el, form, t0, factors in tabs:
        what = "%s el=%d form=%d" % (name, el, form)
        assert lines[at] == "T 0", (what, lines[at:at + 2])
        want = hm.plan([[e for _, e in f] for f in factors], el, form)
        E = sum(len(f["masks"]) for f in want["factors"])
        G = sum(len(f["groups"]) for f in want["factors"])
        scalars = [want["form"], want["g"], want["terms"], E, G, want["max_masks"], want["max_groups"], want["launches"], want["memsets"], want["grid_x"],
                   want["grid_y"], want["mle_passes"], want["upload_bytes"], want["workspace_bytes"], want["table_bytes"]]
        assert [int(x) for x in lines[at + 1].split()] == scalars, what
        at += 2
        coefs = [c for f in factors for c, _ in f]
        for f in want["factors"]:
            assert lines[at] == "F %d %d" % (len(f["masks"]), len(f["groups"])), what
            assert [int(x) for x in lines[at + 1].split()[1:]] == f["masks"], what
            at += 2
            for seg in f["segments"]:
                assert [int(x) for x in lines[at].split()[1:]] == seg, what
                at += 1
            assert [int(x) for x in lines[at].split()[1:]] == [x for grp in f["groups"] for x in grp], what
            assert [int(x, 16) for x in lines[at + 1].split()[1:]] == [sum(coefs[t] for t in seg) % P for seg in f["segments"]], what
            at += 2
        if form == 0:
            seen_forms.add((want["form"], el > hm.TILE_LOG))
            assert want["form"] == (hm.SCATTER if name in ("groups_above_limit", "masks_above_limit") else hm.TILE), what
    assert seen_forms == {(hm.TILE, False), (hm.TILE, True), (hm.SCATTER, True)}
    for what, el, k, form, offsets, n_rows, code in REFUSALS:
        assert lines[at] == "T %d" % code, (what, lines[at:at + 2])
        assert lines[at + 1].startswith("mpoly_hypercube: "), what
        at += 2
    assert lines[at:] == [""]
