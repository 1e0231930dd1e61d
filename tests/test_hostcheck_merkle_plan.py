"""The Merkle level schedule (merkle_plan in myzkp_amd/csrc/mzk_merkle_plan.h: which of the nine kernels hashes which levels, on the
thresholds LEAF_PAIR_MAX, LEVEL_PAIR_MAX and TAIL_NODES and the tree count of a batch) run on the host by
tests/hostcheck/merkle_plan_shim.cpp, a stand-alone program built with -fsanitize=address,undefined: every single tree of 2^1 .. 2^36
leaves and batches of 2^1 .. 2^16 leaves per tree, for all four leaf kinds.  Checked here in integers: the steps tile the levels, stay
inside their kernels' limits, and equal the schedule written out below.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
FIELD, FIELD_PLAIN, GL, BYTES = 0, 1, 2, 3
KINDS = (FIELD, FIELD_PLAIN, GL, BYTES)
K = ("lp", "plain", "gl", "bytes", "level", "pair", "m2", "m3", "tail")      # MerkleKernel
LEAF_OF = {FIELD_PLAIN: "plain", GL: "gl", BYTES: "bytes"}
HASHES_PER_BLOCK = {"lp": 64, "plain": 128, "gl": 128, "bytes": 128, "level": 128, "pair": 64, "m2": 128, "m3": 256, "tail": 256}
BLOCK = {"lp": 128, "plain": 128, "gl": 128, "bytes": 128, "level": 128, "pair": 128, "m2": 256, "m3": 512, "tail": 512}
LEVELS = {"lp": 1, "plain": 1, "gl": 1, "bytes": 1, "level": 1, "pair": 1, "m2": 2, "m3": 3}
TREES = (1, 2, 3, 5, 7, 33, 300, 511, 512, 513, 600, 1024)

SINGLE = [(1 << lg, 1) for lg in range(1, 37)]
BATCHES = [(per, t) for per in (1 << k for k in range(1, 17)) for t in TREES]
assert all(per * t <= 1 << 36 for per, t in BATCHES)      # the ABI's bound on a batch


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(n, trees, kind): [(kernel name, nodes_in, parents, levels, grid, block, out_offset), ...]}, thresholds"""
    d = tmp_path_factory.mktemp("merkle_plan")
    exe = str(d / "merkle_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "merkle_plan_shim.cpp")])
    shapes = sorted({(per * t, t, k) for per, t in SINGLE + BATCHES for k in KINDS})
    src = str(d / "shapes.txt")
    with open(src, "w") as f:
        f.write("".join("%d %d %d\n" % s for s in shapes))
    r = subprocess.run([exe, src], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(shapes)
    assert lines[-2].split()[0] == "T"
    thresholds = dict(zip(("LEAF_PAIR_MAX", "LEVEL_PAIR_MAX", "TAIL_NODES", "LEAF_THREADS"), map(int, lines[-2].split()[1:])))
    out = {}
    for ln in lines[:-2]:
        f = ln.split()
        assert f[0] == "P"
        n, trees, kind, ns = map(int, f[1:5])
        v = list(map(int, f[5:]))
        assert len(v) == 7 * ns
        out[(n, trees, kind)] = [(K[v[7 * i]],) + tuple(v[7 * i + 1:7 * i + 7]) for i in range(ns)]
    assert len(out) == len(shapes)
    return out, thresholds


def test_thresholds(plans):
    assert plans[1] == {"LEAF_PAIR_MAX": 1 << 15, "LEVEL_PAIR_MAX": 16384, "TAIL_NODES": 512, "LEAF_THREADS": 128}


def test_steps_tile_the_levels_and_stay_inside_their_kernels_limits(plans):
    plans, T = plans
    for (n, trees, kind), steps in plans.items():
        where = (n, trees, kind, steps)
        per = n // trees
        assert per * trees == n and per & (per - 1) == 0 and per >= 2
        # the leaf step
        name, nodes_in, parents, levels, grid, block, off = steps[0]
        want_leaf = LEAF_OF.get(kind) or ("lp" if n // 2 <= T["LEAF_PAIR_MAX"] else "plain")
        assert (name, nodes_in, parents, levels, off) == (want_leaf, n, n // 2, 1, 0), where
        count, at = n, 0            # nodes of the level the next step reads; digests written so far
        for i, (name, nodes_in, parents, levels, grid, block, off) in enumerate(steps):
            assert (i == 0) == (name in ("lp", "plain", "gl", "bytes")), where
            assert nodes_in == count and nodes_in % 2 == 0 and parents == nodes_in // 2, where      # reads exactly what the step before left
            assert off == at, where                                                                  # and writes right behind it
            assert 1 <= grid < 1 << 32 and block == BLOCK[name] and block <= 1024, where
            assert grid * HASHES_PER_BLOCK[name] >= parents > (grid - 1) * HASHES_PER_BLOCK[name], where      # covers the parents; no idle workgroup
            if name == "tail":
                assert i == len(steps) - 1 and i > 0 and nodes_in <= T["TAIL_NODES"] and grid == 1, where
                assert nodes_in >> levels == trees and (trees << levels) == nodes_in, where
            else:
                assert levels == LEVELS[name], where
            if name in ("pair", "m2", "m3"):
                assert parents <= T["LEVEL_PAIR_MAX"], where
            if name == "level":
                assert parents > T["LEVEL_PAIR_MAX"], where
            if name in ("m2", "m3"):            # every level inside the launch pairs nodes of ONE tree
                assert nodes_in % trees == 0 and (nodes_in // trees) % (1 << levels) == 0, where
                assert block == 64 << levels, where
            for j in range(levels):
                assert (parents >> j) << j == parents, where
                at += parents >> j
            count = parents >> (levels - 1)
            assert count >= trees, where
        assert count == trees and at == n - trees, where      # the last level is the roots; n - trees digests in all
        assert len(steps) <= 72


def _names(steps):
    return [s[0] for s in steps]


def test_single_tree_schedule_is_the_pinned_table(plans):
    plans, _ = plans
    want = {1: ["lp"]}
    for lg in range(2, 11):
        want[lg] = ["lp", "tail"]
    want[11] = ["lp", "pair", "tail"]
    want[12] = ["lp", "m2", "tail"]
    want[13] = ["lp", "m3", "tail"]
    want[14] = ["lp", "m3", "pair", "tail"]
    want[15] = ["lp", "m3", "m2", "tail"]
    want[16] = ["lp", "m3", "m3", "tail"]          # 2^15 pairs = LEAF_PAIR_MAX, 2^14 hashes = LEVEL_PAIR_MAX: both met with equality
    want[17] = ["plain", "level", "m3", "m3", "tail"]
    want[18] = ["plain", "level", "level", "m3", "m3", "tail"]
    want[19] = ["plain"] + ["level"] * 3 + ["m3", "m3", "tail"]
    want[20] = ["plain"] + ["level"] * 4 + ["m3", "m3", "tail"]
    want[21] = ["plain"] + ["level"] * 5 + ["m3", "m3", "tail"]
    for lg in range(1, 22):
        assert _names(plans[(1 << lg, 1, FIELD)]) == want[lg], lg
        for kind in (FIELD_PLAIN, GL, BYTES):      # the other leaf kinds: their one leaf kernel, the same levels above
            assert _names(plans[(1 << lg, 1, kind)]) == [LEAF_OF[kind]] + want[lg][1:], (lg, kind)
    # the tail's input: 2^(lg-1) nodes up to 2^10 leaves, TAIL_NODES from there on
    for lg in range(2, 22):
        assert plans[(1 << lg, 1, FIELD)][-1][1] == min(1 << (lg - 1), 512), lg
    for lg in range(22, 37):
        assert _names(plans[(1 << lg, 1, FIELD)]) == ["plain"] + ["level"] * (lg - 16) + ["m3", "m3", "tail"], lg


def test_batch_schedules_of_the_gpu_tests(plans):
    """the (leaves per tree, trees) pairs of tests/test_gpu_merkle_levels.py: every ending of a batch"""
    plans, _ = plans
    want = {
        (2048, 3): (["lp", "m2", "pair", "tail"], 384),
        (8192, 5): (["lp", "m3", "m2", "pair", "tail"], 320),
        (16, 512): (["lp", "m3"], None),                       # ends on the third level of multi<3>: no tail
        (16, 511): (["lp", "m2", "pair"], None),
        (32, 300): (["lp", "m3", "pair"], None),
        (32768, 3): (["plain", "level", "m3", "m2", "pair", "tail"], 384),
        (4, 600): (["lp", "pair"], None),                      # more trees than the tail holds nodes: roots from k_merkle_level_pair
        (16384, 7): (["plain", "level", "m3", "m2", "pair", "tail"], 448),
        (4096, 33): (["plain", "level", "level", "m3", "m2", "pair", "tail"], 264),
    }
    for (per, trees), (names, tail_in) in want.items():
        steps = plans[(per * trees, trees, FIELD)]
        assert _names(steps) == names, (per, trees, steps)
        if tail_in is not None:
            assert steps[-1][1] == tail_in, (per, trees)
