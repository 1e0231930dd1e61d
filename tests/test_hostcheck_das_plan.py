"""myzkp_amd/csrc/mzk_das_plan.h (the item form of every tree of Celestia's commitment, the trees a workgroup takes, grids, LDS bytes,
the node storage of a handle, the admitted views) run on the host by tests/hostcheck/das_plan_shim.cpp, a stand-alone program with
its own main: built once plain and once with -fsanitize=address,undefined, both outputs equal.  Checked here against tests/das_model.py
and in integers for EVERY admitted (rows, cols) and squares in 1, 2, 3, 64, 65, 2^20.  CPU only."""
import os, subprocess
import pytest
import das_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
SQUARES = (1, 2, 3, 64, 65, 1 << 20)
MAX_GRID, MAX_LDS = 1 << 20, 64 * 1024          # the limits mzk_rs_plan.h keeps: workgroups of a launch, LDS without an opt-in
WG_ITEMS, TREE_BLOCK, ROOT_BLOCK, NODE = 512, 256, 512, 32


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    d = tmp_path_factory.mktemp("das_plan_shim")
    src = os.path.join(HERE, "hostcheck", "das_plan_shim.cpp")
    common = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    plain, san = str(d / "das_plan_shim"), str(d / "das_plan_shim_san")
    subprocess.check_call(common + ["-O2", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    outs = []
    for exe in (plain, san):
        r = subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        outs.append(r.stdout)
    assert outs[0] == outs[1], "the sanitized build computes something else"
    out = {"T": {}, "L": {}, "S": [], "K": {}, "R": []}
    key = None
    for ln in outs[0].splitlines():
        f = ln.split()
        if f[0] == "T":
            out["T"][int(f[1])] = (int(f[2]), int(f[3]), [int(c) for c in f[4]])
        elif f[0] == "L":
            out["L"][int(f[1])] = [int(c) for c in f[2]]
        elif f[0] == "S":
            out["S"].append(tuple(map(int, f[1:])))
        elif f[0] == "K":
            key = (int(f[1]), int(f[2]))
            out["K"][key] = (tuple(map(int, f[3:])), {})
        elif f[0] == "B":
            out["K"][key][1][int(f[1])] = tuple(map(int, f[2:]))
        elif f[0] == "R":
            out["R"].append((tuple(map(int, f[1:6])), int(f[6]), ln.split(None, 7)[7]))
        else:
            assert f[0] == "ok" and int(f[1]) == 254 * 254
    return out


def test_item_form_equals_the_model_for_every_leaf_count(shim):
    assert sorted(shim["T"]) == list(range(2, 511))
    for n, (depth, items, sizes) in shim["T"].items():
        assert depth == n.bit_length() - 1 and items == 1 << depth, n
        assert sizes == M.item_sizes(n), n


def test_path_depths_equal_the_model_for_every_leaf(shim):
    assert sorted(shim["L"]) == list(range(2, 256))
    for n, depths in shim["L"].items():
        leafs = [bytes([i]) for i in range(n)]
        want = [len(p) if p is not None else 0 for p in (M.open_(i, leafs) for i in range(n))]
        assert depths == want, n
        assert max(depths) <= 8


def test_every_item_of_every_tree_is_one_slot_of_one_workgroup(shim):
    assert len(shim["S"]) == 2 * 254 * 5
    assert all(bad == 0 for _, _, _, bad in shim["S"]), [s for s in shim["S"] if s[3]][:5]


def test_every_admitted_shape_has_a_plan_that_covers_it(shim):
    assert len(shim["K"]) == 254 * 254
    for (rows, cols), (k, launches) in shim["K"].items():
        row_items, row_depth, col_items, col_depth, root_items, root_depth, row_g, col_g = k
        where = (rows, cols, k)
        assert (row_depth, row_items) == shim["T"][cols][:2] and (col_depth, col_items) == shim["T"][rows][:2], where
        assert (root_depth, root_items) == shim["T"][rows + cols][:2] and root_items <= ROOT_BLOCK // 2, where
        assert row_g * row_items == WG_ITEMS == col_g * col_items and WG_ITEMS == 2 * TREE_BLOCK, where
        assert sorted(launches) == sorted(SQUARES), where
        for q, b in launches.items():
            row_wgs, col_wgs, tg, tb, ti, tl, rg, rb, ri, rl, row_nb, col_nb, root_b, sym_b, handle_b, exported = b
            where = (rows, cols, q, b)
            row_trees, col_trees = q * rows, q * cols
            # workgroup w of a side takes trees w * G .. w * G + G - 1: every tree has exactly one, none is idle
            assert (row_wgs - 1) * row_g < row_trees <= row_wgs * row_g, where
            assert (col_wgs - 1) * col_g < col_trees <= col_wgs * col_g, where
            for grid, block, iters, lds, work, want_block in ((tg, tb, ti, tl, row_wgs + col_wgs, TREE_BLOCK), (rg, rb, ri, rl, q, ROOT_BLOCK)):
                assert block == want_block and 1 <= grid <= MAX_GRID and iters >= 1, where
                assert grid * iters >= work and (grid * (iters - 1) < work), where
                assert grid == work or grid == MAX_GRID, where
                assert grid * block < 1 << 32 and 0 < lds <= MAX_LDS, where
            assert tl == 2 * WG_ITEMS * NODE and rl == 2 * 256 * NODE, where
            # node storage = the sum of the levels below the roots; a handle keeps them, the roots and the symbols
            assert row_nb == NODE * row_trees * sum(row_items >> l for l in range(row_depth)), where
            assert col_nb == NODE * col_trees * sum(col_items >> l for l in range(col_depth)), where
            assert root_b == NODE * (row_trees + col_trees + q) and sym_b == q * rows * cols, where
            assert handle_b == row_nb + col_nb + root_b + sym_b == exported, where


def test_every_refusal_and_its_text(shim):
    got = {k: (err, msg) for k, err, msg in shim["R"]}
    side = "das: %s = %d is outside 2 .. 255 (the codes' own bound; a one-leaf tree commits to the leaf itself)"
    sq = "das: squares = %d is outside 1 .. 2^31 / (rows + cols) = %d"
    big = 1 << 31
    assert got == {
        (0, 8, 8, 0, 1): (-1, side % ("rows", 0)), (1, 8, 8, 8, 1): (-1, side % ("rows", 1)), (256, 8, 8, 2048, 1): (-1, side % ("rows", 256)),
        (8, 0, 0, 0, 1): (-1, side % ("cols", 0)), (8, 1, 1, 8, 1): (-1, side % ("cols", 1)), (8, 256, 256, 2048, 1): (-1, side % ("cols", 256)),
        (8, 8, 7, 64, 1): (-1, "das: row_stride = 7 is below cols = 8"),
        (8, 8, 8, 63, 2): (-1, "das: square_stride = 63 is below (rows - 1) * row_stride + cols = 64: the squares overlap"),
        (8, 8, 11, 84, 2): (-1, "das: square_stride = 84 is below (rows - 1) * row_stride + cols = 85: the squares overlap"),
        (8, 8, 8, 64, 0): (-1, sq % (0, big // 16)),
        (8, 8, 8, 64, big // 16 + 1): (-1, sq % (big // 16 + 1, big // 16)),
        (255, 255, 255, 65025, big // 510 + 1): (-1, sq % (big // 510 + 1, big // 510)),
        (2, 2, 2, 4, big): (-1, sq % (big, big // 4)),
    }


def test_the_library_reports_the_same_plan_without_a_gpu():
    import myzkp_amd.build as b
    b.build()
    import myzkp_amd as mz
    p = mz.das_plan(255, 254, 3)
    assert (p["rows"], p["cols"], p["squares"], p["path_max"]) == (255, 254, 3, 8) == (255, 254, 3, mz.DAS_PATH_MAX)
    assert (p["row_items"], p["row_depth"], p["col_items"], p["col_depth"], p["root_items"], p["root_depth"]) == (128, 7, 128, 7, 256, 8)
    assert p["tree_grid"] == p["row_wgs"] + p["col_wgs"] == -(-3 * 255 // 4) + -(-3 * 254 // 4) and p["root_grid"] == 3
    for bad, name in (((1, 5, 1), "rows"), ((5, 256, 1), "cols"), ((5, 5, 0), "squares"), ((2, 2, (1 << 29) + 1), "squares")):
        with pytest.raises(mz.MzkError) as e:
            mz.das_plan(*bad)
        assert e.value.code == -1 and name in e.value.message
