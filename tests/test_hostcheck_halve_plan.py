"""The halving steps of the bucket reduction (myzkp_amd/csrc/mzk_msm_plan.h: halve_multi_wg / _ops / _pair / _live, the index logic
k_halve_multi_row runs, and halve_plan, the launch list launch_halving_steps takes) run by tests/hostcheck/halve_plan_shim.cpp, a
stand-alone program built with -fsanitize=address,undefined, over arrays of exactly 2^lgB records.  For lgB = 4 .. 20: every launch of
up to eight steps with at most 1024 workgroups -- each step's (lo, hi) pairs are the single-step rule's (halve_indices), each once; no
addition reads what another addition of its step writes, and no two workgroups share a record; the records written back are exactly
those later steps and the tail read -- and every split of the last (up to eight) steps into launches of at most four, run on values
against the single-step rule.  Then the launch lists of the shipped layouts.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
WIDE, QUAD, MULTI, ROW = 0, 1, 2, 3          # HALVE_STEP_WIDE, HALVE_STEP_QUAD, HALVE_MULTI_QUAD, HALVE_MULTI_ROW
CUS, TAIL_MAX = 256, 64                       # an MI355X; MZK_TAIL_MAX_OPS' default (mzk_msm.hip)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("halve_plan") / "halve_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "halve_plan_shim.cpp")])
    return exe


def launches(shim, c, n, row=1, cus=CUS):
    """(launch list, first step of the tail) of a commit of n pairs against c-bit tables (c = 0: an MSM over arbitrary points)"""
    out = subprocess.run([shim, "layout", str(c), str(n), str(cus)], capture_output=True, text=True, check=True).stdout.split()
    lay = dict(zip(out[0::2], (int(v) for v in out[1::2])))
    assert lay["err"] == 0 and lay["halve_row"] == 1          # the shipped switch
    rows = subprocess.run([shim, "list", str(lay["lgB"]), str(lay["sets"]), str(cus), str(TAIL_MAX), str(row)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert rows[-1].startswith("tail ")
    return [tuple(int(v) for v in r.split()) for r in rows[:-1]], int(rows[-1].split()[1])


def test_every_launch_and_every_split_agrees_with_the_single_step_rule(shim):
    r = subprocess.run([shim], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 800 and int(words[2]) >= 3500, r.stdout


def test_the_flagship_commit_runs_steps_8_to_15_as_two_row_launches(shim):
    """17-bit tables, 2^16 buckets: the wide quad launch, then 144 and 13 workgroups of four row steps each, and the tail only sums"""
    assert launches(shim, 17, 1 << 20) == ([(MULTI, 0, 8, 256), (ROW, 8, 4, 144), (ROW, 12, 4, 13)], 16)
    assert launches(shim, 17, 1 << 20, row=0) == ([(MULTI, 0, 8, 256), (MULTI, 8, 8, 9)], 16)


def test_the_other_shipped_layouts(shim):
    # 16-bit tables: seven steps are left, four and three
    assert launches(shim, 16, 1 << 20) == ([(MULTI, 0, 8, 128), (ROW, 8, 4, 72), (ROW, 12, 3, 13)], 15)
    assert launches(shim, 16, 1 << 20, row=0) == ([(MULTI, 0, 8, 128), (MULTI, 8, 7, 9)], 15)
    # 20-bit tables: five wide steps, one quad step, eight steps in one quad launch, and the last five on rows
    head = [(WIDE, 0, 1, 2048), (WIDE, 1, 1, 2048), (WIDE, 2, 1, 1536), (WIDE, 3, 1, 1024), (WIDE, 4, 1, 640), (QUAD, 5, 1, 1536), (MULTI, 6, 8, 224)]
    assert launches(shim, 20, 1 << 20) == (head + [(ROW, 14, 4, 30), (ROW, 18, 1, 19)], 19)
    assert launches(shim, 20, 1 << 20, row=0) == (head + [(MULTI, 14, 5, 15)], 19)
    # arbitrary points at 2^20: eight sets of 2^15 buckets; the one quad launch ends where the tail takes over, so nothing changes
    generic = [(WIDE, 0, 1, 128), (WIDE, 1, 1, 128), (WIDE, 2, 1, 96), (WIDE, 3, 1, 64), (QUAD, 4, 1, 160), (MULTI, 5, 8, 24)]
    assert launches(shim, 0, 1 << 20) == (generic, 13) == launches(shim, 0, 1 << 20, row=0)


def test_a_first_quad_launch_is_never_replaced(shim):
    """narrow tables, whose every step fits one quad launch, keep it: the row form follows a k_halve_multi launch, it opens no list"""
    for c in (8, 9):
        got = launches(shim, c, 1 << 13)
        assert got == launches(shim, c, 1 << 13, row=0) and all(k != ROW for k, *_ in got[0]), (c, got)
