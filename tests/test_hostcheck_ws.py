"""The workspace's bookkeeping (myzkp_amd/csrc/mzk_ws.h: leased scratch slots, the refusal of a held slot, growth, the trim after a
refused allocation, the budget, the cache generation) run on the host by tests/hostcheck/ws_shim.cpp, a stand-alone program built with
-fsanitize=address,undefined whose device hooks are malloc, free and a counter.  The program asserts the rules one by one and prints
"ok <letter>" for each; a block freed under a live lease or left behind at exit is the sanitizer's report.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = {
    "a": "a second get of a held slot fails naming both parties, from the same frame and from a nested one; the first block stays",
    "b": "after the inner frame ends the slot is taken again: same pointer if not larger, else one synchronize, one free, a new one",
    "c": "a refused allocation trims earlier calls' free slots only, never a held or a current one; retry, else MZK_E_NOMEM",
    "d": "the total held stays at or below the budget after a trim when idle slots suffice",
    "e": "freeing a cache slot bumps the generation, freeing scratch slots alone does not",
    "f": "the same slot on two contexts does not collide",
    "g": "a frame that took nothing, and one destroyed after an early error return, leave no holder behind",
    "h": "everything is given back at shutdown: no leak at exit",
}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("ws")
    exe = str(d / "ws_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "ws_shim.cpp")])
    return subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))


def test_the_program_ends_clean_under_the_sanitizers(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert "FAIL" not in run.stdout
    assert run.stdout.splitlines()[-1] == "ok all"


@pytest.mark.parametrize("rule", sorted(RULES))
def test_rule(run, rule):
    assert "ok " + rule in run.stdout.splitlines(), RULES[rule] + "\n" + run.stdout[-2000:] + run.stderr[-2000:]
