"""The workspace's bookkeeping (myzkp_amd/csrc/mzk_ws.h: leased scratch slots, the refusal of a held slot, growth, the trim after a
refused allocation, the budget, the cache generation, the pool of size classes, the plan caches' eviction) run on the host by tests/hostcheck/ws_shim.cpp, a stand-alone program built with
-fsanitize=address,undefined whose device hooks are malloc, free and two counters.  The program asserts the rules one by one and prints
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
    "i": "a pool request is rounded to a power of two, 4096 at least; a released block of that class is handed out again with no hook "
         "call; another class allocates",
    "j": "with the pool's cap lowered, a release that would pass it frees the block instead of parking it",
    "k": "a refused pool allocation releases the parked blocks and the idle slots and is retried; refused twice it is MZK_E_NOMEM, the "
         "message naming the request",
    "l": "ws_bytes_held counts parked and lent bytes; ws_trim_idle returns exactly what it freed and leaves lent blocks live",
    "m": "a block taken on context 0 and destroyed while context 1 is current returns to context 0's pool",
    "n": "lru_evict removes the entry with the oldest stamp once the cap is reached, frees its memory exactly once, and removes "
         "nothing below the cap",
    "o": "ws_release_all on both contexts leaves nothing live, parked blocks included",
}
CSRC = os.path.join(os.path.dirname(HERE), "myzkp_amd", "csrc")


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


def occurrences(call):
    hits = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                hits += [(name, no) for no, line in enumerate(f, 1) for _ in range(line.count(call))]
    return hits


@pytest.mark.parametrize("call", ["hipMalloc(", "hipFree("])
def test_device_memory_has_one_way_in_and_one_way_out(call):
    """every allocation passes ws_hook_alloc and every release ws_hook_free, both in mzk_api.hip, where mzk_ws.h meets the device"""
    hits = occurrences(call)
    assert [name for name, _ in hits] == ["mzk_api.hip"], hits


def test_only_the_owner_types_release_device_memory():
    """ws_hook_free is defined in mzk_api.hip and called by mzk_ws.h (the workspace, WsBlock, DevMem) alone: no handle frees by hand"""
    hits = occurrences("ws_hook_free(")
    assert {name for name, _ in hits} == {"mzk_api.hip", "mzk_ws.h"}, hits
    assert [name for name, _ in hits].count("mzk_api.hip") == 1, hits


def test_an_srs_handle_is_made_in_one_place():
    hits = occurrences("new mzk_srs")
    assert [name for name, _ in hits] == ["mzk_srs.h"], hits
