"""The SRS handle (myzkp_amd/csrc/mzk_srs.h: srs_new over the layout ladder of mzk_srs_plan.h, the owner, the direct and wide table
sets) run on the host by tests/hostcheck/srs_handle_main.cpp, a stand-alone program whose device hooks are malloc, free and a refusal
counter.  Built plain and with -fsanitize=address,undefined; it asserts the rules one by one and prints "ok <letter>" for each.  A
table set freed twice or left behind at exit is the sanitizer's report.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RULES = {
    "a": "srs_new lands on the full tables, two bucket sets, four, the prepared points as 0, 2, 4, 6 allocations are refused: each rung "
         "is tried, the idle workspace released, the rung tried again; a rung over the budget is not asked for",
    "b": "with the last rung refused too it is MZK_E_NOMEM in the words of the prepared points, and the handle is gone",
    "c": "an empty handle takes the first rung and no memory; a handle remembers the context it was made on",
    "d": "direct tables attached, replaced and dropped: one owner at a time, their bytes counted while held",
    "e": "wide tables through a const handle: reserved, attached when built, used from then on; a refusal by the device or the budget "
         "is remembered, leaves no message and is not tried again",
}
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def run(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("srs_handle") / ("srs_handle_" + request.param))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + (SANITIZE if request.param == "sanitized" else []) +
                          ["-o", exe, os.path.join(HERE, "hostcheck", "srs_handle_main.cpp")])
    return subprocess.run([exe], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))


def test_the_program_ends_clean(run):
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-4000:]
    assert "AddressSanitizer" not in run.stderr and "LeakSanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
    assert "FAIL" not in run.stdout
    assert run.stdout.splitlines()[-1] == "ok all"


@pytest.mark.parametrize("rule", sorted(RULES))
def test_rule(run, rule):
    assert "ok " + rule in run.stdout.splitlines(), RULES[rule] + "\n" + run.stdout[-2000:] + run.stderr[-2000:]
