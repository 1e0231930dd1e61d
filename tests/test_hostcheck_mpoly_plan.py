"""What mzk_mpoly_compose* decides on the host (myzkp_amd/csrc/mzk_mpoly_plan.h: mp_plan, mp_compile) run by
tests/hostcheck/mpoly_plan_shim.cpp, a stand-alone program built with -fsanitize=address,undefined.  Every compiled term program is
interpreted as k_mp_terms runs it, modulo 2^31 - 1, against the naive sum over the terms at random x, and checked for the structure
the kernel relies on (slots below `slots` and inside the variable's depth, POW only above 2 MP_TABLE on a first slot, coefficient
indices in range and each live term read once, the flush bit on exactly the last op of a run, monotone offsets, no ops where every
term vanishes, the LDS bound): exhaustively over the exponents {0 .. 8, 13} for 1 .. 3 terms of 1 and 2 variables and 1 .. 2 terms of
3, each alone and beside a constraint with full depths and another Horner variable, then 10^6 seeded random constraints of 0 .. 8
variables with duplicate rows, empty point polynomials and exponents up to 2^32 - 1.  Every plan against a restatement in 128-bit
integers, the overflow refusals and the field's largest transform.  Then single plans and programs by value.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
E_ARG, E_LENGTH = -1, -5
# ordered constraints over the 10 exponents, alone and beside the fixed constraint
EXHAUSTIVE = 2 * ((10 + 10 ** 2 + 10 ** 3) + (10 ** 2 + 10 ** 4 + 10 ** 6) + (10 ** 3 + 10 ** 6))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mpoly_plan") / "mpoly_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "mpoly_plan_shim.cpp")])
    return exe


def run(shim, *args):
    r = subprocess.run([shim] + [str(a) for a in args], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout


def plan(shim, max_log, lens, terms):
    """one constraint: (err, n, stride_min, bound)"""
    flat = [e for k in terms for e in k]
    return tuple(int(v) for v in run(shim, "plan", max_log, len(lens), len(terms), *lens, *flat).split())


def prog(shim, lens, terms):
    flat = [e for k in terms for e in k]
    head, ops = run(shim, "prog", len(lens), len(terms), *lens, *flat).split("|")
    return [int(v) for v in head.split()], ops.split()


def test_every_program_computes_its_constraint_and_every_plan_its_bound(shim):
    words = run(shim).split()
    assert words[0] == "ok" and words[4] == "ratio", words
    assert int(words[1]) >= EXHAUSTIVE and int(words[2]) >= 10 ** 6 and int(words[3]) >= 10 ** 5, words
    # a term of 8 variables with exponents 4 .. 6 is LOADC and two products each: nothing costs more per term
    assert 1.0 <= float(words[5]) <= 1 + 2 * 8, words


def test_plans_of_known_shapes(shim):
    assert plan(shim, 28, [6, 4], [(2, 1), (0, 3)]) == (0, 16, 14, 14)
    assert plan(shim, 28, [2], [(63,)]) == (0, 64, 64, 64)
    assert plan(shim, 28, [2], [(64,)]) == (0, 128, 65, 65)
    assert plan(shim, 28, [65], [(1,)]) == (0, 128, 65, 65)
    assert plan(shim, 28, [33, 32], [(1, 1)]) == (0, 64, 64, 64)
    assert plan(shim, 28, [4097], [(1,)]) == (0, 8192, 4097, 4097)
    assert plan(shim, 28, [5, 9], [(0, 0)]) == (0, 1, 1, 1)
    # a positive exponent on an empty polynomial: the term vanishes, exponent 0 keeps it
    assert plan(shim, 28, [0, 9], [(1, 2)]) == (0, 1, 0, 0)
    assert plan(shim, 28, [0, 9], [(0, 2), (3, 7)]) == (0, 32, 17, 17)
    # the field's largest transform and one step past it
    assert plan(shim, 28, [2], [((1 << 28) - 1,)]) == (0, 1 << 28, 1 << 28, 1 << 28)
    assert plan(shim, 28, [2], [(1 << 28,)])[0] == E_LENGTH
    assert plan(shim, 32, [2], [(1 << 28,)]) == (0, 1 << 29, (1 << 28) + 1, (1 << 28) + 1)
    assert plan(shim, 32, [2], [((1 << 32) - 1,)]) == (0, 1 << 32, 1 << 32, 1 << 32)
    assert plan(shim, 32, [3], [((1 << 32) - 1,)])[0] == E_LENGTH
    assert plan(shim, 32, [1 << 40], [((1 << 32) - 1,)])[0] == E_LENGTH             # 2^72: refused, not wrapped
    assert plan(shim, 32, [1 << 40, 0], [((1 << 32) - 1, 1)]) == (0, 1, 0, 0)       # ... unless the term vanishes
    assert plan(shim, 32, [2] * 9, [(1,) * 9])[0] == E_ARG


def test_programs_of_known_shapes(shim):
    # gaps 7 (POW, then ADDC) and 2 (HORNER on the slot of x^2), the run ends on the HORNER: flush there
    assert prog(shim, [2], [(9,), (2,), (0,)]) == ([3, 3], ["LOADC.0.0", "POW.0.7", "ADDC.0.1", "HORNER.1.2!"])
    # depth 1, 2, 3 from the largest exponent; 4 .. 6 is x^3 times a table entry
    assert prog(shim, [2], [(1,)]) == ([1, 1], ["LOADC.0.0", "MULT.0.0!"])
    assert prog(shim, [2], [(2,)]) == ([2, 2], ["LOADC.0.0", "MULT.1.0!"])
    assert prog(shim, [2], [(3,)]) == ([3, 3], ["LOADC.0.0", "MULT.2.0!"])
    assert prog(shim, [2], [(4,)]) == ([3, 3], ["LOADC.0.0", "MULT.2.0", "MULT.0.0!"])
    assert prog(shim, [2], [(6,)]) == ([3, 3], ["LOADC.0.0", "MULT.2.0", "MULT.2.0!"])
    assert prog(shim, [2], [(7,)]) == ([3, 3], ["LOADC.0.0", "POW.0.7!"])
    assert prog(shim, [2], [(0,)]) == ([0, 0], ["LOADC.0.0!"])
    # equal rows: ADDC; a tie of the largest exponents: the first variable is the Horner variable
    assert prog(shim, [2, 2], [(2, 2), (1, 2), (1, 2)]) == ([4, 2, 2], ["LOADC.0.0", "HORNER.0.1", "ADDC.0.2", "MULT.0.0", "MULT.3.0!"])
    # the second variable has the largest exponent: runs by the power of the first, constants first
    assert prog(shim, [2, 2], [(1, 5), (1, 1), (0, 0)]) == ([4, 1, 3], ["LOADC.0.2!", "LOADC.0.0", "MULT.3.0", "MULT.1.0", "ADDC.0.1", "MULT.1.0", "MULT.0.0!"])
    # an empty polynomial: its terms leave the program, its exponent still sizes the tables
    assert prog(shim, [0, 2], [(2, 1), (0, 1)]) == ([3, 2, 1], ["LOADC.0.1", "MULT.2.0!"])
