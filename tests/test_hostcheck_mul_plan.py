"""What mzk_fft_multiply and mzk_fast_multiply decide on the host (myzkp_amd/csrc/mzk_mul_plan.h: fft_mul_plan, fast_mul_plan) run by
tests/hostcheck/mul_plan_shim.cpp, a stand-alone program built with -fsanitize=address,undefined, against a restatement of the
reference's control flow on lengths (polynomial.rs:242-276, ntt.rs:7-23, :66-116): every la, lb in 0 .. 70, every count of trailing
zero coefficients in each operand and, for fast_multiply, every root_order in {2, 4, ..., 4096} -- the error code, the empty result,
the order, the squarings of the root, the copy counts (never above the order: the copies are made into buffers of exactly `order`
bytes) and the kept prefix.  Then single plans: the empty operand against 2^k + 1 coefficients, whose buffers were once sized one
element short of the copy, and the shapes at which an order, a path or a refusal changes.  CPU only."""
import os, subprocess
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_LEN, ROOT_ORDERS = 70, 12
E_ARG, E_NOT_POW2, E_LENGTH = -1, -2, -5
FIELDS = ("err", "empty", "small", "order", "squarings", "copy_a", "copy_b", "keep", "trim")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mul_plan") / "mul_plan_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "mul_plan_shim.cpp")])
    return exe


def plan(shim, *args):
    out = subprocess.run([shim] + [str(a) for a in args], capture_output=True, text=True, check=True).stdout.split()
    return dict(zip(FIELDS, (int(v) for v in out)))


def test_every_plan_agrees_with_the_reference_control_flow(shim):
    r = subprocess.run([shim], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    words = r.stdout.split()
    pairs = (MAX_LEN + 1) ** 2
    with_zeros = ((MAX_LEN + 1) * (MAX_LEN + 2) // 2) ** 2          # sum over la, lb of (la + 1)(lb + 1)
    assert words[0] == "ok" and int(words[1]) >= pairs and int(words[2]) >= with_zeros * ROOT_ORDERS, r.stdout


def test_an_empty_operand_is_the_empty_product_before_anything_is_sized(shim):
    """la = 0, lb = 2^k + 1: m = 2^k = n, one less than the elements of b -- nothing is copied, nothing runs"""
    for lb in (1, 2, 3, 5, 9, 129, 4097, (1 << 20) + 1):
        for la_, lb_ in ((0, lb), (lb, 0)):
            p = plan(shim, "fft", la_, lb_)
            assert p["err"] == 0 and p["empty"] == 1 and p["order"] == 0 and p["copy_a"] == 0 and p["copy_b"] == 0, (la_, lb_, p)
    assert plan(shim, "fft", 0, 0)["err"] == E_LENGTH
    for da, db in ((0, 3), (3, 0), (0, 0)):
        p = plan(shim, "fast", 40, 40, da, db, 1024)
        assert p["err"] == 0 and p["empty"] == 1 and p["order"] == 0, (da, db, p)


def test_plans_of_known_shapes(shim):
    ok = dict(err=0, empty=0, small=0, squarings=0, trim=1)
    assert plan(shim, "fft", 1, 1) == dict(ok, order=1, copy_a=1, copy_b=1, keep=1)
    assert plan(shim, "fft", 40, 25) == dict(ok, order=64, copy_a=40, copy_b=25, keep=64)
    assert plan(shim, "fft", 33, 33) == dict(ok, order=128, copy_a=33, copy_b=33, keep=65)
    assert plan(shim, "fft", (1 << 19) + 1, 8) == dict(ok, order=1 << 20, copy_a=(1 << 19) + 1, copy_b=8, keep=(1 << 19) + 8)
    # degree 7: the small path whatever root_order is, operands taken without their trailing zeros
    assert plan(shim, "fast", 40, 40, 5, 4, 2) == dict(ok, small=1, order=16, copy_a=5, copy_b=4, keep=8)
    # degree 8: order 16 from 2^14 is ten squarings; degree 15 still fits 16, degree 16 takes 32
    ntt = dict(ok, trim=0)
    assert plan(shim, "fast", 5, 5, 5, 5, 1 << 14) == dict(ntt, order=16, squarings=10, copy_a=5, copy_b=5, keep=16)
    assert plan(shim, "fast", 9, 8, 9, 8, 1 << 14) == dict(ntt, order=16, squarings=10, copy_a=9, copy_b=8, keep=16)
    assert plan(shim, "fast", 9, 9, 9, 9, 1 << 14) == dict(ntt, order=32, squarings=9, copy_a=9, copy_b=9, keep=32)
    # no halving: the cyclic product is the reference's
    assert plan(shim, "fast", 12, 12, 12, 12, 16) == dict(ntt, order=16, squarings=0, copy_a=12, copy_b=12, keep=16)
    # stored length: up to the order it is copied whole, one more is the reference's panic inside ntt
    assert plan(shim, "fast", 32, 20, 10, 10, 1024) == dict(ntt, order=32, squarings=5, copy_a=32, copy_b=20, keep=32)
    assert plan(shim, "fast", 33, 20, 10, 10, 1024)["err"] == E_LENGTH
    assert plan(shim, "fast", 11, 11, 11, 11, 48)["err"] == E_NOT_POW2          # order 24
    assert plan(shim, "fast", 3, 3, 4, 3, 16)["err"] == E_ARG
