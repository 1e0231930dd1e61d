"""The digit walk of the window-table layouts (raw_window / walk_digits_whole / digit_bias_word / walk_digits_merged<C> in
myzkp_amd/csrc/mzk_msm_plan.h: the code that decides every bucket and every table row of a commit) run on the host by
tests/hostcheck/digit_walk_shim.cpp, a stand-alone program built with -fsanitize=address,undefined, over msm_layouts.family() and
uniform scalars: every layout of msm_layouts.LAYOUTS through the run-time walk, every width 8..22 through the compile-time one (the
library instantiates eight of the fifteen).  Checked here in integers.  CPU only."""
import os, random, subprocess
import pytest
import msm_layouts
from msm_layouts import R, N_SRS, rows

HERE = os.path.dirname(os.path.abspath(__file__))
UNIFORM = 2000


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    """(scalars, {(index, c, sets): triples of walk_digits_whole}, {(index, C): triples of walk_digits_merged<C>})"""
    d = tmp_path_factory.mktemp("digit_walk")
    exe = str(d / "digit_walk_shim")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(HERE, "hostcheck", "digit_walk_shim.cpp")])
    rng = random.Random(77)
    scalars = msm_layouts.family() + [rng.randrange(R) for _ in range(UNIFORM)]
    src = str(d / "scalars.txt")
    with open(src, "w") as f:
        f.write("".join("%x\n" % k for k in scalars))
    r = subprocess.run([exe, src, str(N_SRS)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok %d" % len(scalars)
    whole, merged = {}, {}
    for ln in lines[:-1]:
        f = ln.split()
        if f[0] == "W":
            whole[(int(f[1]), int(f[2]), int(f[3]))] = tuple(map(int, f[4:]))
        else:
            assert f[0] == "M"
            merged[(int(f[1]), int(f[2]))] = tuple(map(int, f[3:]))
    return scalars, whole, merged


def test_the_compile_time_walk_equals_the_run_time_walk_at_every_width(walked):
    scalars, whole, merged = walked
    assert len(merged) == len(scalars) * len(msm_layouts.WIDTHS)
    for (i, c), triples in merged.items():
        assert triples == whole[(i, c, 1)], (c, hex(scalars[i]))


def test_every_window_lands_in_its_bucket_set_and_table_row(walked):
    scalars, whole, _ = walked
    assert len(whole) == len(scalars) * len(msm_layouts.LAYOUTS)
    for c, s in msm_layouts.LAYOUTS:
        half, nwin = 1 << (c - 1), 254 // c + 1
        for i, k in enumerate(scalars):
            t = whole[(i, c, s)]
            where = (c, s, hex(k))
            wins, keys, pays = t[0::3], t[1::3], t[2::3]
            want = [(w, d) for w, d in enumerate(msm_layouts.signed_digits(k, c)) if d]
            assert list(wins) == [w for w, _ in want] and all(0 <= w < nwin for w in wins), where      # one triple per non-zero digit, in order
            total = 0
            for (w, d), key, pay in zip(want, keys, pays):
                ref, neg = pay & 0x7fffffff, pay >> 31
                assert key < s << (c - 1) and ref < rows(c, s) * N_SRS, where
                assert key >> (c - 1) == w % s and ref // N_SRS == w // s and ref % N_SRS == i, where
                mag = (key & (half - 1)) + 1
                assert (-mag if neg else mag) == d, where
                total += (-mag if neg else mag) << (c * w)
            assert total == k, where
