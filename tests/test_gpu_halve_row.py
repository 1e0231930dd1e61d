"""The late halving steps of the bucket reduction on row operations (k_halve_multi_row, myzkp_amd/csrc/mzk_msm_row.hip; the launch list:
halve_plan, mzk_msm_plan.h).  Commits against window tables on a SHORT SRS (2^13 points), so that the bucket sets are the workload's and
a commit takes a millisecond:
  17 bits  2^16 buckets as in the flagship commit: k_halve_multi, then steps 8..11 and 12..15 as two row launches of four steps;
  16, 15, 14 bits  a last row launch of three, two and one step(s) (steps 12.., after a launch of four);
  11 bits  2^10 buckets: one k_halve_multi launch and the tail (no step is left for a row launch at this width -- the list is pinned by
           tests/test_hostcheck_halve_plan.py; the layout is here because the tail then starts from what a launch of eight steps left).
Inputs: uniform scalars; all scalars equal; every digit inside ONE fold-only region; one occupied bucket only, at the edges of the
regions and of the workgroups' records; and for every step of the row launches two occupied buckets exactly that step's stride apart
-- in region 0 and in the fold-only region 1 -- holding equal points (the addition is a doubling: rowop::add_slow), opposite points
(it cancels to infinity), or one of them nothing.  The SRS repeats one point P eight times and holds -P eight times; a scalar is a digit
times 2^(C w), so its only entry is that digit's bucket (checked on the CPU by the signed-digit walk).
Every commit is compared with the oracle's Pippenger as an affine point, and again through the XYZZ partial record folded by
mzk_g1_fold_partials_dev; with the tuning build MZK_HALVE_ROW = 0 and 1 must give the same affine bytes (one child process each).
(MZK_TAIL_PREWEIGHT does not exist: the tail's weights stayed where they were.)"""
import ctypes, functools, os, subprocess, sys
import numpy as np
import pytest
import orc
from orc import FR, P_FQ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N = 1 << 13
LAYOUTS = (17, 16, 15, 14, 11)
ROW_FROM = 8                 # the first step of the row launches wherever there are any (halve_plan: after k_halve_multi's eight)
I_P, I_NEG = 0, 8            # SRS rows 0..7 hold P, rows 8..15 hold -P


@functools.lru_cache(maxsize=None)
def points():
    p = orc.synth_points(51, N)
    P = p[100].copy()
    Pn = P.copy()
    Pn[4:] = orc.to_limbs([P_FQ - orc.from_limbs(P[None, 4:])[0]], 4)[0]
    p[I_P:I_P + 8] = P
    p[I_NEG:I_NEG + 8] = Pn
    p.setflags(write=False)
    return p


def digit_scalars(C, entries):
    """entries (SRS row, window, digit 1 .. 2^(C-1)) -> N scalars, zero but for sum digit 2^(C window) at each row: no digit exceeds
    half the window, so nothing carries and every entry is ONE bucket entry, digit - 1"""
    vals = [0] * N
    for i, w, d in entries:
        assert 1 <= d <= 1 << (C - 1) and 0 <= w <= 254 // C - 2
        vals[i] += d << (C * w)
    assert max(vals) < orc.P_FR
    return orc.to_limbs(vals, 4)


def occupied(C, scal):
    """the buckets the scalars' signed C-bit digits land in (walk_digits, mzk_msm_plan.h)"""
    half, out = 1 << (C - 1), set()
    for v in (int(x) for x in orc.from_limbs(scal) if x):
        carry = 0
        for w in range(254 // C + 1):
            raw = ((v >> (C * w)) & ((1 << C) - 1)) + carry
            carry = 1 if raw > half else 0
            mag = (1 << C) - raw if carry else raw
            if mag:
                out.add(mag - 1)
    return out


def pair_cases(C, t, base, tag):
    """buckets base and base + stride of step t: step t adds the second onto the first, no earlier step touches either"""
    lgB = C - 1
    stride = 1 << (lgB - t - 1)
    lo, hi, w = base + 1, base + stride + 1, t % 5
    out = {
        "equal": [(I_P, w, lo), (I_P + 1, w, hi)],
        "opposite": [(I_P + 2, w, lo), (I_NEG, w, hi)],
        "only_upper": [(I_P + 3, w, hi)],
        "only_lower": [(I_NEG + 1, w, lo)],
    }
    res = {}
    for what, ent in out.items():
        s = digit_scalars(C, ent)
        assert occupied(C, s) == {d - 1 for _, _, d in ent}
        res["%d-bit step %d %s %s" % (C, t, tag, what)] = (C, s)
    return res


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (window bits, scalars); every commit takes all N points of points()"""
    out = {}
    rng = np.random.default_rng(11)
    for C in LAYOUTS:
        lgB, half = C - 1, 1 << (C - 1)
        out["%d-bit uniform" % C] = (C, orc.synth_vector(FR, 60 + C, N))
        eq = orc.synth_vector(FR, 80 + C, N)
        eq[:] = eq[7]
        out["%d-bit all equal" % C] = (C, eq)
        # region 1 alone: digits in (half / 2, half], buckets [2^(lgB-1), 2^lgB) -- it only folds from step 1 on
        dig = rng.integers(half // 2 + 1, half + 1, size=(N, 4))
        s = digit_scalars(C, [(i, w, int(dig[i, w])) for i in range(N) for w in range(4)])
        assert min(occupied(C, s)) >= half // 2
        out["%d-bit one fold-only region" % C] = (C, s)
        for b in (0, 1, 15, 16, 255, 256, half // 2 - 1, half // 2, half - 1):
            if b < half:
                s = digit_scalars(C, [(200 + b % 7, 2, b + 1)])
                assert occupied(C, s) == {b}
                out["%d-bit only bucket %d" % (C, b)] = (C, s)
        for t in range(ROW_FROM, lgB):
            out.update(pair_cases(C, t, 0, "region 0"))
            if C == 17:
                out.update(pair_cases(C, t, half // 2, "region 1"))
    return out


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def commit_both_ways(mz, h, scal):
    """[the affine bytes, the XYZZ partial record folded to affine bytes]"""
    import torch
    L = mz.lib()
    st, d_c = _stream(), _dev(scal)
    aff = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    part = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    folded = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    assert L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(N), ctypes.c_void_p(aff.data_ptr()), 0, st) == 0, L.mzk_last_error()
    assert L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(N), ctypes.c_void_p(part.data_ptr()), 1, st) == 0, L.mzk_last_error()
    assert L.mzk_g1_fold_partials_dev(ctypes.c_void_p(part.data_ptr()), 1, ctypes.c_void_p(folded.data_ptr()), st) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    return [o.cpu().numpy().tobytes() for o in (aff, folded)]


def run_cases(mz):
    import torch
    L = mz.lib()
    d_p, res = _dev(points()), {}
    for C in LAYOUTS:
        h = ctypes.c_void_p()
        assert L.mzk_srs_from_device_ex(ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(N), C, ctypes.byref(h), _stream()) == 0, L.mzk_last_error()
        torch.cuda.synchronize()
        assert (L.mzk_srs_window_bits(h), L.mzk_srs_bucket_sets(h)) == (C, 1)
        for name, (c, scal) in cases().items():
            if c == C:
                res[name] = commit_both_ways(mz, h, scal)
        L.mzk_srs_free(h)
    return res


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import myzkp_amd as mz
import test_gpu_halve_row as t
mz.init(0)
print(repr(t.run_cases(mz)))
'''


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    return myzkp_amd


@pytest.fixture(scope="module")
def want():
    p = points()
    return {name: orc.msm_fast(scal, p) for name, (_, scal) in cases().items()}


def as_point(mz, raw):
    return mz.array_to_points(np.frombuffer(raw, dtype=np.uint64).reshape(1, 8))[0]


@pytest.fixture(scope="module")
def shipped(mz):
    return run_cases(mz)


@pytest.fixture(scope="module")
def switched():
    """the same calls with MZK_HALVE_ROW = 0 (k_halve_multi all the way) and 1: the switch is read once per process, so a child each"""
    import myzkp_amd.build as b
    tuning = b.build(tuning=True)
    procs = {v: subprocess.Popen([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, MZK_HIP_LIB=tuning, MZK_HALVE_ROW=str(v)),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for v in (0, 1)}
    res = {}
    for v, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, (v, err[-2000:])
        res[v] = eval(out.strip().splitlines()[-1])
    return res


@pytest.mark.parametrize("kind", ["uniform", "all equal", "one fold-only region", "only bucket", "step"])
@pytest.mark.parametrize("C", LAYOUTS)
def test_commit_equals_the_oracle_as_a_point_and_as_a_folded_partial(mz, want, shipped, C, kind):
    names = [n for n in want if n.startswith("%d-bit %s" % (C, kind))]
    assert names
    for name in names:
        assert [as_point(mz, raw) for raw in shipped[name]] == [want[name]] * 2, name


def test_both_settings_of_the_switch_give_the_same_bytes(mz, want, shipped, switched):
    assert set(switched[0]) == set(switched[1]) == set(want)
    for name, w in want.items():
        assert switched[0][name] == switched[1][name] == shipped[name], name
        assert as_point(mz, switched[0][name][0]) == w, name
