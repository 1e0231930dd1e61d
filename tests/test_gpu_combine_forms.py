"""The two forms of the segment combine (myzkp_amd/csrc/mzk_msm.hip): k_seg_combine, a DPP quad per bucket, and k_seg_combine_wide,
a lane per bucket with the next partial's record on its way, which msm_plan selects for the one merged bucket set from
64 x 4 x CUs buckets on.  Every case commits against 17-bit window tables on a SHORT SRS (2^11 to 2^13 points): 2^16 buckets, the
two-level path and the lane form in milliseconds.  Every result is compared as an affine point with the oracle's Pippenger on the
same inputs, and with the same calls made with either form forced (MZK_COMBINE_FORM of the tuning build, one child process per form).

The cases: uniform scalars (buckets of no or one partial); buckets whose entry counts sit on every boundary of the combine (chains of
1, 2, 3, 32 partials, and 33 and 34, which are deferred to k_seg_combine_heavy), constructed digit by digit and checked by a digit
histogram on the CPU; heavy buckets only (equal scalars, a bit vector, one bucket shared by many workgroups); buckets whose partials
are equal, opposite or the point at infinity.  Each with the affine result and with the XYZZ partial record, the affine call twice
in a row on one stream and workspace, and two commits in flight on two contexts."""
import ctypes, functools, os, subprocess, sys
import numpy as np
import pytest
import orc
from orc import FR, P_FQ

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
C = 17                       # window bits: 2^16 buckets in one set
NWIN = 254 // C + 1          # 15 windows
HALF = 1 << (C - 1)
SEG_MIN = 8                  # mzk_msm.hip: the shortest segment the kernels derive from the entry count
HEAVY_SLOTS = 32             # mzk_msm_plan.h: a bucket of more partials is deferred to k_seg_combine_heavy
TABLES = 2
N_MAIN, N_EDGE = 1 << 13, 1 << 11


# ---- the inputs (the children rebuild them from the same seeds) ---------------------------------------------------------------------
def scalars_of(ch):
    """digit matrix (n, NWIN), digits in [0, HALF]: no signed-digit carry, so digit v of any window is one entry of bucket v - 1"""
    assert ch.shape[1] == NWIN and int(ch.max()) <= HALF
    vals = [sum(int(v) << (C * w) for w, v in enumerate(row) if v) for row in ch]
    assert max(vals) < orc.P_FR
    return orc.to_limbs(vals, 4)


def boundary_digits(n, seg):
    """buckets (id, entries) in ascending order; with segments of `seg` entries their chains are 1, 2, 2, 3, 1 (filler), 32 from a segment
    boundary, 33 from a segment boundary, 34 -- behind them a background of single entries in higher buckets"""
    plan = [(0, 1), (100, seg), (200, seg + 1), (300, 2 * seg), (400, seg - 2), (500, 32 * seg), (600, 32 * seg + 1), (700, 33 * seg)]
    rng = np.random.default_rng(5)
    ch = rng.integers(2000, HALF + 1, size=(n, NWIN), dtype=np.int64) * (rng.random((n, NWIN)) < 0.3)
    ch[:, NWIN - 1] = 0                                       # (the top window holds 16 bits: left zero, the scalars stay below r)
    k = 0
    for b, cnt in plan:
        for _ in range(cnt):
            ch[(7 * k) % n, k % (NWIN - 1)] = b + 1           # (7 k mod n is one-to-one below n: no cell is written twice)
            k += 1
    assert k < n
    return ch, plan


def edge_inputs(n, seg):
    """One point P, its negation and the point at infinity repeated over the SRS, all entries of a special bucket in ONE window (the same
    table row): whatever order the sort leaves a bucket's entries in, the partials of
       bucket 10: 2 seg x P from a segment boundary              are equal (a doubling in the combine),
       bucket 20: seg x P and seg x -P                           are opposite, or both infinity,
       bucket 30: 2 seg x infinity and seg x P                   include infinity,
       bucket 40: seg x P, seg x -P, seg x P                     sum to seg x P through three partials,
       bucket 50: 3 x P (moves the next bucket off the boundary), bucket 60: (seg + 4) x P and (seg + 4) x -P across four segments"""
    p = orc.synth_points(41, n)
    P = p[5].copy()
    Pn = P.copy()
    Pn[4:] = orc.to_limbs([P_FQ - orc.from_limbs(P[None, 4:])[0]], 4)[0]
    rng = np.random.default_rng(6)
    ch = np.zeros((n, NWIN), dtype=np.int64)
    ch[:, :3] = rng.integers(2000, HALF + 1, size=(n, 3), dtype=np.int64)          # background: single entries in higher buckets
    plan = [(10, [("P", 2 * seg)]), (20, [("P", seg), ("N", seg)]), (30, [("O", 2 * seg), ("P", seg)]), (40, [("P", seg), ("N", seg), ("P", seg)]),
            (50, [("P", 3)]), (60, [("P", seg + 4), ("N", seg + 4)])]
    i = 8
    for b, parts in plan:
        for what, cnt in parts:
            for _ in range(cnt):
                p[i] = {"P": P, "N": Pn, "O": 0}[what]
                ch[i] = 0
                ch[i, 3] = b + 1
                i += 1
    assert i < n
    return ch, p, [(b, sum(c for _, c in parts)) for b, parts in plan]


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (scalars, points): the SRS of a case is its points, the commit takes all of them"""
    pm = orc.synth_points(31, N_MAIN)
    out = {}
    out["uniform"] = (orc.synth_vector(FR, 32, 1 << 12), pm[:1 << 12])
    out["boundaries"] = (scalars_of(boundary_digits(1 << 12, SEG_MIN)[0]), pm[:1 << 12])
    eq = orc.synth_vector(FR, 33, 1 << 12)
    eq[:] = eq[7]
    out["equal"] = (eq, pm[:1 << 12])                                                 # fifteen buckets hold everything
    bits = np.zeros((N_MAIN, 4), dtype=np.uint64)
    bits[:, 0] = np.random.default_rng(7).integers(0, 2, size=N_MAIN).astype(np.uint64)
    out["bits"] = (bits, pm)                                                          # one bucket
    out["one_bucket"] = (scalars_of(np.full((N_MAIN, NWIN), 1000, dtype=np.int64)), pm)   # every digit of every scalar: workgroups share it
    ch, pe, _ = edge_inputs(N_EDGE, SEG_MIN)
    out["edge"] = (scalars_of(ch), pe)
    return out


# ---- what the kernels make of them, on the CPU ---------------------------------------------------------------------------------------
def bucket_counts(scal):
    """entries per bucket: the signed c-bit digits of walk_digits (mzk_msm_plan.h), bucket |d| - 1"""
    cnt = np.zeros(HALF, dtype=np.int64)
    for v in orc.from_limbs(scal):
        carry = 0
        for w in range(NWIN):
            raw = ((v >> (C * w)) & ((1 << C) - 1)) + carry
            carry = 1 if raw > HALF else 0
            mag = (1 << C) - raw if carry else raw
            if mag:
                cnt[mag - 1] += 1
    return cnt


def chains(cnt, seg):
    """bucket -> (partials, first entry) as k_seg_combine* see them: slots offsets[b] / seg + b .. (offsets[b + 1] - 1) / seg + b"""
    off = np.concatenate([[0], np.cumsum(cnt)])
    return {int(b): (int((off[b + 1] - 1) // seg - off[b] // seg + 1), int(off[b])) for b in np.nonzero(cnt)[0]}


def device_seg(n, total, num_cu):
    """segment_length (mzk_msm.hip) over msm_plan's segment count for n pairs against 17-bit tables"""
    e_max = n * NWIN
    lanes = num_cu * 4 * 3 * 64
    seg_host = max(16, -(-e_max // lanes))
    t_max = -(-e_max // seg_host)
    return max(SEG_MIN, -(-total // t_max))


# ---- the calls ---------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _srs(mz, pts):
    import torch
    L = mz.lib()
    d_p, h = _dev(pts), ctypes.c_void_p()
    assert L.mzk_srs_from_device_ex(ctypes.c_void_p(d_p.data_ptr()), ctypes.c_size_t(pts.shape[0]), C, ctypes.byref(h), _stream()) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    assert (L.mzk_srs_window_bits(h), L.mzk_srs_bucket_sets(h)) == (C, 1)
    return h


def commit_all_ways(mz, h, scal):
    """[affine, affine again on the same stream and workspace, the XYZZ partial record folded to a point]"""
    import torch
    L = mz.lib()
    n, st = scal.shape[0], _stream()
    d_c = _dev(scal)
    outs = [torch.full((8,), -1, dtype=torch.int64, device="cuda") for _ in range(3)]
    part = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    for k in range(2):          # back to back, nothing in between: what the first call left in the workspace meets the second
        assert L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(n), ctypes.c_void_p(outs[k].data_ptr()), 0, st) == 0, L.mzk_last_error()
    assert L.mzk_kzg_commit_srs_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(n), ctypes.c_void_p(part.data_ptr()), 1, st) == 0, L.mzk_last_error()
    assert L.mzk_g1_fold_partials_dev(ctypes.c_void_p(part.data_ptr()), 1, ctypes.c_void_p(outs[2].data_ptr()), st) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    return [mz.array_to_points(o.cpu().numpy().view(np.uint64).reshape(1, 8))[0] for o in outs]


def run_cases(mz):
    res = {}
    for name, (scal, pts) in cases().items():
        h = _srs(mz, pts)
        res[name] = commit_all_ways(mz, h, scal)
        mz.lib().mzk_srs_free(h)
    return res


CHILD = r'''
import sys
sys.path.insert(0, "tests")
import myzkp_amd as mz
import test_gpu_combine_forms as t
mz.init(0)
print(repr(t.run_cases(mz)))
'''


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd
    myzkp_amd.init(0)
    yield myzkp_amd
    myzkp_amd.init_devices([0])


@pytest.fixture(scope="module")
def want():
    return {name: orc.msm_fast(scal, pts) for name, (scal, pts) in cases().items()}


@pytest.fixture(scope="module")
def shipped(mz):
    return run_cases(mz)


@pytest.fixture(scope="module")
def forced():
    """the same calls with the quad form (1) and the lane form (2) forced: the switch is read once per process, so a child per form,
    both at once"""
    import myzkp_amd.build as b
    tuning = b.build(tuning=True)
    procs = {form: subprocess.Popen([sys.executable, "-c", CHILD], cwd=ROOT, env=dict(os.environ, MZK_HIP_LIB=tuning, MZK_COMBINE_FORM=str(form)),
                                    stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for form in (1, 2)}
    res = {}
    for form, p in procs.items():
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, (form, err[-2000:])
        res[form] = eval(out.strip().splitlines()[-1])
    return res


def test_the_constructed_buckets_sit_on_the_boundaries():
    """the digit histogram of the constructed scalars, and the chains the kernels cut it into: fails if a boundary is missed"""
    import torch
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = 1 << 12
    ch, plan = boundary_digits(n, SEG_MIN)
    cnt = bucket_counts(scalars_of(ch))
    seg = device_seg(n, int(cnt.sum()), num_cu)
    assert seg == SEG_MIN, (seg, int(cnt.sum()))
    assert [int(cnt[b]) for b, _ in plan] == [c for _, c in plan] == [1, seg, seg + 1, 2 * seg, seg - 2, 32 * seg, 32 * seg + 1, 33 * seg]
    assert int(cnt[:1999].sum()) == sum(c for _, c in plan)              # nothing else in front of or between them
    got = chains(cnt, seg)
    assert [got[b][0] for b, _ in plan] == [1, 2, 2, 3, 1, HEAVY_SLOTS, HEAVY_SLOTS + 1, HEAVY_SLOTS + 2]
    assert got[500][1] % seg == 0 and got[600][1] % seg == 0           # the last bucket kept and the first one deferred start on a boundary
    assert max(v[0] for b, v in got.items() if b >= 1999) <= 2          # the background is ordinary
    # heavy only: fifteen / one / one bucket(s), every one deferred, the last shared by several workgroups (more than 16 x 64 partials)
    cs = cases()
    for name, nb, least in (("equal", NWIN, HEAVY_SLOTS + 1), ("bits", 1, HEAVY_SLOTS + 1), ("one_bucket", 1, 16 * 64 + 1)):
        scal = cs[name][0]
        c2 = bucket_counts(scal)
        g2 = chains(c2, device_seg(scal.shape[0], int(c2.sum()), num_cu))
        assert len(g2) <= nb and min(v[0] for v in g2.values()) >= least, (name, g2)
    # exceptional operands: the special buckets hold what edge_inputs says, from the boundaries it says
    ch, _, eplan = edge_inputs(N_EDGE, SEG_MIN)
    c3 = bucket_counts(scalars_of(ch))
    seg = device_seg(N_EDGE, int(c3.sum()), num_cu)
    assert seg == SEG_MIN and [int(c3[b]) for b, _ in eplan] == [c for _, c in eplan] and int(c3[:1999].sum()) == sum(c for _, c in eplan)
    g3 = chains(c3, seg)
    assert [(g3[b][0], g3[b][1] % seg) for b, _ in eplan] == [(2, 0), (2, 0), (3, 0), (3, 0), (1, 0), (4, 3)]


@pytest.mark.parametrize("name", ["uniform", "boundaries", "equal", "bits", "one_bucket", "edge"])
def test_commit_equals_the_oracle_in_every_output_form(want, shipped, name):
    assert shipped[name] == [want[name]] * 3, name


@pytest.mark.parametrize("form", [1, 2])
def test_forced_forms_give_the_same_points(want, forced, form):
    for name, w in want.items():
        assert forced[form][name] == [w] * 3, (form, name)


def test_two_commits_in_flight_on_two_contexts(mz, want):
    """mzk_kzg_commit_srs_batch_dev with two contexts: each commit has its own workspace, heavy list and counters"""
    import torch
    mz.init_devices([0, 0])
    L = mz.lib()
    cs = cases()
    pts = cs["equal"][1]
    names = ["boundaries", "equal", "uniform", "equal"]
    n = pts.shape[0]
    assert all(cs[k][0].shape[0] == n and cs[k][1] is not None for k in names)
    h = _srs(mz, pts)
    d_c = _dev(np.stack([cs[k][0] for k in names]))
    d_o = torch.full((len(names) * 8,), -1, dtype=torch.int64, device="cuda")
    assert L.mzk_kzg_commit_srs_batch_dev(h, ctypes.c_void_p(d_c.data_ptr()), ctypes.c_size_t(n), ctypes.c_size_t(len(names)), ctypes.c_void_p(d_o.data_ptr()),
                                          ctypes.c_int(2), _stream()) == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    got = mz.array_to_points(d_o.cpu().numpy().view(np.uint64).reshape(len(names), 8))
    assert got == [want[k] for k in names]
    L.mzk_srs_free(h)
    mz.init_devices([0])
