"""The two quotient stages of FastStark::prove on M128, device-resident, at the trace sizes T = 2000, 30000, 120000 (17 colinearity
checks: T + 68 coefficients per trace polynomial), 7 alternated runs each after 2 warm-ups, wall time around a call that ends
synchronised:
  div      mzk_poly_div_roots_dev: two registers, 2 and 1 boundary roots (fast_stark.rs:217-224)
  copy     mzk_selftest_copy_dev of the same rows there and back per root round: what a division round costs in memory traffic alone
  batch    mzk_fast_coset_divide_batch_dev: two transition polynomials of 2 (T + 67) + 1 coefficients over the zerofier of T - 1 roots
  rows     the same two divisions through mzk_fast_coset_divide, one row at a time from host buffers (the form that existed before);
           checked equal to `batch`
    python tools/timing/stark_quotients_time.py [T ...] [--no-settle]"""
import sys, os, time, ctypes, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, orc, myzkp_amd as mz
mz.init(0)
L = mz.lib()
M = mz.FIELD_M128
st = torch.cuda.current_stream().cuda_stream
RUNS, WARM = 7, 2


def synth(seed, n):
    t = torch.empty(n * 2, dtype=torch.int64, device="cuda")
    assert L.mzk_synth_field_dev(M, ctypes.c_uint64(seed), ctypes.c_size_t(n), ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(st)) == 0
    return t


_pad = torch.zeros(4, dtype=torch.int64, device="cuda")


def settle():
    """untimed: one 16-byte device copy and a wait.  The first launch after a call that returned megabytes into pageable host memory
    (`rows`) waits 17 - 27 ms on this runtime, whatever that launch is; without this the next callable's clock would carry it."""
    if "--no-settle" in sys.argv:
        return
    assert L.mzk_selftest_copy_dev(ctypes.c_void_p(_pad.data_ptr()), ctypes.c_void_p(_pad.data_ptr() + 16), ctypes.c_size_t(16), ctypes.c_void_p(st)) == 0
    torch.cuda.synchronize()


def timed(fns):
    """alternate the callables; {name: [ms]}"""
    out = {k: [] for k in fns}
    for r in range(WARM + RUNS):
        for k, f in fns.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            if r >= WARM:
                out[k].append((time.perf_counter() - t0) * 1e3)
            settle()
    return out


def line(name, v, note=""):
    print("  %-6s min %.3f  median %.3f  max %.3f ms (%d runs)   %s" % (name, min(v), statistics.median(v), max(v), len(v), note), flush=True)


print("device:", torch.cuda.get_device_name(0))
for T in [int(a) for a in sys.argv[1:] if a.isdigit()] or [2000, 30000, 120000]:
    n = T + 68
    lg = (2 * n).bit_length()
    omicron = orc.root_of(M, lg)
    print("T=%d: trace polynomials of %d coefficients, omicron domain 2^%d" % (T, n, lg))
    rows = synth(1, 2 * n)
    quo = torch.empty_like(rows)
    roots = [[1, pow(omicron, T - 1, orc.MOD[M])], [1]]
    div = lambda: mz.poly_div_roots_dev(M, rows.data_ptr(), n, [n, n], roots, quo.data_ptr(), st)

    def copy():                                     # round 1: two rows, round 2: one row
        for k in (2, 1):
            assert L.mzk_selftest_copy_dev(ctypes.c_void_p(rows.data_ptr()), ctypes.c_void_p(quo.data_ptr()), ctypes.c_size_t(k * n * 16), ctypes.c_void_p(st)) == 0
    # numerators: multiples of the zerofier's shape are not needed for timing -- the recipe does the same work on any numerator
    ln = 2 * (n - 1) + 1
    zer = synth(2, T)                               # T - 1 roots: T coefficients
    num = synth(3, 2 * ln)
    tq = torch.empty_like(num)
    batch = lambda: mz.fast_coset_divide_batch_dev(M, num.data_ptr(), ln, [ln, ln], zer.data_ptr(), T, orc.M128_GEN, omicron, 1 << lg, tq.data_ptr(), ln, st)
    h_num = num.cpu().numpy().view(np.uint64).reshape(2, ln, 2)
    h_zer = zer.cpu().numpy().view(np.uint64).reshape(T, 2)
    host_rows = lambda: [mz.fast_coset_divide(M, h_num[i], h_zer, orc.M128_GEN, omicron, 1 << lg) for i in range(2)]
    lens = batch()
    torch.cuda.synchronize()
    got = tq.cpu().numpy().view(np.uint64).reshape(2, ln, 2)
    same = all(np.array_equal(got[i][:lens[i]], q) for i, q in enumerate(host_rows()))
    res = timed({"div": div, "copy": copy, "batch": batch, "rows": host_rows})
    line("div", res["div"], "%d + %d coefficient-rounds" % (2 * n, n))
    line("copy", res["copy"])
    line("batch", res["batch"], "quotients of %s coefficients" % lens)
    line("rows", res["rows"], "equal to batch: %s; batch is %.1fx faster by the medians" % (same, statistics.median(res["rows"]) / statistics.median(res["batch"])))
