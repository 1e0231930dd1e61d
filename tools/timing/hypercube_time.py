"""Evaluation tables from sparse factors (mzk_mpoly_hypercube_evals_dev) at el = 16, 20, 24 with k = 3 factors, each with the same number
of distinct support masks in {1, 16, 256, 4096, 65536, 2^el} (uniformly random masks, one term per mask), in the three forms.

Per grid point, after WARM calls, the median over REPS calls (50; 5 from 2^20 masks up, where the host plan alone takes
seconds, and for a forced TILE with more than 2^27 uniform group tests) of
  dev    the device work behind the upload, from the library's event pair MZK_PH_HYPERCUBE (tile kernel, or memset + scatter + passes)
  call   the whole call on the host clock, enqueue to synchronize: host plan, merge, upload and dev
and, once per point, `plan`: mzk_mpoly_hypercube_plan alone on the host clock (the mask / sort / group work, no device).
References from the same process: hipMemsetAsync of the k tables, and mzk_mle_evals_from_coeffs_dev in place on each of the k tables
(the dense butterfly), both between events on the stream.

Gates, on `dev` against the references of the same el (exit status 1 if one fails; the lines say which):
  1  TILE at <= 16 masks within 2 x the memset of the tables
  2  SCATTER within 1.25 x (memset + the k dense butterflies) at every point
  3  AUTO within 1.25 x the faster forced form at every point
Headline: mzk_sumcheck_product_prove_terms_dev with 256 terms per factor, k = d = 3, against mzk_sumcheck_product_prove_dev on tables
copied from pageable host memory first (host clock, copy included), at el = 20 and 24.

Each el runs in a child process of its own under a time limit; the first that fails or runs out of time ends the run.
Not measured: 2^24 masks at el = 24 (a host term table of 4.8 GB), and the forced TILE form where its uniform group tests
(tiles x groups x k) exceed 2^31.
Usage: python tools/timing/hypercube_time.py [--max-el 24] [--out profiles/hypercube_time.txt]"""
import ctypes, os, statistics, subprocess, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)

K = D = 3
WARM, REPS, REPS_LARGE = 2, 50, 5
FORMS = (("auto", 0), ("tile", 1), ("scatter", 2))
LIMIT = {16: 180, 20: 300, 24: 380}
TILE_TEST_CAP = 1 << 31


def hip_runtime():
    """the HIP runtime this process already has (torch's), for hipMemsetAsync"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def run_el(el):
    import numpy as np, torch
    import myzkp_amd as mz
    mz.init(0)
    L = mz.lib()
    hip = hip_runtime()
    PH_HYPERCUBE = next(ph for ph in range(64) if L.mzk_prof_name(ph) == b"hypercube_tables")       # by name: the enum may grow
    SZ, VP = ctypes.c_size_t, ctypes.c_void_p
    stream = torch.cuda.current_stream()
    sp = VP(stream.cuda_stream)
    n = 1 << el
    rng = np.random.default_rng(el)
    g = torch.Generator(device="cuda").manual_seed(el)
    tables = torch.randint(0, 1 << 62, (K, n, 4), dtype=torch.int64, device="cuda", generator=g)
    tables[:, :, 3] &= (1 << 60) - 1
    nbytes = K * n * 32

    def events(fn, reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        out = []
        for it in range(WARM + reps):
            a.record()
            fn()
            b.record()
            b.synchronize()
            if it >= WARM:
                out.append(a.elapsed_time(b))
        return statistics.median(out)

    def butterflies():
        for f in range(K):
            p = tables.data_ptr() + f * n * 32
            assert L.mzk_mle_evals_from_coeffs_dev(VP(p), SZ(el), VP(p), sp) == 0

    def memset():
        assert hip.hipMemsetAsync(VP(tables.data_ptr()), 0, SZ(nbytes), sp) == 0
    t_mle = events(butterflies, 20)          # on random canonical-range limbs first, then the tables are zero
    t_set = events(memset, 20)
    print("# el = %d, k = %d: tables of %d bytes; hipMemsetAsync %.4f ms; %d dense butterflies (mzk_mle_evals_from_coeffs_dev in place) %.4f ms"
          % (el, K, nbytes, t_set, K, t_mle))
    print("# el  masks/factor  groups/factor  plan ms | auto: form dev ms call ms | tile: dev ms call ms | scatter: dev ms call ms | auto/best")
    fails = []
    for M in sorted({1, 16, 256, 4096, 65536, n}):
        if M > n:
            continue
        if M == n and el > 20:
            print("  %2d  %12d  not measured: the host term table alone is %.1f GB" % (el, M, K * M * el * 4 / 1e9))
            continue
        masks = [rng.permutation(n) if M == n else rng.choice(n, size=M, replace=False) for _ in range(K)]
        shifts = (el - 1 - np.arange(el)).astype(np.int64)
        te = np.concatenate([((m.astype(np.int64)[:, None] >> shifts) & 1).astype(np.uint32) for m in masks])
        tc = rng.integers(0, 1 << 62, size=(K * M, 4), dtype=np.int64).astype(np.uint64)
        tc[:, 3] &= np.uint64((1 << 60) - 1)
        toff = (ctypes.c_size_t * (K + 1))(*[f * M for f in range(K + 1)])
        pc, pe = tc.ctypes.data_as(VP), te.ctypes.data_as(VP)
        reps = REPS if M < (1 << 20) else REPS_LARGE
        from myzkp_amd._lib import _HypercubePlan
        plan = _HypercubePlan()
        t_plan = []
        for it in range(1 + min(reps, 9)):
            t0 = time.perf_counter()
            assert L.mzk_mpoly_hypercube_plan(pe, toff, SZ(K), SZ(el), 0, ctypes.byref(plan)) == 0
            t_plan.append((time.perf_counter() - t0) * 1e3)
        t_plan = statistics.median(t_plan[1:])
        res = {}
        for name, form in FORMS:
            if form == 1 and (n >> min(el, 10)) * plan.max_groups * K > TILE_TEST_CAP:
                res[name] = None
                continue
            dev, call = [], []
            tests = (n >> min(el, 10)) * plan.max_groups * K
            for it in range(WARM + (REPS_LARGE if form == 1 and tests > 1 << 27 else reps)):
                L.mzk_prof_reset()
                L.mzk_prof_enable(1)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                rc = L.mzk_mpoly_hypercube_evals_dev(pc, pe, toff, SZ(K), SZ(el), form, VP(tables.data_ptr()), sp)
                assert rc == 0, L.mzk_last_error()
                stream.synchronize()
                t1 = time.perf_counter()
                L.mzk_prof_enable(0)
                ms, cnt = ctypes.c_double(), ctypes.c_uint64()
                L.mzk_prof_read(PH_HYPERCUBE, ctypes.byref(ms), ctypes.byref(cnt))
                assert cnt.value == 1
                if it >= WARM:
                    dev.append(ms.value)
                    call.append((t1 - t0) * 1e3)
            res[name] = (statistics.median(dev), statistics.median(call))
        L.mzk_prof_reset()
        forced = [res[x][0] for x in ("tile", "scatter") if res[x]]
        best = min(forced)
        fmt = lambda r: "%9.4f %9.3f" % r if r else "  skipped: too many group tests"
        ratio = res["auto"][0] / best
        print("  %2d  %12d  %13d  %7.3f | %s %s | %s | %s | %.2f" % (el, M, plan.max_groups, t_plan, "TILE   " if plan.form == 1 else "SCATTER", fmt(res["auto"]),
                                                                     fmt(res["tile"]), fmt(res["scatter"]), ratio))
        if M <= 16:
            r1 = res["tile"][0] / t_set
            print("#     gate 1: TILE / memset = %.2f (limit 2.00) -> %s" % (r1, "ok" if r1 <= 2.0 else "FAIL"))
            if r1 > 2.0:
                fails.append("1 (el %d, %d masks: %.2f)" % (el, M, r1))
        r2 = res["scatter"][0] / (t_set + t_mle)
        print("#     gate 2: SCATTER / (memset + butterflies) = %.2f (limit 1.25) -> %s" % (r2, "ok" if r2 <= 1.25 else "FAIL"))
        if r2 > 1.25:
            fails.append("2 (el %d, %d masks: %.2f)" % (el, M, r2))
        print("#     gate 3: AUTO / faster forced form = %.2f (limit 1.25) -> %s" % (ratio, "ok" if ratio <= 1.25 else "FAIL"))
        if ratio > 1.25:
            fails.append("3 (el %d, %d masks: %.2f)" % (el, M, ratio))
    if el >= 20:
        headline(el, mz, L, torch, np, rng, stream)
    if fails:
        print("# gates failed: " + "; ".join(fails))
        sys.exit(1)


def headline(el, mz, L, torch, np, rng, stream):
    SZ, VP = ctypes.c_size_t, ctypes.c_void_p
    n, M = 1 << el, 256
    shifts = (el - 1 - np.arange(el)).astype(np.int64)
    te = np.concatenate([((rng.choice(n, size=M, replace=False).astype(np.int64)[:, None] >> shifts) & 1).astype(np.uint32) for _ in range(K)])
    tc = rng.integers(0, 1 << 62, size=(K * M, 4), dtype=np.int64).astype(np.uint64)
    tc[:, 3] &= np.uint64((1 << 60) - 1)
    toff = (ctypes.c_size_t * (K + 1))(*[f * M for f in range(K + 1)])
    _, total = mz.sumcheck_product_layout(el, K, D, 0)
    proof = torch.zeros(total, dtype=torch.uint8, device="cuda")
    sp = VP(stream.cuda_stream)
    host = rng.integers(0, 1 << 60, size=(K, n, 4), dtype=np.int64)
    dev = torch.empty((K, n, 4), dtype=torch.int64, device="cuda")

    def terms():
        rc = L.mzk_sumcheck_product_prove_terms_dev(tc.ctypes.data_as(VP), te.ctypes.data_as(VP), toff, SZ(K), SZ(el), SZ(D), None, SZ(0), SZ(0), VP(proof.data_ptr()),
                                                    SZ(total), sp)
        assert rc == 0, L.mzk_last_error()

    def uploaded():
        dev.copy_(torch.from_numpy(host))
        rc = L.mzk_sumcheck_product_prove_dev(VP(dev.data_ptr()), SZ(el), SZ(K), SZ(D), None, SZ(0), SZ(0), VP(proof.data_ptr()), SZ(total), sp)
        assert rc == 0, L.mzk_last_error()
    out = []
    for fn in (terms, uploaded):
        t = []
        for it in range(2 + 9):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            stream.synchronize()
            if it >= 2:
                t.append((time.perf_counter() - t0) * 1e3)
        out.append(statistics.median(t))
    print("# headline, el = %d, k = d = %d, 256 terms per factor, median of 9, host clock: prove_terms_dev %.3f ms; tables of %d bytes copied from "
          "pageable host memory + prove_dev %.3f ms; ratio %.2f" % (el, K, out[0], K * n * 32, out[1], out[1] / out[0]))


def main():
    if "--el" in sys.argv:
        run_el(int(sys.argv[sys.argv.index("--el") + 1]))
        return
    max_el = int(sys.argv[sys.argv.index("--max-el") + 1]) if "--max-el" in sys.argv else 24
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "hypercube_time.txt")
    rc = 0
    with open(path, "w") as out:
        def say(s):
            print(s, end="")
            out.write(s)
            out.flush()
        say("tools/timing/hypercube_time.py on one MI355X: mzk_mpoly_hypercube_evals_dev, k = %d, median of %d calls (%d from 2^20 masks up) after %d; ms\n"
            % (K, REPS, REPS_LARGE, WARM))
        for el in [e for e in (16, 20, 24) if e <= max_el]:
            try:
                r = subprocess.run([sys.executable, "-u", os.path.abspath(__file__), "--el", str(el)], capture_output=True, text=True, timeout=LIMIT[el])
            except subprocess.TimeoutExpired as e:
                say((e.stdout or b"").decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
                say("# el = %d: stopped at its time limit of %d s; nothing further was run\n" % (el, LIMIT[el]))
                sys.exit(2)
            say(r.stdout)
            if r.returncode not in (0, 1):
                say("# el = %d: the child ended with status %d; nothing further was run\n%s\n" % (el, r.returncode, r.stderr[-2000:]))
                sys.exit(2)
            rc |= r.returncode
    sys.exit(rc)


if __name__ == "__main__":
    main()
