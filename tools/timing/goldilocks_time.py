"""Times the Goldilocks kernels next to the M128 transform on one MI355X and writes profiles/goldilocks_time.txt.

    hipcc --offload-arch=gfx950 -O3 -o tools/microbench/copy_bw tools/microbench/copy_bw.hip      (once, where hipcc is)
    python tools/timing/goldilocks_time.py [--out profiles/goldilocks_time.txt] [--reps 50] [--warmup 5]

One GPU visit, two steps, each a child process under its own time limit, the second only if the first succeeded:
  1. tools/microbench/copy_bw (prebuilt): the copy rate of this box, the yardstick of the transform rows;
  2. this file with --measure: in ONE process, device-resident (hipEvent pairs around single calls, warm-up, median of --reps):
       forward NTT over M64, M64X3 and M128 at 2^16, 2^20, 2^24; coset LDE 2^18 -> 2^20, fold at 2^20, Merkle commit at 2^20 and the
       FRI commit loop (host callback included) at 2^16 for the two Goldilocks ids; FRI::prove at 2^16 and 2^20 (expansion 4, 17 tests)
       as one call (mzk_fri_prove_gl_dev) and as the composition it replaces (commit with a host callback, leaves, open_multi).
A transform row reports (bytes in + bytes out) / time as a fraction of the copy rate -- the HBM-roofline figure of a kernel that would
read and write the data once; the transform makes two to three passes, which is what the fraction shows.
Gates (exit status 1 when missed): the M64 transform is not slower than the M128 transform at 2^20 and at 2^24 in this run; the
one-call prover is not slower than the composed form (the same kernels minus one host round trip per round).
The M64X3 : M64 ratio is reported against the 3 that the work count predicts, without a threshold."""
import argparse, ctypes, os, re, statistics, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
COPY_BW = os.path.join(ROOT, "tools", "microbench", "copy_bw")
M128, M64, M64X3 = 1, 3, 4
NAMES = {M128: "M128", M64: "M64", M64X3: "M64X3"}


def measure(reps, warmup, copy_gbs):
    import numpy as np, torch
    import myzkp_amd as mz
    mz.init(0)
    L = mz.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream()
    st = ctypes.c_void_p(stream.cuda_stream)
    vp, SZ = ctypes.c_void_p, ctypes.c_size_t
    P64 = mz.MODULUS[M64]

    def check(rc):
        if rc != 0:
            raise RuntimeError(L.mzk_last_error().decode())

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts), min(ts)

    def device_elems(fid, n, seed):
        """n canonical elements in HBM: M128 from the library's generator, Goldilocks words as random 63-bit values (all below p)"""
        nl = mz.LIMBS[fid]
        if fid == M128:
            t = torch.empty(n * nl, dtype=torch.int64, device=dev)
            check(L.mzk_synth_field_dev(fid, ctypes.c_uint64(seed), SZ(n), vp(t.data_ptr()), st))
            return t
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        return torch.randint(0, 1 << 62, (n * nl,), dtype=torch.int64, device=dev, generator=g)

    def limbs(fid, v):
        return mz.to_limbs([v], mz.LIMBS[fid])

    lines, ntt_ms, prove_ms = [], {}, {}
    EXPANSION, TESTS = 4, 17

    def prove_rows(fid, lg, cw):
        """mzk_fri_prove_gl_dev, and today's composition of the same proof: the commit loop with the transcript in a host callback (one
        round trip per round), the last codeword, the indices sampled on the host, then merkle_open_multi and the revealed leaves"""
        import hashlib
        n, nl = 1 << lg, mz.LIMBS[fid]
        w, off = mz.root_of_unity(fid, lg), 7
        wl, ol = limbs(fid, w), limbs(fid, off)
        R, _, total = mz.fri_proof_layout_gl(fid, n, EXPANSION, TESTS)
        proof = torch.empty(total, dtype=torch.uint8, device=dev)

        def one_call():
            check(L.mzk_fri_prove_gl_dev(fid, vp(cw.data_ptr()), SZ(n), vp(wl.ctypes.data), vp(ol.ctypes.data), SZ(EXPANSION), SZ(TESTS), vp(proof.data_ptr()),
                                         SZ(total), st))

        def u64le(x):
            return int(x).to_bytes(8, "little")

        def leaf(v):        # the base leaf of mzk.h: sign byte, digit count, u32 digits
            d = [v & 0xFFFFFFFF, v >> 32] if v >> 32 else ([v] if v else [])
            return bytes([1 if v else 0]) + u64le(len(d)) + b"".join(x.to_bytes(4, "little") for x in d)

        def elem_leaf(row):
            if nl == 1:
                return leaf(int(row[0]))
            k = 3
            while k and int(row[k - 1]) == 0:
                k -= 1
            return u64le(k) + b"".join(leaf(int(c)) for c in row[:k])

        def composed():
            stream = [b""]

            def challenge(rnd, last, root):
                stream[0] += u64le(1) + u64le(32) + root
                if last:
                    return None
                d = hashlib.shake_256(u64le(rnd + 1) + stream[0]).digest(32)
                return int.from_bytes(d[24:], "big") % P64
            _, _, trees = mz.fri_commit(fid, None, w, off, R, challenge, keep_trees=True, codewords=False, device_ptr=cw.data_ptr(), n=n)
            m = n >> (R - 1)
            last = trees[-1].leaves(list(range(m)))
            body = u64le(m) + b"".join(u64le(len(x)) + x for x in (elem_leaf(row) for row in last))
            seed = hashlib.shake_256(u64le(R + 1) + stream[0] + body).digest(32)
            top, seen, counter = [], set(), 0
            while len(top) < TESTS:
                h = hashlib.blake2b(seed + u64le(counter), digest_size=32).digest()
                idx = int.from_bytes(h[24:], "big") % (n // 2)
                counter += 1
                if idx % m not in seen:
                    seen.add(idx % m)
                    top.append(idx)
            lists = [[] for _ in range(R)]
            for i in range(R - 1):
                half_len = (n >> i) // 2
                a = [t % half_len for t in top]
                lists[i] += a + [x + half_len for x in a]
                lists[i + 1] += a
            mz.merkle_open_multi(trees, lists)
            for r in range(R):
                trees[r].leaves(lists[r])
            for t in trees:
                t.close()
        one, one_best = timed(one_call)
        comp, comp_best = timed(composed)
        lines.append("prove  %-5s 2^%-2d fri_prove_gl_dev, %d rounds            median %8.4f ms  best %8.4f ms" % (NAMES[fid], lg, R, one, one_best))
        lines.append("prove  %-5s 2^%-2d composed: commit (host callback), leaves, open_multi  median %8.4f ms  best %8.4f ms" %
                     (NAMES[fid], lg, comp, comp_best))
        return one, comp
    for lg in (16, 20, 24):
        n = 1 << lg
        for fid in (M64, M64X3, M128):
            src, dst = device_elems(fid, n, 5), torch.empty(n * mz.LIMBS[fid], dtype=torch.int64, device=dev)
            root = limbs(fid, mz.root_of_unity(fid, lg))
            med, best = timed(lambda: check(L.mzk_ntt_dev(fid, vp(root.ctypes.data), vp(src.data_ptr()), vp(dst.data_ptr()), SZ(n), 0, st)))
            ntt_ms[(fid, lg)] = med
            gbs = 2 * n * 8 * mz.LIMBS[fid] / (med * 1e-3) / 1e9
            lines.append("ntt    %-5s 2^%-2d  median %8.4f ms  best %8.4f ms  (in + out) / time %7.1f GB/s = %.3f of the copy rate" %
                         (NAMES[fid], lg, med, best, gbs, gbs / copy_gbs))
            del src, dst
    for fid in (M64, M64X3):
        nl = mz.LIMBS[fid]
        nc, order = 1 << 18, 1 << 20
        coef, out = device_elems(fid, nc, 6), torch.empty(order * nl, dtype=torch.int64, device=dev)
        off, gen = limbs(fid, 7), limbs(fid, mz.root_of_unity(fid, 20))
        med, best = timed(lambda: check(L.mzk_coset_lde_dev(fid, vp(coef.data_ptr()), SZ(nc), vp(off.ctypes.data), vp(gen.ctypes.data), vp(out.data_ptr()), SZ(order), st)))
        lines.append("lde    %-5s 2^18 -> 2^20  median %8.4f ms  best %8.4f ms" % (NAMES[fid], med, best))
        half = torch.empty(order // 2 * nl, dtype=torch.int64, device=dev)
        alpha = limbs(fid, 0x1234567 + (0x89abcdef << 64) * (nl == 3) + (0x13579bdf << 128) * (nl == 3))
        med, best = timed(lambda: check(L.mzk_fri_fold_dev(fid, vp(out.data_ptr()), SZ(order), vp(alpha.ctypes.data), vp(off.ctypes.data), vp(gen.ctypes.data), vp(half.data_ptr()), st)))
        lines.append("fold   %-5s 2^20          median %8.4f ms  best %8.4f ms" % (NAMES[fid], med, best))
        rootbuf, rl = (ctypes.c_uint8 * 64)(), SZ()
        med, best = timed(lambda: check(L.mzk_merkle_commit_field_dev(fid, vp(out.data_ptr()), SZ(order), rootbuf, SZ(64), ctypes.byref(rl), st)))
        lines.append("merkle %-5s 2^20 commit   median %8.4f ms  best %8.4f ms  (the call waits for the root)" % (NAMES[fid], med, best))
        n16 = 1 << 16
        cw = out[:n16 * nl]
        w16 = mz.root_of_unity(fid, 16)

        def commit():
            _, _, trees = mz.fri_commit(fid, None, w16, 7, 10, lambda rnd, last, root: (int.from_bytes(root[:8], "little") % P64), keep_trees=True,
                                        codewords=False, device_ptr=cw.data_ptr(), n=n16)
            for t in trees:
                if t is not None:
                    t.close()
        med, best = timed(commit)
        lines.append("fri    %-5s 2^16 commit loop, 10 rounds, trees kept  median %8.4f ms  best %8.4f ms  (host callback and handle release included)" %
                     (NAMES[fid], med, best))
        # FRI::prove in one enqueue next to the composed form it replaces, timed in the same run on the same codeword (the LDE above)
        for lg in (16, 20):
            n = 1 << lg
            prove_ms[(fid, lg)] = prove_rows(fid, lg, out[:n * nl])
        del coef, out, half
    ok = True
    for (fid, lg), (one, composed) in sorted(prove_ms.items()):
        verdict = "ok" if one <= composed else "MISSED"
        ok = ok and one <= composed
        lines.append("gate   prove %-5s 2^%d: one call %.4f ms <= composed %.4f ms: %s" % (NAMES[fid], lg, one, composed, verdict))
    for lg in (20, 24):
        a, b = ntt_ms[(M64, lg)], ntt_ms[(M128, lg)]
        verdict = "ok" if a <= b else "MISSED"
        ok = ok and a <= b
        lines.append("gate   2^%d: M64 %.4f ms <= M128 %.4f ms: %s" % (lg, a, b, verdict))
    for lg in (16, 20, 24):
        lines.append("ratio  2^%d: M64X3 : M64 = %.2f (work count: 3)" % (lg, ntt_ms[(M64X3, lg)] / ntt_ms[(M64, lg)]))
    print("\n".join(lines))
    return 0 if ok else 1


def sclk_mhz():
    try:
        import bench
        snap = bench.gpu_sysfs_snapshot()
        return {c: bench.sclk_now_mhz(c) for c in snap}
    except Exception as ex:      # noqa: BLE001
        return "unavailable (%s)" % ex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--measure", type=float, default=None, help="(child) run the measurements against this copy rate in GB/s")
    a = ap.parse_args()
    if a.reps < 50:
        ap.error("--reps: at least 50")
    if a.measure is not None:
        return measure(a.reps, a.warmup, a.measure)
    if not os.path.exists(COPY_BW):
        print("tools/microbench/copy_bw is missing: build it first (see the top of this file)")
        return 2
    head = ["tools/timing/goldilocks_time.py on one MI355X; median of %d single calls after %d warm-ups, hipEvent pairs; times in ms" % (a.reps, a.warmup)]
    try:
        head.append("commit %s" % subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown")
    except OSError:
        head.append("commit unknown")
    head.append("shader clock before the run (MHz per card): %s" % (sclk_mhz(),))
    cp = subprocess.run([COPY_BW], capture_output=True, text=True, timeout=180)
    if cp.returncode != 0:
        print(cp.stdout + cp.stderr)
        return cp.returncode or 1
    rates = [float(m.group(1)) for m in re.finditer(r"1024 MiB:\s*([0-9.]+) GB/s", cp.stdout)]
    copy_gbs = max(rates)
    head.append("copy rate (tools/microbench/copy_bw, best form at 1 GiB, read + write): %.1f GB/s" % copy_gbs)
    ms = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", str(copy_gbs), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                        capture_output=True, text=True, timeout=900)
    head.append("shader clock after the run (MHz per card): %s" % (sclk_mhz(),))
    text = "\n".join(head) + "\n\n" + ms.stdout + (("\n" + ms.stderr) if ms.returncode not in (0, 1) else "")
    print(text)
    if a.out and ms.returncode in (0, 1):
        with open(a.out, "w") as f:
            f.write(text)
    return ms.returncode


if __name__ == "__main__":
    sys.exit(main())
