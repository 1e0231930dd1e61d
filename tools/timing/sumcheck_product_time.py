"""The product sum-check in one call (mzk_sumcheck_product_prove_dev) at el = 8, 16, 20, 24 with k = d = 3, tables in HBM, no header.

Per shape, after 3 warm-up calls, the median of 9 calls of: the whole proof (host clock around enqueue + synchronize), and -- from the
library's event pairs (mzk_prof_*: MZK_PH_SCP_*), in a separate set of 9 calls so that the events do not price the first figure --
round 0's kernel, the later round kernels, the round-end (transcript) kernels and the tail, each summed over the proof.  Also the
launch count, round 0's achieved bytes/s against the issue's traffic bound k * 32 * (n + n/2) bytes (round 0 itself reads k * 32 * n
and writes nothing), and at the largest shape a device-to-device copy of the tables' bytes timed the same way.

Two gates, both against figures of the same run (exit status 1 if one fails):
  A  at el = 24, round 0 takes at most MARGIN_COPY x the device-to-device copy of the same bytes;
  B  the tail's time per round is at most one grid round's kernel plus round-end time at the hand-over size (el = 8: one grid round
     of 128 index pairs, then the tail) -- otherwise the tail threshold is wrong.
Usage: python tools/timing/sumcheck_product_time.py [--max-el 24] > profiles/sumcheck_product_time.txt"""
import ctypes, os, statistics, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import numpy as np, torch
import myzkp_amd as mz

MARGIN_COPY = 2.0
K = D = 3
TAIL_LOG = 7
PH = {"round0": 13, "rounds": 14, "round_ends": 15, "tail": 16}
WARM, REPS = 3, 9


def tables_on_device(el):
    """k tables of 2^el canonical values: four random limbs, the top one below 2^60 (p's top limb is 0x30644e72e131a029)"""
    g = torch.Generator(device="cuda").manual_seed(el)
    t = torch.randint(0, 1 << 62, (K, 1 << el, 4), dtype=torch.int64, device="cuda", generator=g)
    t[:, :, 3] &= (1 << 60) - 1
    return t


def main():
    max_el = int(sys.argv[sys.argv.index("--max-el") + 1]) if "--max-el" in sys.argv else 24
    mz.init(0)
    L = mz.lib()
    SZ = ctypes.c_size_t
    stream = torch.cuda.current_stream()
    rows, gate_fail = {}, []
    print("# product sum-check, k = d = %d, no header; median of %d after %d warm-up calls; ms" % (K, REPS, WARM))
    print("# el  launches  whole    round0   rounds   round_ends  tail     round0 GB/s (bound %d*32*(n+n/2) bytes)" % K)
    for el in [e for e in (8, 16, 20, 24) if e <= max_el]:
        n = 1 << el
        t = tables_on_device(el)
        _, total = mz.sumcheck_product_layout(el, K, D, 0)
        proof = torch.zeros(total, dtype=torch.uint8, device="cuda")

        def call():
            rc = L.mzk_sumcheck_product_prove_dev(ctypes.c_void_p(t.data_ptr()), SZ(el), SZ(K), SZ(D), None, SZ(0), SZ(0), ctypes.c_void_p(proof.data_ptr()),
                                                  SZ(total), ctypes.c_void_p(stream.cuda_stream))
            assert rc == 0, L.mzk_last_error()
        whole = []
        for it in range(WARM + REPS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            stream.synchronize()
            if it >= WARM:
                whole.append((time.perf_counter() - t0) * 1e3)
        ph = {k: [] for k in PH}
        launches = 0
        for it in range(REPS):
            L.mzk_prof_reset()
            L.mzk_prof_enable(1)
            call()
            stream.synchronize()
            L.mzk_prof_enable(0)
            launches = 0
            for name, idx in PH.items():
                ms, cnt = ctypes.c_double(), ctypes.c_uint64()
                L.mzk_prof_read(idx, ctypes.byref(ms), ctypes.byref(cnt))
                ph[name].append(ms.value)
                launches += cnt.value
        L.mzk_prof_reset()
        med = {k: statistics.median(v) for k, v in ph.items()}
        assert launches == (2 * (el - TAIL_LOG) + 1 if el > TAIL_LOG else 1)
        gbs = K * 32 * (n + n // 2) / (med["round0"] * 1e-3) / 1e9 if med["round0"] else 0.0
        rows[el] = med
        print("  %2d  %8d  %7.3f  %7.3f  %7.3f  %10.3f  %7.3f  %8.1f" % (el, launches, statistics.median(whole), med["round0"], med["rounds"], med["round_ends"],
                                                                        med["tail"], gbs))
        if el == max_el and el >= 20:
            dst = torch.empty_like(t)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            copy = []
            for it in range(WARM + REPS):
                a.record()
                dst.copy_(t)
                b.record()
                b.synchronize()
                if it >= WARM:
                    copy.append(a.elapsed_time(b))
            c = statistics.median(copy)
            ratio = med["round0"] / c
            print("# gate A, el = %d: device-to-device copy of %d bytes %.3f ms; round 0 / copy = %.2f (margin %.1f) -> %s"
                  % (el, K * n * 32, c, ratio, MARGIN_COPY, "ok" if ratio <= MARGIN_COPY else "FAIL"))
            if ratio > MARGIN_COPY:
                gate_fail.append("A")
            del dst
        del t, proof
    if 8 in rows and 16 in rows:
        per_round = rows[16]["tail"] / TAIL_LOG
        grid = rows[8]["round0"] + rows[8]["round_ends"]
        print("# gate B: tail %.4f ms per round (el = 16, %d rounds in one launch); one grid round + round end at the hand-over size (el = 8) %.4f ms -> %s"
              % (per_round, TAIL_LOG, grid, "ok" if per_round <= grid else "FAIL"))
        if per_round > grid:
            gate_fail.append("B")
    if gate_fail:
        print("# gates failed: " + " ".join(gate_fail))
        sys.exit(1)


if __name__ == "__main__":
    main()
