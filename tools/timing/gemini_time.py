"""Gemini and the sum-check prover (algebra/gemini.rs, algebra/sumcheck.rs) at el = 12, 16 and 20 on a resident default-table SRS
handle of n + 1 powers.  Per size, best of 6 after 2 warm-up calls:
  split-fold      mzk_gemini_split_fold_dev, levels in HBM
  open (one call) mzk_gemini_open_srs_dev (evaluations, quotients, witness and degree-bound MSMs)
  open (composed) today's entry points per level: mzk_kzg_batch_open and mzk_kzg_prove_degree_bound on host powers, plus
                  mzk_kzg_commit_srs_dev per level for the commitments (the one-call figure adds mzk_gemini_commit_srs_dev to match)
  sum-check       mzk_sumcheck_prove_srs with a Python callback (the model transcript), and microseconds per round
Both open forms are checked equal.  `--sizes 12,16` picks sizes; `--prove-only` times the sum-check prove alone (for a kernel trace)."""
import ctypes, os, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, os.path.join(HERE, "..", "..", "tests"))
import numpy as np, torch
import myzkp_amd as mz, orc
import gemini_model as gm

mz.init(0)
L = mz.lib()


def dp(t):
    return ctypes.c_void_p(t.data_ptr())


def best(fn, reps=8):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return min(ts[2:]), out


def main():
    sizes = [12, 16, 20]
    if "--sizes" in sys.argv:
        sizes = [int(x) for x in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    prove_only = "--prove-only" in sys.argv
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for el in sizes:
        n = 1 << el
        alpha = 0x600D + el
        powers = mz.kzg_setup_g1(alpha, n)
        srs = mz.Srs(powers)
        coefs = orc.synth_vector(orc.FR, 40 + el, n)
        rhos = orc.from_limbs(orc.synth_vector(orc.FR, 41 + el, el))
        beta = orc.from_limbs(orc.synth_vector(orc.FR, 42 + el, 1))[0]
        if prove_only:
            h = gm.hypercube_sum_closed(orc.from_limbs(coefs))
            for _ in range(3):
                t0 = time.perf_counter()
                srs.sumcheck_prove(coefs, gm.ModelChallenge(el, h))
                print("el=%d: sum-check prove %.3f ms" % (el, (time.perf_counter() - t0) * 1e3), flush=True)
            srs.close()
            continue
        d_c = torch.from_numpy(coefs.view(np.int64).reshape(-1).copy()).cuda()
        d_l = torch.zeros((2 * n - 1) * 4, dtype=torch.int64, device="cuda")
        t_fold, _ = best(lambda: mz.gemini_split_fold_dev(d_c.data_ptr(), n, rhos, d_l.data_ptr(), st.value))
        levels = [l for l in mz._lib._levels_split(d_l.cpu().numpy().view(np.uint64).reshape(-1, 4), n)]
        d_cm = torch.zeros((el + 1) * 8, dtype=torch.int64, device="cuda")
        d_y = torch.zeros(el * 12, dtype=torch.int64, device="cuda")
        d_w = torch.zeros(el * 8, dtype=torch.int64, device="cuda")
        d_d = torch.zeros((el + 1) * 8, dtype=torch.int64, device="cuda")
        b = orc.to_limbs([beta], 4)

        def one():
            assert L.mzk_gemini_open_srs_dev(srs._h, dp(d_l), ctypes.c_size_t(n), orc.ptr(b), dp(d_y), dp(d_w), dp(d_d), st) == 0

        def one_with_commit():
            assert L.mzk_gemini_commit_srs_dev(srs._h, dp(d_l), ctypes.c_size_t(n), dp(d_cm), st) == 0
            one()
        t_open, _ = best(one)
        t_both, _ = best(one_with_commit)
        us = [beta, gm.neg(beta), beta * beta % gm.P]
        d_lv = [torch.from_numpy(l.view(np.int64).reshape(-1).copy()).cuda() for l in levels]

        def composed():
            out = []
            for i, l in enumerate(levels):
                assert L.mzk_kzg_commit_srs_dev(srs._h, dp(d_lv[i]), ctypes.c_size_t(l.shape[0]), dp(d_cm[8 * i:]), 0, st) == 0
            torch.cuda.synchronize()
            for i, l in enumerate(levels):
                if i < el:
                    out.append(mz.kzg_batch_open(l, us, powers))
                out.append(mz.kzg_prove_degree_bound(l, powers, l.shape[0]))
            return out
        t_comp, comp = best(composed, 4 if el >= 20 else 8)
        ys, ws, deg = srs.gemini_open(levels, beta)
        want = []
        for i in range(el + 1):
            if i < el:
                want.append((list(ys[i]), ws[i]))
            want.append(deg[i])
        assert comp == want, "composed and one-call opens differ"
        h = gm.hypercube_sum_closed(orc.from_limbs(coefs))
        ts = []
        for _ in range(4):
            cb = gm.ModelChallenge(el, h)
            t0 = time.perf_counter()
            srs.sumcheck_prove(coefs, cb)
            ts.append((time.perf_counter() - t0) * 1e3)
        t_sc = min(ts[1:])
        print("el=%d: split-fold %.3f ms | open one call %.3f ms, commit+open %.3f ms, composed commit+open %.3f ms (ratio %.2f) | "
              "sum-check prove %.3f ms (%.1f us per round incl. the Python callback)"
              % (el, t_fold, t_open, t_both, t_comp, t_both / t_comp, t_sc, (t_sc - t_both) * 1e3 / el), flush=True)
        srs.close()


if __name__ == "__main__":
    main()
