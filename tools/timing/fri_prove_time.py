"""FRI::prove (fri.rs:99-143) of one M128 codeword, expansion factor 4 and 17 colinearity tests, at 2^14, 2^16 and 2^20: the one
call (mzk_fri_prove_dev: commit, proof stream, index sampling and query phase on the device, one synchronize) against the composed
form (mzk_fri_commit_keep_trees_dev with the real transcript in a Python challenge callback, then mzk_merkle_leaves for the last
codeword, Blake2b index sampling on the host and mzk_merkle_open_multi + mzk_merkle_leaves for the query phase).  Both start from the
codeword in HBM; best of 8 after 2 warm-up calls.  Prints one line per shape and checks that both forms give the same proof."""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import numpy as np, torch
import myzkp_amd as mz, orc
import fri_prove_model as fm

mz.init(0)
fid, p, EXP, TESTS = orc.M128, orc.MOD[orc.M128], 4, 17


def composed(d, n, omega):
    R = fm.num_rounds(n, EXP, TESTS)
    stream = []

    def challenge(rnd, last, rt):
        stream.append([rt])
        return None if last else fm.sample(fm.fiat_shamir(stream)) % p

    _, roots, trees = mz.fri_commit(fid, None, omega, orc.M128_GEN, R, challenge, keep_trees=True, codewords=False, device_ptr=d.data_ptr(), n=n)
    m = n >> (R - 1)
    last = trees[-1].leaves(list(range(m)))
    stream.append([fm.leaf(v) for v in orc.from_limbs(last)])
    top = fm.sample_indices(fm.fiat_shamir(stream), n // 2, m, TESTS)
    wanted, vals = [[] for _ in range(R)], []
    for i in range(R - 1):
        half = (n >> i) // 2
        a = [t % half for t in top]
        wanted[i] += a + [x + half for x in a]
        wanted[i + 1] += a
        vals.append(trees[i].leaves(a + [x + half for x in a]))
        vals.append(trees[i + 1].leaves(a))
    paths = mz.merkle_open_multi(trees, wanted)
    for t in trees:
        t.close()
    return roots, top, paths, vals


def main():
    for lg in (14, 16, 20):
        n = 1 << lg
        R = fm.num_rounds(n, EXP, TESTS)
        cw = orc.synth_vector(fid, lg, n)
        d = torch.from_numpy(cw.view(np.int64).reshape(-1).copy()).to("cuda:0")
        omega = orc.root_of(fid, lg)
        one_t, comp_t = [], []
        for it in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            proof = mz.fri_prove(fid, None, omega, orc.M128_GEN, EXP, TESTS, device_ptr=d.data_ptr(), n=n)
            one_t.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            roots, top, _, _ = composed(d, n, omega)
            comp_t.append((time.perf_counter() - t0) * 1e3)
            assert roots == proof["merkle_roots"] and top == proof["top_level_indices"]
        one, comp = min(one_t[2:]), min(comp_t[2:])
        print("2^%d, %d rounds: one call %.3f ms (%.1f us per round), composed %.3f ms (%.1f us per round), ratio %.2f"
              % (lg, R, one, one * 1e3 / R, comp, comp * 1e3 / R, one / comp), flush=True)


if __name__ == "__main__":
    main()
