"""FastStark::prove on M128: the one call against the stage-by-stage form, identical proofs checked.
  A  Stark.prove_dev (mzk_stark_prove_dev): trace, randomizer and proof in HBM, wall time around a call that ends synchronised.
  B  the same proof from the entry points that existed BEFORE the one call, the two quotient stages and the plan: run this mode with
     MZK_HIP_LIB pointing at a build of that earlier library.  Boundary quotients on the host (Python integers, where that library leaves
     them), transition quotients through mzk_fast_coset_divide row by row, everything else through the HOST-BUFFER forms of the stages
     -- so B carries PCIe copies a device-pointer composition of the same stages would not; it is an upper bound of that composition, and is
     reported with and without the host boundary stage.
Workloads: the two-register AIR next0 = prev0^2 + prev1, next1 = prev0 prev1 + X at T = 2000 / 30000 / 120000 with 17 colinearity checks,
expansion 4, and Rescue-Prime at the reference's parameters.  2 warm-ups, 7 runs, median and spread.  Each mode writes the SHA3 of its
proofs; mode B compares them with mode A's file and says so.
    python tools/timing/stark_prove_time.py A out.json                      # then, against the earlier build:
    MZK_HIP_LIB=... python tools/timing/stark_prove_time.py B out.json
    python tools/timing/stark_prove_time.py trace 30000                     # three calls of A at one size, for a kernel / copy trace"""
import sys, os, time, json, random, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch, orc, myzkp_amd as mz
import mpoly_model as mm, fri_prove_model as fm, stark_model as sm
mz.init(0)
M = mz.FIELD_M128
P = mm.M128_P
G = mm.M128_GEN
WARM, RUNS = 2, 7


def workloads(sizes):
    out = []
    for T in sizes:
        if T == 0:                       # Rescue-Prime, the reference's test
            with open(os.path.join(ROOT, "tests", "golden", "rescue_prime_m128.json")) as f:
                rp = mm.RescuePrime(json.load(f))
            tr = rp.trace(123456789)
            cons = [mm.terms_of(a) for a in rp.transition_constraints(mm.m128_root(7))]
            out.append(("rescue-prime", 4, 2, rp.m, rp.n + 1, cons, [list(r) for r in tr], [(0, 1, 0), (rp.n, 0, tr[-1][0])]))
            continue
        lg = ((T + 68) * 2).bit_length()
        omicron = mm.m128_root(lg)
        rows, x = [[3, 4]], 1
        for _ in range(T - 1):
            u, v = rows[-1]
            rows.append([(u * u + v) % P, (u * v + x) % P])
            x = x * omicron % P
        cons = [[(1, (0, 0, 0, 1, 0)), (P - 1, (0, 2, 0, 0, 0)), (P - 1, (0, 0, 1, 0, 0))], [(1, (0, 0, 0, 0, 1)), (P - 1, (0, 1, 1, 0, 0)), (P - 1, (1, 0, 0, 0, 0))]]
        out.append(("T=%d" % T, 4, 17, 2, T, cons, rows, [(0, 0, 3), (0, 1, 4), (T - 1, 0, rows[-1][0])]))
    return out


def staged(e, checks, m, cycles, cons, trace, boundary, randomizer, clock):
    """the stage-by-stage form; clock[name] accumulates the host boundary stage's seconds"""
    L = lambda v: orc.to_limbs([int(a) for a in v], 2)
    rl = len(trace)
    lg = (rl * 2).bit_length()
    olen, flen = 1 << lg, (1 << lg) * e
    omicron, omega = mm.m128_root(lg), mm.m128_root(lg + (e.bit_length() - 1))
    tps = mz.fast_interpolate_batch(M, L([pow(omicron, i, P) for i in range(rl)]), np.stack([L([row[s] for row in trace]) for s in range(m)]), omicron, olen)
    t0 = time.perf_counter()
    roots = [[pow(omicron, c, P) for c, r, _ in boundary if r == s] for s in range(m)]
    bqs = [L(sm.div_roots(orc.from_limbs(tp), roots[s], P)) for s, tp in enumerate(tps)]
    clock["host boundary"] = clock.get("host boundary", 0.0) + time.perf_counter() - t0
    codewords = [mz.coset_lde(M, q, G, omega, flen) for q in bqs]
    proof = {"bqc_roots": [bytes(mz.merkle_commit_field(M, cw)) for cw in codewords]}
    point = [L([0, 1])] + list(tps) + [mz.poly_scale(M, q, omicron) for q in tps]
    tpolys = mz.mpoly_compose(M, cons, point)
    tz = mz.fast_zerofier(M, L([pow(omicron, i, P) for i in range(cycles - 1)]), omicron, olen)
    tqs = [mz.fast_coset_divide(M, tp, tz, G, omicron, olen) for tp in tpolys]
    r_cw = mz.coset_lde(M, L(randomizer), G, omega, flen)
    proof["rdc_root"] = bytes(mz.merkle_commit_field(M, r_cw))
    pd = [1] + [rl - 1] * (2 * m)
    tqdb = [max(sum(a * b for a, b in zip(pd, k)) for _, k in terms) - (cycles - 1) for terms in cons]
    max_degree = (1 << len(format(max(tqdb), "b"))) - 1
    weights = sm.sample_weights(1 + 2 * len(cons) + 2 * m, fm.fiat_shamir([[r] for r in proof["bqc_roots"]] + [[proof["rdc_root"]]]), P)
    polys, shifts = [L(randomizer)], [0]
    for a, q in enumerate(tqs):
        polys += [q, q]; shifts += [0, max_degree - tqdb[a]]
    for s, q in enumerate(bqs):
        polys += [q, q]; shifts += [0, max_degree - (rl - 1 - len(roots[s]))]
    comb = mz.poly_lincomb(M, polys, weights, shifts)
    fri = mz.fri_prove(M, mz.coset_lde(M, comb, G, omega, flen), omega, G, e, checks)
    fri["last_codeword"] = orc.from_limbs(fri["last_codeword"])
    fri["top_level_indices"] = sorted(fri["top_level_indices"])
    dup = list(fri["top_level_indices"]) + [(i + e) % flen for i in fri["top_level_indices"]]
    dup = sorted(dup + [(i + flen // 2) % flen for i in dup])
    all_cw = codewords + [r_cw, mz.coset_lde(M, tz, G, omega, flen)]
    paths = mz.merkle_open_multi([mz.MerkleTree(M, cw) for cw in all_cw], [dup] * (m + 2))
    pts = [orc.from_limbs(cw[dup]) for cw in all_cw]
    proof.update({"fri": fri, "bqc_points": [v for s in range(m) for v in pts[s]], "bqc_paths": [q for s in range(m) for q in paths[s]],
                  "rdc_points": pts[m], "rdc_paths": paths[m], "tzc_points": pts[m + 1], "tzc_paths": paths[m + 1]})
    return proof


def line(name, v, note=""):
    print("  %-22s min %8.3f  median %8.3f  max %8.3f ms (%d runs)   %s" % (name, min(v), statistics.median(v), max(v), len(v), note), flush=True)


def main():
    mode = sys.argv[1]
    if mode == "trace":
        sizes, path = [int(sys.argv[2])], None
    else:
        sizes, path = [0, 2000, 30000, 120000], sys.argv[2]
    print("mode %s, library %s, device %s" % (mode, os.environ.get("MZK_HIP_LIB", "the tree's own"), torch.cuda.get_device_name(0)), flush=True)
    digests = {}
    for name, e, checks, m, cycles, cons, rows, boundary in workloads(sizes):
        rnd = random.Random(cycles)
        trace = rows + [[rnd.randrange(P) for _ in range(m)] for _ in range(4 * checks)]
        if mode in ("A", "trace"):
            with mz.Stark(M, e, checks, m, cycles, 2, G, cons) as st:
                d = st.dims(boundary)
                randomizer = [rnd.randrange(P) for _ in range(d["randomizer_length"])]
                _, total = mz.stark_proof_layout(M, d)
                to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).cuda()
                d_t = to_dev(orc.to_limbs([v for row in trace for v in row], 2))
                d_r = to_dev(orc.to_limbs(randomizer, 2))
                d_p = torch.zeros(total, dtype=torch.uint8, device="cuda")
                ms = []
                for r in range((WARM + RUNS) if mode == "A" else 3):
                    torch.cuda.synchronize(); t0 = time.perf_counter()
                    st.prove_dev(d_t.data_ptr(), len(trace), boundary, d_r.data_ptr(), d_p.data_ptr(), total, 0)
                    torch.cuda.synchronize()
                    if r >= WARM or mode == "trace":
                        ms.append((time.perf_counter() - t0) * 1e3)
                raw = d_p.cpu().numpy().tobytes()
                proof = mz.stark_unpack_proof(M, d, raw)
                proof.pop("indices")
                digests[name] = sm.proof_digest(proof)
                print("%s: omicron domain %d, FRI domain %d, proof %d bytes" % (name, d["omicron_domain_length"], d["fri_domain_length"], total), flush=True)
                line("A prove_dev", ms)
        else:
            pd = [1] + [len(trace) - 1] * (2 * m)
            tq = max(max(sum(a * b for a, b in zip(pd, k)) for _, k in terms) for terms in cons) - (cycles - 1)
            randomizer = [rnd.randrange(P) for _ in range(1 << len(format(tq, "b")))]
            ms, host = [], []
            for r in range(WARM + RUNS):
                clock = {}
                torch.cuda.synchronize(); t0 = time.perf_counter()
                proof = staged(e, checks, m, cycles, cons, trace, boundary, randomizer, clock)
                torch.cuda.synchronize()
                if r >= WARM:
                    ms.append((time.perf_counter() - t0) * 1e3); host.append(clock["host boundary"] * 1e3)
            digests[name] = sm.proof_digest(proof)
            print("%s:" % name, flush=True)
            line("B stage by stage", ms)
            line("  its host boundary", host)
            line("B without that stage", [a - b for a, b in zip(ms, host)])
    if path and mode == "A":
        json.dump(digests, open(path, "w"))
    if path and mode == "B":
        want = json.load(open(path))
        print("proofs identical to mode A's: %s" % {k: want.get(k) == v for k, v in digests.items()}, flush=True)


main()
