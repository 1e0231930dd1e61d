"""Rescue-Prime on the device (mzk_rescue_hash_dev / mzk_rescue_trace_dev) at the reference's parameters, one chain per lane.
    python tools/timing/rescue_time.py [out.txt]          (default profiles/rescue_time.txt)
Device rows are the median of 50 calls, each timed by a pair of device events on the stream the call is enqueued on, after 5 warm-up
calls of that shape; outputs are compared with the model (tests/rescue_cases.py) on a sample of lanes before anything is timed.
  * hash_dev and trace_dev for 2^10, 2^16 and 2^20 inputs: hashes/s, and M128 products/s from the plan's count (PRODUCTS_PER_HASH);
  * the ratio t(2^20) / t(2^16) against the ideal 16;
  * the yardstick, in the same session: the products/s of the term kernel of mzk_mpoly_compose_dev over the Rescue-Prime AIR at
    L = 2^18 (N = 2^20 points, 2 x 274 products per point), its time taken as the call's median minus the median of the call's
    transforms alone (tools/timing/mpoly_time.py measures the two the same way) -- the same product, independent per lane;
  * preimage -> proof for one input, wall clock, median of 7 after 2 warm-ups: input upload + trace_dev + prove_dev on one stream against
    the host-trace form of tools/timing/stark_prove_time.py (the model's trace in Python integers, uploaded, then prove_dev).
The tool reports and sets no gate: there is no earlier kernel to hold it against, and the ratios are to be read, not asserted."""
import ctypes, json, os, random, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import myzkp_amd as mz
import mpoly_model as mm
import rescue_cases as rc

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rescue_time.txt")
REPS, WARM = 50, 5
M, P = mz.FIELD_M128, rc.M128_P
mz.init(0)
L = mz.lib()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def sclk_mhz():
    try:
        import bench
        return {c: bench.sclk_now_mhz(c) for c in bench.gpu_sysfs_snapshot()}
    except Exception as ex:      # noqa: BLE001
        return "unavailable (%s)" % ex


def device_median(fn, reps=REPS, warm=WARM):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def limbs(vals):
    return mz.to_limbs([int(v) for v in vals], 2)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to(dev)


say("# tools/timing/rescue_time.py: medians of %d calls by device events; wall-clock rows say so" % REPS)
say("# device: %s; shader clock before the run (MHz per card): %s" % (torch.cuda.get_device_name(0), sclk_mhz()))
c = rc.BY_NAME["reference"]
h = mz.RescuePrime(M, c["m"], c["n"], c["alpha"], c["alphainv"], c["mds"], c["rc"])
plan = mz.rescue_plan(M, c["m"], c["n"], c["alpha"], c["alphainv"], 1 << 20)
per_hash = plan["products_per_hash"]
rows, m = c["n"] + 1, c["m"]
say("# parameters: m = %d, n_rounds = %d, alpha = %d (%d products), alphainv: %d products (binary %d); %d products per hash; grid cap %d workgroups of %d"
    % (m, c["n"], c["alpha"], plan["alpha_products"], plan["alphainv_products"], plan["alphainv_binary"], per_hash, plan["grid_cap"], plan["block"]))
t_hash = {}
for lg in (10, 16, 20):
    n = 1 << lg
    rng = np.random.default_rng(lg)
    a = np.empty((n, 2), dtype=np.uint64)
    a[:, 0] = rng.integers(0, 1 << 63, size=n, dtype=np.uint64)
    a[:, 1] = rng.integers(0, 0xcb80000000000000, size=n, dtype=np.uint64)
    d_in, d_out = to_dev(a), torch.zeros(n * 2, dtype=torch.int64, device=dev)
    d_tr = torch.zeros(n * rows * m * 2, dtype=torch.int64, device=dev)
    hash_ = lambda: h.hash_dev(d_in.data_ptr(), n, 1, d_out.data_ptr(), stream)
    trace = lambda: h.trace_dev(d_in.data_ptr(), n, 1, d_tr.data_ptr(), rows * m, d_out.data_ptr(), stream)
    sample = sorted({0, 1, 63, 64, n // 2, n - 65, n - 1})
    hash_(); torch.cuda.synchronize()
    got = d_out.cpu().numpy().view(np.uint64).reshape(n, 2)
    want = {i: rc.model_trace(c, mz.from_limbs(a[i:i + 1])[0]) for i in sample}
    assert all(mz.from_limbs(got[i:i + 1])[0] == want[i][-1][0] for i in sample), "hash_dev differs from the model"
    trace(); torch.cuda.synchronize()
    tr = d_tr.cpu().numpy().view(np.uint64).reshape(n, rows * m, 2)
    assert all(mz.from_limbs(tr[i]) == [v for row in want[i] for v in row] for i in sample), "trace_dev differs from the model"
    del tr, got
    th, tt = device_median(hash_), device_median(trace)
    t_hash[lg] = (th, tt)
    for name, t in (("hash_dev ", th), ("trace_dev", tt)):
        say("2^%-2d inputs  %s %10.3f ms  %12.0f hashes/s  %8.2f G M128 products/s" % (lg, name, t, n / t * 1e3, n * per_hash / t * 1e-6))
    del d_in, d_out, d_tr
    torch.cuda.empty_cache()
say("ratio t(2^20) / t(2^16): hash_dev %.2f, trace_dev %.2f (ideal 16)" % (t_hash[20][0] / t_hash[16][0], t_hash[20][1] / t_hash[16][1]))

# ---- the yardstick: the term kernel of mzk_mpoly_compose_dev over the Rescue-Prime AIR, L = 2^18 -----------------------------------------
rp = mm.RescuePrime(rc.golden())
cons = [mm.terms_of(x) for x in rp.transition_constraints(mm.m128_root(7))]
ln = 1 << 18
rnd = np.random.default_rng(1000 + ln + M)
point = [mz.to_limbs([0, 1], 2)]
for _ in range(4):
    q = rnd.integers(0, 1 << 63, size=(ln, 2), dtype=np.uint64)
    q[:, 1] >>= np.uint64(4)
    point.append(q)
lens = [q.shape[0] for q in point]
N, smin, _ = mz.mpoly_compose_plan(M, cons, lens)
d_pt = to_dev(np.concatenate(point))
d_o = torch.zeros(len(cons) * smin * 2, dtype=torch.int64, device=dev)
d_t = torch.zeros((len(lens) + len(cons)) * N * 2, dtype=torch.int64, device=dev)
root = mz.to_limbs([mz.root_of_unity(M, N.bit_length() - 1)], 2)
tc, te, toff = mz.mpoly_term_table(M, cons, len(lens))
poff = (ctypes.c_size_t * (len(lens) + 1))(*[sum(lens[:i]) for i in range(len(lens) + 1)])
out_lens = (ctypes.c_size_t * len(cons))()
vp = lambda x: x.ctypes.data_as(ctypes.c_void_p)
SZ, VP = ctypes.c_size_t, ctypes.c_void_p


def compose():
    assert L.mzk_mpoly_compose_dev(M, vp(tc), vp(te), toff, SZ(len(cons)), SZ(len(lens)), VP(d_pt.data_ptr()), poff, VP(d_o.data_ptr()), SZ(smin), out_lens, VP(stream)) == 0


def transforms():
    x, y = VP(d_t.data_ptr()), VP(d_t.data_ptr() + len(lens) * N * 16)
    assert L.mzk_ntt_batch_dev(M, vp(root), x, x, SZ(N), SZ(len(lens)), 0, VP(stream)) == 0
    assert L.mzk_ntt_batch_dev(M, vp(root), y, y, SZ(N), SZ(len(cons)), 1, VP(stream)) == 0


t_new, t_tr = device_median(compose, 20, 3), device_median(transforms, 20, 3)
PER_POINT = 2 * 274
say("mpoly_compose_dev, Rescue-Prime AIR, L = 2^18 (N = 2^%d): call %.3f ms, its transforms alone %.3f ms; the rest as the term kernel: %.2f G M128 products/s (%d per point)"
    % (N.bit_length() - 1, t_new, t_tr, N * PER_POINT / (t_new - t_tr) * 1e-6, PER_POINT))
say("ratio of the product rates, rescue hash_dev at 2^20 : term kernel = %.2f" % ((1 << 20) * per_hash / t_hash[20][0] / (N * PER_POINT / (t_new - t_tr))))
del d_pt, d_o, d_t

# ---- preimage -> proof for one input ---------------------------------------------------------------------------------------------------------
x0 = rc.CHAIN_INPUT
rnd = random.Random(rows)
with mz.Stark(M, 4, 2, m, rows, 2, mm.M128_GEN, cons) as st:
    tr0 = rp.trace(x0)
    boundary = [(0, 1, 0), (rp.n, 0, tr0[-1][0])]
    d = st.dims(boundary)
    rl = d["randomized_trace_length"]
    random_rows = [[rnd.randrange(P) for _ in range(m)] for _ in range(rl - rows)]
    randomizer = [rnd.randrange(P) for _ in range(d["randomizer_length"])]
    _, total = mz.stark_proof_layout(M, d)
    d_r = to_dev(limbs(randomizer))
    d_p, d_p2 = torch.zeros(total, dtype=torch.uint8, device=dev), torch.zeros(total, dtype=torch.uint8, device=dev)
    d_buf = to_dev(limbs([0] * (rows * m) + [v for row in random_rows for v in row]))       # the random rows already in place
    x_l = limbs([x0])

    def host_form():
        t = rp.trace(x0)
        d_t = to_dev(limbs([v for row in t + random_rows for v in row]))
        st.prove_dev(d_t.data_ptr(), rl, boundary, d_r.data_ptr(), d_p.data_ptr(), total, stream)

    def device_form():
        d_x = to_dev(x_l)
        h.trace_dev(d_x.data_ptr(), 1, 1, d_buf.data_ptr(), rl * m, None, stream)
        st.prove_dev(d_buf.data_ptr(), rl, boundary, d_r.data_ptr(), d_p2.data_ptr(), total, stream)

    def prove_only():
        st.prove_dev(d_buf.data_ptr(), rl, boundary, d_r.data_ptr(), d_p2.data_ptr(), total, stream)

    def wall(fn):
        ms = []
        for r in range(9):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if r >= 2:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms
    w_host, w_dev, w_prove = wall(host_form), wall(device_form), wall(prove_only)
    assert torch.equal(d_p, d_p2), "the two forms give different proofs"
    for name, v in (("host trace (Python integers) + upload + prove_dev", w_host), ("input upload + trace_dev + prove_dev, one stream", w_dev), ("prove_dev alone", w_prove)):
        say("preimage -> proof, one input, wall clock: %-52s min %8.3f  median %8.3f  max %8.3f ms (%d runs)" % (name, min(v), statistics.median(v), max(v), len(v)))
h.close()
say("# shader clock after the run (MHz per card): %s" % (sclk_mhz(),))
say("# no gate: the rows are to be read")
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote " + OUT)
