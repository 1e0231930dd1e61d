"""mzk_mpoly_compose_dev against the only way the library could produce the same polynomials before it, and against its own transforms.
Term structure: the two transition constraints of the Rescue-Prime AIR (2 x 272 terms, exponents up to [78, 3, 3, 3, 3];
tests/golden/rescue_prime_m128.json through tests/mpoly_model.py), over the point (X, four polynomials of L coefficients):
  m128 L=36       the reference's own shape (N = 128)
  m128 L=2^14, 2^16, 2^18     N = 2^16, 2^18, 2^20
  fr   L=2^14     the same exponents and coefficients read as Fr elements
Per shape, runs ALTERNATE inside this one process (new, transforms alone, term-by-term; new, ...), and min / median / max are printed:
  new         mzk_mpoly_compose_dev, point and result in HBM
  transforms  mzk_ntt_batch_dev of n_vars rows forward and n_constraints rows inverse at the same N: the floor of the new call
  term-by-term  the composition as it had to be written before: every power by square-and-multiply through mzk_fast_multiply
              (memoised per variable and exponent), every term the product of its factors through mzk_fast_multiply, the
              coefficient through mzk_poly_scale, the sum of the terms on the host (numpy limb arithmetic); checked equal to `new`.
              Only at the shapes listed in --parent-shapes (default 36,16384): it grows with 544 products of N points per run.
`--trace-only SHAPE` runs the new call five times at one shape and nothing else (for rocprofv3 --kernel-trace --stats)."""
import ctypes, json, os, statistics, sys, time
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import myzkp_amd as mz
import mpoly_model as mm

FR, M128 = 0, 1
NL = {FR: 4, M128: 2}
PRIME = {FR: mm.FR_P, M128: mm.M128_P}


def p_limbs(fid):
    return [(PRIME[fid] >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(NL[fid])]


def addmod(fid, a, b):
    """(a + b) mod p on (n, limbs) uint64 arrays, both canonical"""
    nl, pl = NL[fid], p_limbs(fid)
    n = max(a.shape[0], b.shape[0])
    x, y = np.zeros((n, nl), dtype=np.uint64), np.zeros((n, nl), dtype=np.uint64)
    x[:a.shape[0]], y[:b.shape[0]] = a, b
    out = np.empty_like(x)
    carry = np.zeros(n, dtype=bool)
    for j in range(nl):
        s = x[:, j] + y[:, j]
        c1 = s < x[:, j]
        s2 = s + carry.astype(np.uint64)
        carry = c1 | (s2 < s)
        out[:, j] = s2
    ge = np.ones(n, dtype=bool)                       # out >= p, limb by limb from the top
    decided = np.zeros(n, dtype=bool)
    for j in reversed(range(nl)):
        gt, lt = out[:, j] > np.uint64(pl[j]), out[:, j] < np.uint64(pl[j])
        ge = np.where(~decided & lt, False, ge)
        decided |= gt | lt
    sub = carry | ge
    borrow = np.zeros(n, dtype=bool)
    for j in range(nl):
        pj = np.uint64(pl[j])
        d = out[:, j] - pj
        b1 = out[:, j] < pj
        d2 = d - borrow.astype(np.uint64)
        b2 = d < borrow.astype(np.uint64)
        out[:, j] = np.where(sub, d2, out[:, j])
        borrow = b1 | b2
    return out


def trim(a):
    nz = np.nonzero(a.any(axis=1))[0]
    return a[:nz[-1] + 1] if nz.size else a[:0]


def np2(x):
    n = 1
    while n < x:
        n *= 2
    return n


class TermByTerm:
    """the composition through the entry points the library had before mzk_mpoly_compose"""
    def __init__(self, fid, point):
        self.fid, self.point, self.memo = fid, point, {}
        self.roots = {}

    def mul(self, a, b):
        if a.shape[0] == 0 or b.shape[0] == 0:
            return a[:0]
        order = max(np2(a.shape[0] + b.shape[0]), 16)
        if order not in self.roots:
            self.roots[order] = mz.root_of_unity(self.fid, order.bit_length() - 1)
        return trim(mz.fast_multiply(self.fid, a, b, self.roots[order], order))

    def power(self, i, e):
        if (i, e) not in self.memo:
            if e == 1:
                r = trim(self.point[i])
            elif e % 2:
                r = self.mul(self.power(i, e - 1), self.power(i, 1))
            else:
                h = self.power(i, e // 2)
                r = self.mul(h, h)
            self.memo[(i, e)] = r
        return self.memo[(i, e)]

    def constraint(self, terms):
        acc = np.zeros((0, NL[self.fid]), dtype=np.uint64)
        one = mz.to_limbs([1], NL[self.fid])
        for c, k in terms:
            prod = None
            for i, e in enumerate(k):
                if e:
                    f = self.power(i, e)
                    prod = f if prod is None else self.mul(prod, f)
            prod = one if prod is None else prod
            if prod.shape[0]:
                acc = addmod(self.fid, acc, mz.poly_scale(self.fid, prod, 1, lead=c))
        return trim(acc)


def stats(ts):
    return "min %.3f  median %.3f  max %.3f ms (%d runs)" % (min(ts), statistics.median(ts), max(ts), len(ts))


def main():
    mz.init(0)
    L = mz.lib()
    with open(os.path.join(ROOT, "tests", "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    cons = [mm.terms_of(a) for a in rp.transition_constraints(mm.m128_root(7))]
    shapes = [(M128, 36), (M128, 1 << 14), (M128, 1 << 16), (M128, 1 << 18), (FR, 1 << 14)]
    parent_shapes = [36, 1 << 14]
    if "--parent-shapes" in sys.argv:
        parent_shapes = [int(x) for x in sys.argv[sys.argv.index("--parent-shapes") + 1].split(",") if x]
    trace_only = None
    if "--trace-only" in sys.argv:
        fname, ln = sys.argv[sys.argv.index("--trace-only") + 1].split(":")
        trace_only = (FR if fname == "fr" else M128, int(ln))
        shapes = [trace_only]
    reps = 7
    st = torch.cuda.current_stream().cuda_stream
    print("time: %s (UTC %s)" % (time.strftime("%Y-%m-%d %H:%M:%S"), time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime())))
    print("device: %s" % torch.cuda.get_device_name(0))
    for fid, ln in shapes:
        nl = NL[fid]
        rnd = np.random.default_rng(1000 + ln + fid)
        point = [mz.to_limbs([0, 1], nl)]
        for _ in range(4):
            q = rnd.integers(0, 1 << 63, size=(ln, nl), dtype=np.uint64)
            q[:, nl - 1] >>= np.uint64(4)                           # below p
            point.append(q)
        lens = [q.shape[0] for q in point]
        n, smin, bounds = mz.mpoly_compose_plan(fid, cons, lens)
        d_in = torch.from_numpy(np.concatenate(point).view(np.int64).reshape(-1).copy()).cuda()
        d_out = torch.zeros(len(cons) * smin * nl, dtype=torch.int64, device="cuda")
        d_tr = torch.zeros((len(lens) + len(cons)) * n * nl, dtype=torch.int64, device="cuda")
        root = mz.to_limbs([mz.root_of_unity(fid, n.bit_length() - 1)], nl)
        rp_ = root.ctypes.data_as(ctypes.c_void_p)

        # the term table is marshalled once: a prover builds it once per AIR
        tc, te, toff = mz.mpoly_term_table(fid, cons, len(lens))
        poff = (ctypes.c_size_t * (len(lens) + 1))(*[sum(lens[:i]) for i in range(len(lens) + 1)])
        out_lens = (ctypes.c_size_t * len(cons))()
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)

        def new():
            rc = L.mzk_mpoly_compose_dev(fid, vp(tc), vp(te), toff, ctypes.c_size_t(len(cons)), ctypes.c_size_t(len(lens)), ctypes.c_void_p(d_in.data_ptr()), poff,
                                         ctypes.c_void_p(d_out.data_ptr()), ctypes.c_size_t(smin), out_lens, ctypes.c_void_p(st))
            assert rc == 0, L.mzk_last_error()
            return [int(x) for x in out_lens]

        def transforms():
            a, b = ctypes.c_void_p(d_tr.data_ptr()), ctypes.c_void_p(d_tr.data_ptr() + len(lens) * n * nl * 8)
            assert L.mzk_ntt_batch_dev(fid, rp_, a, a, ctypes.c_size_t(n), ctypes.c_size_t(len(lens)), 0, ctypes.c_void_p(st)) == 0
            assert L.mzk_ntt_batch_dev(fid, rp_, b, b, ctypes.c_size_t(n), ctypes.c_size_t(len(cons)), 1, ctypes.c_void_p(st)) == 0

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, r

        name = "%s L=%d N=%d (out_stride_min %d)" % ("fr" if fid == FR else "m128", ln, n, smin)
        if trace_only:
            for _ in range(5):
                print("%s: new %.3f ms" % (name, timed(new)[0]), flush=True)
            continue
        with_parent = ln in parent_shapes
        for _ in range(2):                                         # warm-up: plans, workspace
            new(); transforms()
        t_new, t_tr, t_par = [], [], []
        lens_out = None
        for r in range(reps):
            t, lens_out = timed(new)
            t_new.append(t)
            t_tr.append(timed(transforms)[0])
            if with_parent and r < 3:
                tb = TermByTerm(fid, point)                      # powers memoised across both constraints
                t, res = timed(lambda: [tb.constraint(c) for c in cons])
                t_par.append(t)
                rows = d_out.cpu().numpy().view(np.uint64).reshape(len(cons), smin, nl)
                assert all(np.array_equal(rows[a, :lens_out[a]], res[a]) and res[a].shape[0] == lens_out[a] for a in range(len(cons))), "term-by-term differs"
        print(name, flush=True)
        print("  new           %s   lengths %s" % (stats(t_new), lens_out))
        print("  transforms    %s   (%d forward + %d inverse rows)" % (stats(t_tr), len(lens), len(cons)))
        if t_par:
            print("  term-by-term  %s   checked equal; new is %.0fx faster by the medians" % (stats(t_par), statistics.median(t_par) / statistics.median(t_new)))
        else:
            print("  term-by-term  not run at this shape (see --parent-shapes)")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
