"""Celestia's commitment on the device: roots only, the handle form, 4096 openings, against the calls it replaces and a copy of the bytes.
    python tools/timing/das_time.py [out.txt]          (default profiles/das_time.txt)
Device rows are the median of 50 calls, each timed by a pair of device events on the stream the call is enqueued on, after 5 warm-up
calls of that shape.  Host rows (squares = 1) are the median of 50 wall-clock times from host buffers to host results: the one call
mzk_das_commit, and the composed form that was the only way before it -- rows + cols + 1 calls of mzk_merkle_commit_bytes, the column
calls behind a host transpose.  Roots of both forms are compared before anything is timed.
Gates, printed as met or MISSED: the one-call form is not slower than the composed form at any shape.  Reported without a gate: the time
per Keccak permutation at 255 x 255 x 256 against the time per hash of mzk_merkle_commit_field_dev over 2^25 M128 leaves in the same
run (2^25 - 1 hashes against 33.2 million permutations; a lane per hash at every level of that tree down from 2^24 nodes) -- the number that
says whether the in-LDS schedule keeps its lanes busy."""
import ctypes, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import myzkp_amd as mz

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "das_time.txt")
REPS, WARM, OPENINGS = 50, 5, 4096
SIDES, COUNTS = (16, 64, 128, 255), (1, 16, 256)

mz.init(0)
L = mz.lib()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
st = ctypes.c_void_p(stream)
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


def device_median(fn, after=None):
    for _ in range(WARM):
        fn()
        if after:
            after()
    torch.cuda.synchronize()
    ms = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        if after:
            after()
    return statistics.median(ms)


def host_median(fn):
    for _ in range(2):
        fn()
    ms = []
    for _ in range(REPS):
        t = time.perf_counter(); fn(); ms.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ms)


def composed(m):
    """Celestia::commit through mzk_merkle_commit_bytes: one call per row, per column (host transpose first) and for the data root"""
    rows, cols = m.shape
    root, n = np.zeros(32, dtype=np.uint8), ctypes.c_size_t(0)

    def one(leaves, off):
        assert L.mzk_merkle_commit_bytes(leaves.ctypes.data_as(ctypes.c_void_p), off.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(len(off) - 1),
                                         root.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(32), ctypes.byref(n)) == 0
        return root.copy()
    off_r, off_c = np.arange(cols + 1, dtype=np.uint64), np.arange(rows + 1, dtype=np.uint64)
    rr = [one(m[r], off_r) for r in range(rows)]
    t = np.ascontiguousarray(m.T)
    cr = [one(t[c], off_c) for c in range(cols)]
    both = np.concatenate(rr + cr)
    return rr, cr, one(both, (32 * np.arange(rows + cols + 1)).astype(np.uint64))


say("# tools/timing/das_time.py: medians of %d calls; device rows by device events, host rows by wall clock" % REPS)
say("# shader clock before the run (MHz per card): %s" % (sclk_mhz(),))
gates_ok = True
per_perm_ns = None
for side in SIDES:
    for count in COUNTS:
        g = torch.Generator(device=dev); g.manual_seed(side * 1000 + count)
        code = torch.randint(0, 256, (count, side, side), dtype=torch.uint8, device=dev, generator=g)
        rr = torch.zeros(count * side * 32, dtype=torch.uint8, device=dev); cr = torch.zeros_like(rr)
        dr = torch.zeros(count * 32, dtype=torch.uint8, device=dev)
        nbytes = (count * side * side + 15) // 16 * 16
        src = torch.zeros(nbytes // 8 + 2, dtype=torch.int64, device=dev); dst = torch.zeros_like(src)
        perms = count * 2 * side * (side - 1)
        commit = lambda: mz.das_commit_dev(code.data_ptr(), side, side, side, side * side, count, rr.data_ptr(), cr.data_ptr(), dr.data_ptr(), stream)
        held = []
        build = lambda: held.append(mz.DasGrid.from_device(code.data_ptr(), side, side, side, side * side, count, stream))
        drop = lambda: held.pop().close()
        copy = lambda: L.mzk_selftest_copy_dev(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), ctypes.c_size_t(nbytes), st)
        t_commit, t_build, t_copy = device_median(commit), device_median(build, drop), device_median(copy)
        grid = mz.DasGrid.from_device(code.data_ptr(), side, side, side, side * side, count, stream)
        pos = torch.stack([torch.randint(0, count, (OPENINGS,), device=dev, generator=g), torch.randint(0, side, (OPENINGS,), device=dev, generator=g),
                           torch.randint(0, side, (OPENINGS,), device=dev, generator=g), torch.randint(0, 2, (OPENINGS,), device=dev, generator=g)], dim=1).contiguous()
        paths = torch.zeros(OPENINGS * 256, dtype=torch.uint8, device=dev); lens = torch.zeros(OPENINGS * 8, dtype=torch.uint8, device=dev)
        deps = torch.zeros(OPENINGS, dtype=torch.uint8, device=dev); leafs = torch.zeros_like(deps)
        t_open = device_median(lambda: grid.open_dev(pos.data_ptr(), OPENINGS, paths.data_ptr(), lens.data_ptr(), deps.data_ptr(), leafs.data_ptr(), stream))
        torch.cuda.synchronize()
        assert torch.equal(torch.from_numpy(grid.roots()[2].reshape(-1)).to(dev), dr)
        grid.close()
        say("%3d x %3d x %-3d  commit %8.3f ms  (%6.2f ns per permutation)  | handle build %8.3f ms | %d openings %7.3f ms | copy of the bytes %7.3f ms"
            % (side, side, count, t_commit, t_commit * 1e6 / perms, t_build, OPENINGS, t_open, t_copy))
        if (side, count) == (255, 256):
            per_perm_ns = t_commit * 1e6 / perms
        if count == 1:
            m = code[0].cpu().numpy()
            one = mz.das_commit(m)
            old = composed(m)
            assert [bytes(x) for x in one[0][0]] == [bytes(x) for x in old[0]] and [bytes(x) for x in one[1][0]] == [bytes(x) for x in old[1]] and bytes(one[2][0]) == bytes(old[2])
            t_one, t_old = host_median(lambda: mz.das_commit(m)), host_median(lambda: composed(m))
            ok = t_one <= t_old
            gates_ok = gates_ok and ok
            say("                  host buffers: one call %8.3f ms | %d calls of mzk_merkle_commit_bytes %9.3f ms | %6.1fx | gate (one call not slower): %s"
                % (t_one, 2 * side + 1, t_old, t_old / t_one, "met" if ok else "MISSED"))
        del code, rr, cr, dr, src, dst
        torch.cuda.empty_cache()

# the Merkle tree kernels at an equal number of hashes: 2^25 M128 leaves, one tree
n = 1 << 25
elems = torch.zeros(n * 2, dtype=torch.int64, device=dev)
assert L.mzk_synth_field_dev(mz.FIELD_M128, ctypes.c_uint64(3), ctypes.c_size_t(n), ctypes.c_void_p(elems.data_ptr()), st) == 0
root, rl = np.zeros(48, dtype=np.uint8), ctypes.c_size_t(0)
tree = lambda: L.mzk_merkle_commit_field_dev(mz.FIELD_M128, ctypes.c_void_p(elems.data_ptr()), ctypes.c_size_t(n), root.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(48),
                                             ctypes.byref(rl), st)
assert tree() == 0, L.mzk_last_error()
t_tree = device_median(tree)
per_hash_ns = t_tree * 1e6 / (n - 1)
say("merkle commit of 2^25 M128 leaves: %8.3f ms  (%6.2f ns per hash, %d hashes)" % (t_tree, per_hash_ns, n - 1))
say("ratio: das permutation at 255 x 255 x 256 : merkle hash = %.2f (reported, no gate)" % (per_perm_ns / per_hash_ns))
say("# shader clock after the run (MHz per card): %s" % (sclk_mhz(),))
say("# gates: %s" % ("all met" if gates_ok else "MISSED"))
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote " + OUT)
sys.exit(0 if gates_ok else 1)
