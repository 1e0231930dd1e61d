"""mzk_merkle_open_multi at the FRI query shape (2^14 M128 leaves, expansion 4, 8 colinearity tests: 9 round trees, three index lists per
layer) and mzk_merkle_open_batch of 64 indices of the 2^14-leaf tree, at the C boundary: median of 200 calls after 20 warm-ups, twice.
One process per library (MZK_HIP_LIB names it); the last field is a hash of everything the calls wrote.
profiles/merkle_open_refactor_time.txt holds a parent / branch comparison made with it."""
import ctypes, os, sys, time
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import myzkp_amd as mz, orc
import fri_prove_model as fm
mz.init(0); L = mz.lib()
SZ = ctypes.c_size_t

def median_us(fn):
    for _ in range(20): fn()
    ts = []
    for _ in range(200):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e6

lg0, expansion, tests = 14, 4, 8
rounds = fm.num_rounds(1 << lg0, expansion, tests)
trees = [mz.MerkleTree(orc.M128, orc.synth_vector(orc.M128, 3 + r, 1 << (lg0 - r))) for r in range(rounds)]
rng = np.random.default_rng(7)
hs, lists = [], []
for r in range(rounds - 1):            # per layer: a and b in round r's tree, c in round r + 1's
    n = 1 << (lg0 - r)
    c = rng.integers(0, n // 2, tests).astype(np.uint64)
    hs += [trees[r], trees[r], trees[r + 1]]
    lists += [c, c + np.uint64(n // 2), c]
T = len(hs)
flat = np.ascontiguousarray(np.concatenate(lists))
handles = (ctypes.c_void_p * T)(*[t._h for t in hs]); cnt = (SZ * T)(*[tests] * T); depths = (SZ * T)()
entries = sum(tests * (t.n.bit_length() - 1) for t in hs)
buf = np.zeros(48 * entries, dtype=np.uint8); lens = np.zeros(entries, dtype=np.uint64)
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
def multi():
    assert L.mzk_merkle_open_multi(handles, SZ(T), P(flat), cnt, P(buf), SZ(48), P(lens), depths) == 0
idx = rng.integers(0, 1 << lg0, 64).astype(np.uint64)
bbuf = np.zeros(48 * 64 * lg0, dtype=np.uint8); blens = np.zeros(64 * lg0, dtype=np.uint64); d = SZ()
def batch():
    assert L.mzk_merkle_open_batch(trees[0]._h, P(idx), SZ(64), P(bbuf), SZ(48), P(blens), ctypes.byref(d)) == 0
m1, b1 = median_us(multi), median_us(batch)
m2, b2 = median_us(multi), median_us(batch)
import hashlib
print("lib %s rounds %d lists %d indices %d | open_multi %.1f / %.1f us | open_batch(64 of 2^14) %.1f / %.1f us | sha %s" % (
    os.environ.get("MZK_HIP_LIB", "tree"), rounds, T, flat.shape[0], m1, m2, b1, b2,
    hashlib.sha256(buf.tobytes() + lens.tobytes() + bbuf.tobytes() + blens.tobytes()).hexdigest()[:16]), flush=True)
