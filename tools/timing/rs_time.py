"""Reed-Solomon over GF(2^8) on the device against a plain copy of the same traffic: encode, encode + Fr columns, decode of clean words
and of words with t errors each.
    python tools/timing/rs_time.py [out.txt]          (default profiles/rs_time.txt)
Every row is the median of 50 calls, each timed by a pair of device events on the stream the call is enqueued on, after 5 warm-up
calls of that shape; the codec call and mzk_selftest_copy_dev alternate inside the same loop, so both see the same machine.  The copy
moves (bytes read + bytes written) / 2 bytes -- it reads and writes that much each, the same traffic as the call next to it.
Decoded messages are compared with the encoder's input before anything is timed."""
import ctypes, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
import myzkp_amd as mz

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "rs_time.txt")
REPS, WARM = 50, 5
SHAPES = [(16, 8, 1 << 16), (16, 8, 1 << 20), (16, 8, 1 << 22), (255, 223, 1 << 12), (255, 223, 1 << 16)]

mz.init(0)
L = mz.lib()
dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream().cuda_stream
st = ctypes.c_void_p(stream)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_pair(fn, copy_bytes, src, dst):
    """(median ms of fn, median ms of the copy of copy_bytes), alternating"""
    nb = (copy_bytes + 15) // 16 * 16
    cp = lambda: L.mzk_selftest_copy_dev(ctypes.c_void_p(src.data_ptr()), ctypes.c_void_p(dst.data_ptr()), ctypes.c_size_t(nb), st)
    for _ in range(WARM):
        fn(); assert cp() == 0, L.mzk_last_error()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(REPS)]
    for a, b, c in ev:
        a.record(); fn(); b.record(); cp(); c.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b, _ in ev), statistics.median(b.elapsed_time(c) for _, b, c in ev)


def row(what, n, k, batch, traffic, fn, src, dst):
    ms, cms = median_pair(fn, traffic // 2, src, dst)
    say("%-28s (%3d,%3d) x 2^%-2d  %8.3f ms  %7.1f GB/s of traffic | copy of the same traffic %8.3f ms | %5.2fx the copy"
        % (what, n, k, batch.bit_length() - 1, ms, traffic / ms / 1e6, cms, ms / cms))


say("# tools/timing/rs_time.py: medians of %d calls, device events; traffic = bytes read + bytes written by the call" % REPS)
for n, k, batch in SHAPES:
    t = (n - k) // 2
    g = torch.Generator(device=dev); g.manual_seed(n * 1000 + k)
    msgs = torch.randint(0, 256, (batch, k), dtype=torch.uint8, device=dev, generator=g)
    code = torch.zeros((batch, n), dtype=torch.uint8, device=dev)
    cols = torch.zeros(n * batch * 4, dtype=torch.int64, device=dev)
    back = torch.zeros((batch, k), dtype=torch.uint8, device=dev)
    status = torch.zeros(batch, dtype=torch.uint8, device=dev)
    big = n * batch * 32 // 2 + (n + k) * batch      # the largest copy below
    src = torch.zeros(big // 8 + 2, dtype=torch.int64, device=dev); dst = torch.zeros_like(src)
    enc = lambda: mz.rs_encode_dev(n, k, msgs.data_ptr(), batch, code.data_ptr(), None, stream)
    enc_cols = lambda: mz.rs_encode_dev(n, k, msgs.data_ptr(), batch, code.data_ptr(), cols.data_ptr(), stream)
    enc()
    # t errors in every codeword: t distinct positions, non-zero values
    bad = code.clone()
    pos = torch.rand((batch, n), device=dev, generator=g).topk(t, dim=1).indices
    val = torch.randint(1, 256, (batch, t), dtype=torch.uint8, device=dev, generator=g)
    bad.scatter_(1, pos, bad.gather(1, pos) ^ val)
    dec = lambda words: (lambda: mz.rs_decode_dev(n, k, words.data_ptr(), batch, None, back.data_ptr(), status.data_ptr(), stream))
    for words, want in ((code, 0), (bad, t)):
        dec(words)()
        torch.cuda.synchronize()
        assert torch.equal(back, msgs) and bool((status == want).all()), (n, k, batch, want)
    row("encode", n, k, batch, (k + n) * batch, enc, src, dst)
    if n == 16:
        row("encode + Fr columns", n, k, batch, (k + n + n + 32 * n) * batch, enc_cols, src, dst)
    row("decode, clean", n, k, batch, (n + k + 1) * batch, dec(code), src, dst)
    row("decode, %d errors per word" % t, n, k, batch, (n + k + 1) * batch, dec(bad), src, dst)
    del msgs, code, cols, back, status, src, dst, bad, pos, val
    torch.cuda.empty_cache()
os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote " + OUT)
