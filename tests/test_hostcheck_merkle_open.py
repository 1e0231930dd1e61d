"""The host half of opening field-element Merkle trees (myzkp_amd/csrc/mzk_merkle_open_plan.h: where each tree's share of the gather
scratch and of paths / path_lens lies, host_leaf, and the unpack of what k_merkle_gather_batch leaves) run without a GPU by
tests/hostcheck/merkle_open_shim.cpp, a stand-alone program with its own main that links nothing of the library: built once plain and
once with -fsanitize=address,undefined.  The vectors written here stand in for the kernel: per opened index the sibling digests of
levels 1 .. depth - 1 cut from merkle_model.nodes and the sibling element's raw limbs, in the order the kernel writes them.  The unpack
must leave merkle_model.expected_open in a buffer pre-filled with 0xA5, byte for byte: the bytes behind an entry's length stay 0xA5.
CPU only."""
import os, subprocess
import numpy as np
import merkle_model as mm

HERE = os.path.dirname(os.path.abspath(__file__))
E_LENGTH = -5
NAMES = {mm.FR: "Fr", mm.M128: "M128", mm.M64: "M64", mm.M64X3: "M64X3"}


def _hex(a):
    b = np.ascontiguousarray(a).tobytes()
    return b.hex() or "-"


class Tree:
    """the leaf vector of n elements of field fid, its digests by the model and its leaf lengths"""
    def __init__(self, fid, n, signed=False, seed=5):
        self.fid, self.n, self.depth = fid, n, n.bit_length() - 1
        self.arr, self.neg = mm.signed_vector(fid, n, seed + n) if signed else (mm.leaf_vector(fid, n, seed + n), None)
        blob, off = mm.leaves(fid, self.arr, self.neg)
        self.nd = mm.nodes(blob, off)
        self.leaf_len = np.diff(off)

    def gathered(self, idx):
        """(digests, sibling limbs) as block q of k_merkle_gather_batch writes them for idx[q]"""
        idx = np.asarray(idx, dtype=np.int64)
        dig = np.zeros((idx.shape[0], self.depth - 1, 32), dtype=np.uint8)
        for l in range(1, self.depth):
            dig[:, l - 1] = self.nd[mm.level_start(self.n, l) + ((idx >> l) ^ 1)]
        return dig, np.ascontiguousarray(self.arr[idx ^ 1], dtype="<u8")

    def expected(self, idx, stride):
        """(paths (count * depth, stride) on a 0xA5 background, path_lens (count * depth,)) by the model"""
        wide = max(stride, 64)
        paths, lens = mm.expected_open(self.fid, self.arr, self.nd, idx, wide, self.neg)
        paths, lens = paths.reshape(-1, wide), lens.reshape(-1)
        out = np.full((paths.shape[0], stride), 0xA5, dtype=np.uint8)
        keep = np.arange(stride)[None, :] < lens[:, None]
        out[keep] = paths[:, :stride][keep]
        return out, lens


def _case(name, stride, opened):
    """one call: opened = [(Tree, indices) or None for a skipped tree (count 0, null handle)].  The expected result is the trees'
    expected openings back to back; a sibling leaf longer than the stride ends the call there: MZK_E_LENGTH, its entry and its length,
    and nothing written from that entry on."""
    tree_lines, idx_all, hn, hl, paths, lens = [], [], [], [], [], []
    for o in opened:
        if o is None:
            tree_lines.append("tree -1 0 0 -")
            continue
        t, idx = o
        idx = np.asarray(idx, dtype=np.uint64)
        tree_lines.append("tree %d %d %d %s" % (t.fid, t.depth, idx.shape[0], _hex(t.neg) if t.neg is not None else "-"))
        dig, limbs = t.gathered(idx)
        p, ln = t.expected(idx, stride)
        idx_all.append(idx.astype("<u8")); hn.append(dig.reshape(-1)); hl.append(limbs.reshape(-1).view(np.uint8)); paths.append(p); lens.append(ln)
    idx_all, hn, hl = np.concatenate(idx_all), np.concatenate(hn), np.concatenate(hl)
    paths, lens = np.concatenate(paths), np.concatenate(lens).astype("<u8")
    entries = lens.shape[0]
    rc, bad_entry, bad_len = 0, 0, 0
    long = np.flatnonzero(lens > stride)
    if long.shape[0]:
        rc, bad_entry, bad_len = E_LENGTH, int(long[0]), int(lens[long[0]])
        paths[bad_entry:] = 0xA5
        lens = lens.copy()
        lens.view(np.uint8)[8 * bad_entry:] = 0xA5
    scratch = idx_all.nbytes + hn.nbytes + hl.nbytes + 64
    head = "case %s stride %d trees %d indices %d nodes %d leaves %d entries %d scratch %d rc %d bad_entry %d bad_len %d" % (
        name, stride, len(opened), idx_all.shape[0], hn.nbytes // 8, hl.nbytes // 4, entries, scratch, rc, bad_entry, bad_len)
    return rc, "\n".join([head] + tree_lines + ["idx " + _hex(idx_all), "hn " + _hex(hn), "hl " + _hex(hl), "paths " + _hex(paths), "lens " + _hex(lens)])


def _cases():
    out = []
    for fid in (mm.FR, mm.M128, mm.M64, mm.M64X3):
        for signed in ((False, True) if fid in (mm.FR, mm.M128) else (False,)):
            for n in (2, 4, 64):
                t = Tree(fid, n, signed)
                longest = int(t.leaf_len.max())
                assert n < 64 or longest == {mm.FR: 41, mm.M128: 25, mm.M64: 17, mm.M64X3: 59}[fid]      # the vector holds a full-length leaf
                name = "%s%s-%d" % (NAMES[fid], "-signed" if signed else "", n)
                every = np.arange(n)
                # a stride of exactly the longest leaf (digests need 32), and of 32: every leaf of M128 and M64 fits that
                rc, text = _case(name + "-exact", max(32, longest), [(t, every)])
                assert rc == 0
                out.append(text)
                if longest <= 32:
                    rc, text = _case(name + "-32", 32, [(t, every)])
                    assert rc == 0
                    out.append(text)
    # several trees in one call: depths 1, 3 and 6, a skipped tree in the middle, a repeated index
    a, b, c = Tree(mm.FR, 2), Tree(mm.M128, 64, signed=True), Tree(mm.M64X3, 8)
    rc, text = _case("multi", 64, [(a, [1, 0]), None, (b, [5, 63, 5, 0, 32]), (c, [7, 2, 2])])
    assert rc == 0
    out.append(text)
    # a stride below one leaf's length: the second tree's third opening is the first whose sibling leaf does not fit 32 bytes
    t = Tree(mm.FR, 64)
    short = [int(i) for i in np.flatnonzero(t.leaf_len <= 32)]
    assert len(short) >= 2 and int(t.leaf_len.max()) > 32
    first_long = int(np.flatnonzero(t.leaf_len > 32)[0])
    rc, text = _case("short-stride", 32, [(Tree(mm.M128, 4), [0, 3]), (t, [short[0] ^ 1, short[1] ^ 1, first_long ^ 1, short[0] ^ 1])])
    assert rc == E_LENGTH and " bad_entry %d " % (2 * 2 + 2 * 6) in text
    out.append(text)
    return out


def test_layout_and_unpack_equal_the_model(tmp_path):
    src = os.path.join(HERE, "hostcheck", "merkle_open_shim.cpp")
    cases = _cases()
    vec = tmp_path / "vectors.txt"
    vec.write_text("\n".join(cases) + "\n")
    common = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"]
    plain, san = str(tmp_path / "merkle_open_shim"), str(tmp_path / "merkle_open_shim_san")
    subprocess.check_call(common + ["-O1", "-o", plain, src])
    subprocess.check_call(common + ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", san, src])
    for exe in (plain, san):
        r = subprocess.run([exe, str(vec)], capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
        assert r.stdout == "ok %d\n" % len(cases)
