"""mzk_fri_prove / mzk_fri_prove_dev: FRI::prove (zkstark/fri.rs:99-143) in one call, with the reference's REAL proof stream on the
device (FiatShamirTransformer = SHAKE256 over the bincode of Vec<Vec<Vec<u8>>>, F::sample, Blake2b-256 sample_indices).

  golden    tests/golden/fri_prove_vectors.json (tests/fri_prove_model.py: Python integers and hashlib), bit-exact
  verifier  fri.rs:262-400 restated in tests/fri_prove_model.py accepts the proof of the reference's test_fri_field flow, rejects
            the corrupted codeword of fri.rs:531-538 and a proof with one revealed value changed
  composed  the same proof built from the callback entry points: mzk_fri_commit_keep_trees with a Python challenge running the real
            transcript, mzk_merkle_open_multi and mzk_merkle_leaves -- field for field
  model     the packed bytes section by section and the unpacked fields against tests/fri_prove_model.py: periodic codewords that put
            every leaf length into every tree (with and without signs on round 0), and a last codeword of 512 elements
  _dev      from a torch tensor, and two proofs enqueued back to back before one synchronize
  errors    every validation failure returns before anything is enqueued"""
import ctypes, json, os
import numpy as np
import pytest
import orc
import fri_prove_model as fm
import fri_prove_cases as fc
from orc import FR, M128

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GEN = orc.M128_GEN
PRIME = {FR: fm.P_FR, M128: fm.P_M128}


@pytest.fixture(scope="module")
def mz():
    import myzkp_amd as m
    m.init(0)
    return m


def codeword_of(fid, n, seed):
    return orc.synth_vector(fid, seed, n)


def root(fid, lg):
    return orc.root_of(fid, lg)


def as_model(proof):
    """fri_unpack_proof's dict -> plain lists (last codeword as ints) for comparison with the model"""
    out = dict(proof)
    out["last_codeword"] = orc.from_limbs(proof["last_codeword"])
    return out


def test_golden_vectors(mz):
    cases = json.load(open(os.path.join(HERE, "golden", "fri_prove_vectors.json")))
    assert len(cases) == 3
    for c in cases:
        fid, n = c["field"], c["n"]
        vals = [int(v) for v in c["codeword"]]
        neg = np.array([1 if v < 0 else 0 for v in vals], dtype=np.uint8)
        mags = orc.to_limbs([abs(v) for v in vals], orc.LIMBS[fid])
        proof = mz.fri_prove(fid, mags, int(c["omega"]), int(c["offset"]), c["expansion_factor"], c["num_colinearity_tests"],
                             negative=neg if neg.any() else None)
        assert proof["top_level_indices"] == c["top_level_indices"], c["name"]
        assert [r.hex() for r in proof["merkle_roots"]] == c["merkle_roots"], c["name"]
        assert [str(v) for v in orc.from_limbs(proof["last_codeword"])] == c["last_codeword"], c["name"]
        for L, G in zip(proof["revealed_layers"], c["revealed_layers"]):
            for k in "abc":
                assert [str(v) for v in L[k][0]] == G[k]["values"], (c["name"], k)
                assert [[e.hex() for e in p] for p in L[k][1]] == G[k]["paths"], (c["name"], k)
        assert len(proof["revealed_layers"]) == len(c["revealed_layers"])


@pytest.mark.parametrize("degree,expansion,tests", [(63, 4, 17), (4095, 4, 17), (1023, 8, 10)])
def test_fri_field_real_transcript(mz, degree, expansion, tests):
    P = fm.P_M128
    n = (degree + 1) * expansion
    lg = n.bit_length() - 1
    omega = orc.m128_root(lg)
    coef = list(range(degree + 1))                                                        # fri.rs:514-518
    codeword = mz.ntt(M128, omega, orc.to_limbs(coef + [0] * (n - degree - 1), 2))
    proof = as_model(mz.fri_prove(M128, codeword, omega, GEN, expansion, tests))
    assert len(proof["merkle_roots"]) == fm.num_rounds(n, expansion, tests)
    points = []
    assert fm.verify(P, proof, omega, GEN, n, expansion, tests, points)
    assert len(points) == 2 * tests
    for x, y in points:                                                                   # fri.rs:527-529
        assert sum(c * pow(omega, x * i, P) for i, c in enumerate(coef)) % P == y
    bad = codeword.copy()                                                                 # fri.rs:531-538
    bad[:degree // 3] = orc.to_limbs([1], 2)[0]
    assert not fm.verify(P, as_model(mz.fri_prove(M128, bad, omega, GEN, expansion, tests)), omega, GEN, n, expansion, tests)
    L0 = proof["revealed_layers"][0]
    L0["a"][0][3] = (L0["a"][0][3] + 1) % P
    assert not fm.verify(P, proof, omega, GEN, n, expansion, tests)


def composed(mz, fid, codeword, omega, offset, expansion, tests, negative=None):
    """The same proof from today's entry points: keep-trees commit with the real transcript in a Python callback, then
    merkle_open_multi for every path and MerkleTree.leaves for every value (fri.rs:99-260)."""
    p = PRIME[fid]
    n = codeword.shape[0]
    R = fm.num_rounds(n, expansion, tests)
    stream = []

    def challenge(rnd, last, rt):
        stream.append([rt])
        return None if last else fm.sample(fm.fiat_shamir(stream)) % p

    _, roots, trees = mz.fri_commit(fid, codeword, omega, offset, R, challenge, negative=negative, keep_trees=True, codewords=False)
    m = n >> (R - 1)
    last = trees[-1].leaves(list(range(m)))
    stream.append([fm.leaf(v) for v in orc.from_limbs(last)])
    top = fm.sample_indices(fm.fiat_shamir(stream), n // 2, m, tests)
    wanted, per = [[] for _ in range(R)], []
    for i in range(R - 1):
        half = (n >> i) // 2
        a = [t % half for t in top]
        b = [x + half for x in a]
        per.append((a, b))
        wanted[i] += a + b
        wanted[i + 1] += a
    opened = mz.merkle_open_multi(trees, wanted)
    layers = []
    for i, (a, b) in enumerate(per):
        skip = tests if i > 0 else 0

        def vals(t, idx):
            mags, ng = trees[t].leaves(idx, with_sign=True)
            return [-v if s else v for v, s in zip(orc.from_limbs(mags), ng)]
        layers.append({"a": (vals(i, a), opened[i][skip:skip + tests]), "b": (vals(i, b), opened[i][skip + tests:skip + 2 * tests]),
                       "c": (vals(i + 1, a), opened[i + 1][:tests])})
    for t in trees:
        t.close()
    return {"top_level_indices": top, "last_codeword": orc.from_limbs(last), "merkle_roots": roots, "revealed_layers": layers}


@pytest.mark.parametrize("fid", [M128, FR])
@pytest.mark.parametrize("lg", [10, 12, 14, 16])
def test_equals_composed_form(mz, fid, lg):
    n = 1 << lg
    cw = codeword_of(fid, n, 40 + lg)
    w, expansion, tests = root(fid, lg), 4, 17
    one = as_model(mz.fri_prove(fid, cw, w, 7, expansion, tests))
    assert one == composed(mz, fid, cw, w, 7, expansion, tests)


def test_equals_composed_form_2_20(mz):
    n = 1 << 20
    cw = codeword_of(M128, n, 99)
    w = root(M128, 20)
    assert as_model(mz.fri_prove(M128, cw, w, GEN, 4, 17)) == composed(mz, M128, cw, w, GEN, 4, 17)


@pytest.mark.parametrize("fid", [M128, FR])
def test_signed_round_zero(mz, fid):
    n, p = 1 << 10, PRIME[fid]
    cw = codeword_of(fid, n, 5)
    neg = (np.arange(n) % 3 == 1).astype(np.uint8)
    cw[7] = 0
    w = root(fid, 10)
    one = as_model(mz.fri_prove(fid, cw, w, 3, 4, 17, negative=neg))
    assert one == composed(mz, fid, cw, w, 3, 4, 17, negative=neg)
    model, _ = fm.prove(p, [-v if s else v for v, s in zip(orc.from_limbs(cw), neg)], w, 3, 4, 17)
    assert one == model
    assert any(v < 0 for v in one["revealed_layers"][0]["a"][0] + one["revealed_layers"][0]["b"][0])


# ---- against the model, packed bytes and fields: every leaf length in every tree, and a last codeword of two scan batches ----------------
def pack(fid, proof, tests):
    """the model's proof in mzk_fri_prove's packed form: {section: bytes}; a negative value is a magnitude and a sign byte of 1"""
    limbs = lambda vs: orc.to_limbs([abs(v) for v in vs], orc.LIMBS[fid]).tobytes()
    out = {"status": bytes(8), "top_indices": np.array(proof["top_level_indices"], dtype=np.uint64).tobytes(),
           "roots": b"".join(proof["merkle_roots"]), "last_codeword": limbs(proof["last_codeword"])}
    values, signs, paths, lens = [], [], [], []
    for layer in proof["revealed_layers"]:
        for k in "abc":
            values.append(limbs(layer[k][0]))
            signs += [1 if v < 0 else 0 for v in layer[k][0]]
            for path in layer[k][1]:
                for entry in path:
                    assert len(entry) <= fm.PATH_STRIDE
                    paths.append(entry + bytes(fm.PATH_STRIDE - len(entry)))
                    lens.append(len(entry))
    out.update(values=b"".join(values), signs=bytes(signs), paths=b"".join(paths), path_lens=np.array(lens, dtype=np.uint64).tobytes())
    return out


def prove_and_compare(mz, fid, cw, lg, expansion, tests, flags=None):
    """one proof of the codeword `cw` (ints; a negative one is given as magnitude and Sign::Minus flag, `flags` may flag zeros as well)
    through the C entry point against the model: the packed sections byte for byte (zero padding of every path slot included; not
    the alignment gaps between sections), then the unpacked fields; returns the model's proof"""
    n, nl = len(cw), orc.LIMBS[fid]
    omega, offset = root(fid, lg), 7
    want, _ = fm.prove(PRIME[fid], cw, omega, offset, expansion, tests)
    neg = np.array([1 if v < 0 else 0 for v in cw] if flags is None else flags, dtype=np.uint8)
    assert all(f for v, f in zip(cw, neg) if v < 0) and not any(f for v, f in zip(cw, neg) if v > 0)
    mags, w, o = orc.to_limbs([abs(v) for v in cw], nl), orc.to_limbs([omega], nl), orc.to_limbs([offset], nl)
    R, sec, total = fm.layout(nl, n, expansion, tests)
    buf = (ctypes.c_uint8 * total)()
    rc = mz.lib().mzk_fri_prove(fid, orc.ptr(mags), orc.ptr(neg) if neg.any() else None, ctypes.c_size_t(n), orc.ptr(w), orc.ptr(o),
                                ctypes.c_size_t(expansion), ctypes.c_size_t(tests), buf, ctypes.c_size_t(total))
    assert rc == 0, mz.lib().mzk_last_error()
    raw = bytes(buf)
    packed = pack(fid, want, tests)
    for k in fm.SECTIONS:
        off, size = sec[k]
        assert len(packed[k]) == size, k
        assert raw[off:off + size] == packed[k], k
    got = as_model(mz.fri_unpack_proof(fid, n, expansion, tests, raw))
    for k in ("top_level_indices", "last_codeword", "merkle_roots", "revealed_layers"):
        assert got[k] == want[k], k
    return want


@pytest.mark.parametrize("fid", [M128, FR])
@pytest.mark.parametrize("n,expansion,tests,rounds,m", [(64, 4, 4, 2, 32), (64, 2, 3, 3, 16), (1024, 16, 17, 4, 128)])
def test_edge_vectors_through_a_periodic_codeword(mz, fid, n, expansion, tests, rounds, m):
    """cw[i] = v[i mod m]: every fold has a = b, so the edge values -- the zero element and every trimmed word count -- are every round's
    leaves, every revealed sibling's candidates and the last codeword"""
    assert fm.num_rounds(n, expansion, tests) == rounds and n >> (rounds - 1) == m
    v = fc.edge_vector(PRIME[fid], 2 * orc.LIMBS[fid], m)
    want = prove_and_compare(mz, fid, fc.periodic(v, n), n.bit_length() - 1, expansion, tests)
    assert want["last_codeword"] == v


@pytest.mark.parametrize("fid", [M128, FR])
def test_edge_vectors_with_signs_on_round_zero(mz, fid):
    """the m = 32 periodic case with Sign::Minus flags on round 0 (periodic as well, so that a = b still holds after the fold has
    canonicalised them), the zero element flagged too: its leaf stays NoSign"""
    n, expansion, tests, rounds, m = 64, 4, 4, 2, 32
    assert fm.num_rounds(n, expansion, tests) == rounds and n >> (rounds - 1) == m
    p = PRIME[fid]
    flags = [1 if j % 3 != 2 else 0 for j in range(m)]
    v = [-x if f else x for x, f in zip(fc.edge_vector(p, 2 * orc.LIMBS[fid], m), flags)]
    assert v[0] == 0 and flags[0] and v[1] == -1
    want = prove_and_compare(mz, fid, fc.periodic(v, n), 6, expansion, tests, flags=fc.periodic(flags, n))
    assert want["last_codeword"] == [x % p for x in v]
    L0 = want["revealed_layers"][0]
    assert any(x < 0 for x in L0["a"][0] + L0["b"][0]) and all(x >= 0 for x in L0["c"][0])


@pytest.mark.parametrize("fid", [M128, FR])
def test_last_codeword_of_two_scan_batches(mz, fid):
    """m = 512: the second batch of records starts where the first one's prefix sum ended"""
    n, expansion, tests, rounds, m = 4096, 4, 100, 4, 512
    assert fm.num_rounds(n, expansion, tests) == rounds and n >> (rounds - 1) == m
    cw = orc.from_limbs(codeword_of(fid, n, 61 + fid))
    cw[n // 2], cw[n - 1] = 0, PRIME[fid] - 1
    prove_and_compare(mz, fid, cw, 12, expansion, tests)


def test_dev_form_and_back_to_back(mz):
    import torch
    n, fid, exp, tests = 1 << 12, M128, 4, 17
    w = root(fid, 12)
    cws = [codeword_of(fid, n, s) for s in (11, 12)]
    want = [mz.fri_prove(fid, c, w, GEN, exp, tests) for c in cws]
    for c, wnt in zip(cws, want):                                        # the Python _dev path: torch tensor in, same proof out
        t = torch.from_numpy(c.view(np.int64)).cuda()
        got = mz.fri_prove(fid, None, w, GEN, exp, tests, device_ptr=t.data_ptr(), n=n)
        assert as_model(got) == as_model(wnt)
    _, _, total = mz.fri_proof_layout(fid, n, exp, tests)
    ts = [torch.from_numpy(c.view(np.int64)).cuda() for c in cws]
    outs = [torch.zeros(total, dtype=torch.uint8, device="cuda") for _ in cws]
    torch.cuda.synchronize()
    s = torch.cuda.current_stream()
    wl, ol = orc.to_limbs([w], 2), orc.to_limbs([GEN], 2)
    for t, o in zip(ts, outs):                                            # two proofs enqueued, then ONE synchronize
        rc = mz.lib().mzk_fri_prove_dev(fid, ctypes.c_void_p(t.data_ptr()), None, ctypes.c_size_t(n), orc.ptr(wl), orc.ptr(ol), ctypes.c_size_t(exp),
                                        ctypes.c_size_t(tests), ctypes.c_void_p(o.data_ptr()), ctypes.c_size_t(total), ctypes.c_void_p(s.cuda_stream))
        assert rc == 0
    s.synchronize()
    for o, wnt in zip(outs, want):
        assert as_model(mz.fri_unpack_proof(fid, n, exp, tests, o.cpu().numpy().tobytes())) == as_model(wnt)


def test_errors_enqueue_nothing(mz):
    L = mz.lib()
    cw = codeword_of(M128, 1 << 10, 3)
    w, o = orc.to_limbs([root(M128, 10)], 2), orc.to_limbs([GEN], 2)
    _, _, total = mz.fri_proof_layout(M128, 1 << 10, 4, 17)
    buf = (ctypes.c_uint8 * total)()
    sentinel = bytes([0xA5]) * total
    ctypes.memmove(buf, sentinel, total)

    def call(fid=M128, c=cw, n=1 << 10, ww=w, oo=o, exp=4, tests=17, cap=total):
        return L.mzk_fri_prove(fid, None if c is None else orc.ptr(c), None, ctypes.c_size_t(n), None if ww is None else orc.ptr(ww), orc.ptr(oo),
                               ctypes.c_size_t(exp), ctypes.c_size_t(tests), buf, ctypes.c_size_t(cap))
    bad_w = orc.to_limbs([fm.P_M128], 2)
    cases = [(dict(fid=7), -1), (dict(c=None), -1), (dict(ww=None), -1), (dict(n=0), -5), (dict(n=1000), -2), (dict(exp=1 << 10), -5),
             (dict(exp=512), -5), (dict(tests=1 << 9), -5), (dict(n=64, exp=2, tests=20), -5), (dict(ww=bad_w), -6), (dict(cap=total - 1), -5)]
    for kw, code in cases:
        assert call(**kw) == code, kw
        assert bytes(buf) == sentinel, kw
    # the device form: nothing may be enqueued either -- the output tensor stays as it was
    import torch
    t = torch.from_numpy(cw.view(np.int64)).cuda()
    out = torch.full((total,), 0xA5, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()
    rc = L.mzk_fri_prove_dev(M128, ctypes.c_void_p(t.data_ptr()), None, ctypes.c_size_t(1 << 10), orc.ptr(w), orc.ptr(o), ctypes.c_size_t(4),
                             ctypes.c_size_t(17), ctypes.c_void_p(out.data_ptr()), ctypes.c_size_t(total - 8), ctypes.c_void_p(s.cuda_stream))
    assert rc == -5
    s.synchronize()
    assert bytes(out.cpu().numpy()) == sentinel
