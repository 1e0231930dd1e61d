"""mzk_stark_prove / mzk_stark_prove_dev (the Stark class): FastStark::prove in one call.
  * the golden proofs (tests/golden/stark_vectors.json) bit for bit from Stark.prove and prove_dev; the model's verifier accepts them,
    rejects the false-boundary proofs produced BY THE LIBRARY and one changed byte / value in every proof section;
  * scale: the two-register AIR of tests/test_gpu_stark_stages.py at T = 2000, 30000, 120000 with 17 colinearity checks and once over Fr:
    the model's verifier (O(T) per query) accepts and rejects the false boundary; the proof equals the one assembled stage by stage
    (whose roots that file rebuilds from Python long division and the oracle); two calls give identical bytes; host and _dev forms agree;
  * workspace hygiene: a prove between unrelated calls changes none of their results, nor they its own; the workspace can be released.
Every case here has two registers, degree 2, expansion 4 and two constraints with equal shifts, and every refusal happens before the
first launch.  Other register counts, degrees, expansion factors, constraint counts and shifts, boundaries that leave a register
without an entry, the prefix interpolation and zerofier, the small coset division, a constant register, a refusal after work is
enqueued and one handle over several boundaries are tests/test_gpu_stark_shapes.py, bit for bit against the model's prover."""
import json, os, random, sys
import numpy as np
import pytest
import orc
import mpoly_model as mm
import stark_model as sm
from test_gpu_stark_stages import env, rescue, prove_staged, two_register     # noqa: F401 (env is a fixture)

pytestmark = pytest.mark.gpu
M128 = orc.M128
P = mm.M128_P


def limbs_trace(fid, trace):
    nl = orc.LIMBS[fid]
    return orc.to_limbs([v for row in trace for v in row], nl).reshape(len(trace), len(trace[0]), nl)


def prove_both(env, st, fid, trace, boundary, randomizer):
    """host form, host form again, _dev form: identical bytes; returns (raw, unpacked without the convenience section)"""
    torch, mz, dev, stream = env
    nl = orc.LIMBS[fid]
    t, r = limbs_trace(fid, trace), orc.to_limbs(randomizer, nl)
    raw = st.prove_raw(t, boundary, r)
    assert st.prove_raw(t, boundary, r) == raw, "two calls differ"
    dims = st.dims(boundary)
    _, total = mz.stark_proof_layout(fid, dims)
    assert len(raw) == total
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to(dev)
    d_t, d_r = to_dev(t), to_dev(r)
    d_p = torch.zeros(total + 8, dtype=torch.uint8, device=dev)
    st.prove_dev(d_t.data_ptr(), len(trace), boundary, d_r.data_ptr(), d_p.data_ptr(), total, stream)
    torch.cuda.synchronize()
    assert d_p[:total].cpu().numpy().tobytes() == raw, "host and _dev forms differ"
    proof = mz.stark_unpack_proof(fid, dims, raw)
    indices = proof.pop("indices")
    top = proof["fri"]["top_level_indices"]
    flen, e = dims["fri_domain_length"], dims["fri_domain_length"] // dims["omicron_domain_length"]
    dup = top + [(i + e) % flen for i in top]
    assert top == sorted(top) and indices == sorted(dup + [(i + flen // 2) % flen for i in dup])
    return raw, proof


def tampered(proof, P=P):
    """one changed value / path byte / root in every section of the FastStarkProof (P: the field's modulus)"""
    for key in ("bqc_points", "rdc_points", "tzc_points"):
        bad = dict(proof)
        bad[key] = [(proof[key][0] + 1) % P] + list(proof[key][1:])
        yield key, bad
    for key in ("bqc_paths", "rdc_paths", "tzc_paths"):
        bad = dict(proof)
        first = list(proof[key][0])
        first[-1] = bytes([first[-1][0] ^ 1]) + first[-1][1:]
        bad[key] = [first] + list(proof[key][1:])
        yield key, bad
    bad = dict(proof)
    bad["bqc_roots"] = [bytes([proof["bqc_roots"][0][0] ^ 1]) + proof["bqc_roots"][0][1:]] + proof["bqc_roots"][1:]
    yield "bqc_roots", bad
    bad = dict(proof)
    bad["rdc_root"] = bytes([proof["rdc_root"][0] ^ 1]) + proof["rdc_root"][1:]
    yield "rdc_root", bad
    bad = dict(proof)
    bad["fri"] = dict(proof["fri"], last_codeword=[(proof["fri"]["last_codeword"][0] + 1) % P] + proof["fri"]["last_codeword"][1:])
    yield "fri", bad


def test_golden_proofs_bit_for_bit(env):
    mz = env[1]
    rp, model, air = rescue()
    cons = [mm.terms_of(a) for a in air]
    with open(os.path.join(orc.ROOT, "tests", "golden", "stark_vectors.json")) as f:
        gold = json.load(f)
    sys.path.insert(0, os.path.join(orc.ROOT, "tests", "golden"))
    import make_golden_stark as mg
    tz_root = bytes.fromhex(gold["transition_zerofier_root"])
    with mz.Stark(M128, 4, 2, rp.m, rp.n + 1, 2, mm.M128_GEN, cons) as st:
        assert st.transition_zerofier_root() == tz_root
        full = 0
        for case in gold["cases"]:
            tr = rp.trace(int(case["input"]))
            claimed = int(case["claimed_output"])
            boundary = [(0, 1, 0), (rp.n, 0, claimed)]
            trace = [list(r) for r in tr] + [[int(v) for v in row] for row in case["random_rows"]]
            _, proof = prove_both(env, st, M128, trace, boundary, [int(v) for v in case["randomizer"]])
            assert [r.hex() for r in proof["bqc_roots"]] == case["bqc_roots"] and proof["rdc_root"].hex() == case["rdc_root"], case["name"]
            assert sm.proof_digest(proof) == case["digest"], case["name"]
            if "proof" in case:
                assert mg.render(proof) == case["proof"]
                full += 1
            if claimed == tr[-1][0]:
                assert model.verify(proof, air, boundary, tz_root) is True, case["name"]
                for key, bad in tampered(proof):
                    assert model.verify(bad, air, boundary, tz_root) is not True, key
            else:
                assert model.verify(proof, air, boundary, tz_root) == "combination", case["name"]
        assert full == 1 and len(gold["cases"]) >= 4


@pytest.mark.parametrize("fid,T", [(M128, 2000), (M128, 30000), (M128, 120000), (orc.FR, 2000)])
def test_scale(env, fid, T):
    mz = env[1]
    p = orc.MOD[fid]
    checks, e = 17, 4
    lg = ((T + 4 * checks) * 2).bit_length()
    omicron, omega = orc.root_of(fid, lg), orc.root_of(fid, lg + 2)
    g = orc.M128_GEN if fid == M128 else 5
    rnd = random.Random(T + fid)
    rows, cons = two_register(p, T, 3, 4, omicron)
    boundary = [(0, 0, 3), (0, 1, 4), (T - 1, 0, rows[-1][0])]
    false_boundary = boundary[:2] + [(T - 1, 0, (rows[-1][0] + 1) % p)]
    trace = rows + [[rnd.randrange(p) for _ in range(2)] for _ in range(4 * checks)]
    model = sm.FastStark(p, g, omega, omicron, e, checks, 2, T, 2)
    air = [{tuple(k): c for c, k in terms} for terms in cons]

    def zerofier_at(v):
        acc, w = 1, 1
        for _ in range(T - 1):
            acc, w = acc * (v - w) % p, w * omicron % p
        return acc

    with mz.Stark(fid, e, checks, 2, T, 2, g, cons) as st:
        d = st.dims(boundary)
        assert (d["omicron_domain_length"], d["fri_domain_length"]) == (1 << lg, 1 << (lg + 2))
        randomizer = [rnd.randrange(p) for _ in range(d["randomizer_length"])]
        _, proof = prove_both(env, st, fid, trace, boundary, randomizer)
        staged, extra = prove_staged(env, fid, p, g, omega, omicron, e, checks, 2, T, 2, cons, trace, boundary, randomizer)
        assert st.transition_zerofier_root() == extra["tz_root"]
        assert sm.proof_digest(proof) == sm.proof_digest(staged)
        assert model.verify(proof, air, boundary, extra["tz_root"], zerofier_at) is True
        _, bad = prove_both(env, st, fid, trace, false_boundary, randomizer)
        assert model.verify(bad, air, false_boundary, extra["tz_root"], zerofier_at) == "combination"


def test_errors_before_anything_is_enqueued(env):
    mz = env[1]
    rp, model, air = rescue()
    cons = [mm.terms_of(a) for a in air]
    rnd = random.Random(5)
    tr = rp.trace(7)
    boundary = [(0, 1, 0), (rp.n, 0, tr[-1][0])]
    trace = [list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(8)]
    rand = [rnd.randrange(P) for _ in range(128)]
    with mz.Stark(M128, 4, 2, rp.m, rp.n + 1, 2, mm.M128_GEN, cons) as st:
        t, r = limbs_trace(M128, trace), orc.to_limbs(rand, 2)
        good = st.prove_raw(t, boundary, r)
        for args, code in (((t[:-1], boundary, r), -5), ((t, boundary + [(1, 0, 0)] * 40, r), -5),
                           ((limbs_trace(M128, [[P, 0]] + trace[1:]), boundary, r), -6), ((t, boundary, orc.to_limbs([P] + rand[1:], 2)), -6),
                           ((t, [(0, 1, P)], r), -6)):
            with pytest.raises(mz.MzkError) as e:
                st.prove_raw(*args)
            assert e.value.code == code
        import ctypes
        L, sz = mz.lib(), ctypes.c_size_t
        bc, br, bv, nb = st._boundary(boundary)
        buf = (ctypes.c_uint8 * len(good))()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        assert L.mzk_stark_prove(st._h, ptr(t), sz(36), bc, br, ptr(bv), nb, ptr(r), buf, sz(len(good) - 1)) == -5          # proof_cap too small
        assert L.mzk_stark_prove(st._h, None, sz(36), bc, br, ptr(bv), nb, ptr(r), buf, sz(len(good))) == -1
        assert L.mzk_stark_prove(None, ptr(t), sz(36), bc, br, ptr(bv), nb, ptr(r), buf, sz(len(good))) == -1
        assert st.prove_raw(t, boundary, r) == good
    with pytest.raises(mz.MzkError) as e:
        mz.Stark(M128, 3, 2, rp.m, rp.n + 1, 2, mm.M128_GEN, cons)
    assert e.value.code == -2
    with pytest.raises(mz.MzkError) as e:
        mz.Stark(M128, 4, 2, rp.m, rp.n + 1, 2, P, cons)
    assert e.value.code == -6


def test_workspace_hygiene(env):
    torch, mz, dev, stream = env
    rp, model, air = rescue()
    cons = [mm.terms_of(a) for a in air]
    rnd = random.Random(6)
    tr = rp.trace(99)
    boundary = [(0, 1, 0), (rp.n, 0, tr[-1][0])]
    t = limbs_trace(M128, [list(r) for r in tr] + [[rnd.randrange(P) for _ in range(rp.m)] for _ in range(8)])
    r = orc.to_limbs([rnd.randrange(P) for _ in range(128)], 2)
    v = orc.synth_vector(M128, 50, 1 << 12)
    f = orc.synth_vector(orc.FR, 51, 300)
    srs = orc.kzg_setup_ref(5, 299)
    point = [orc.synth_vector(M128, 52, 40), orc.synth_vector(M128, 53, 33)]

    def others():
        y, w = mz.kzg_open(f, 12345, srs)
        return (mz.ntt(M128, orc.root_of(M128, 12), v).tobytes(), str(y), str(w),
                [q.tobytes() for q in mz.mpoly_compose(M128, [[(3, (1, 2)), (5, (0, 1))]], point)])

    with mz.Stark(M128, 4, 2, rp.m, rp.n + 1, 2, mm.M128_GEN, cons) as st:
        before = others()
        mine = st.prove_raw(t, boundary, r)
        assert others() == before
        assert st.prove_raw(t, boundary, r) == mine
        mz.trim_workspace()
        assert st.prove_raw(t, boundary, r) == mine
        assert others() == before
