"""FastStark::prove stage by stage through the library's entry points -- the sequence mzk_stark_prove chains, run one call at a time so
that every intermediate can be looked at (tests/test_gpu_stark.py checks the one call) -- against what does not come from the library:
  * the golden proofs (tests/golden/stark_vectors.json, reference parameters: Rescue-Prime, 28 cycles, expansion 4, 2 colinearity
    checks): the proof the stages produce is the golden one bit for bit, true and false outputs; the model's verifier accepts the
    former, rejects the latter and rejects a proof with one value or path byte changed in any section;
  * every intermediate of the model (trace polynomials, boundary quotients, transition polynomials and quotients, weights, combination)
    and the sizes of mzk_stark_plan;
  * at scale, the two-register AIR next0 = prev0^2 + prev1, next1 = prev0 prev1 + X at T = 2000 / 30000 / 120000 with 17 colinearity
    checks (FRI domain 2^15 / 2^18 / 2^20) and once over Fr: the boundary-quotient roots equal roots rebuilt from Python long division
    by the expanded zerofier + the oracle's coset evaluation + the oracle's Merkle commit; the transition quotients of the composed
    constraints, divided in one call, times the zerofier give back the transition polynomials.
The weights come from sample_weights over the roots the LIBRARY produced, so a wrong root changes everything after it."""
import json, os, random, sys
import numpy as np
import pytest
import orc
import mpoly_model as mm
import fri_prove_model as fm
import stark_model as sm

pytestmark = pytest.mark.gpu
M128 = orc.M128
P = mm.M128_P


@pytest.fixture(scope="module")
def env():
    import torch
    import myzkp_amd as mz
    mz.init(0)
    return torch, mz, torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream


def L(vals):
    return orc.to_limbs([int(v) for v in vals], 2)


def I(arr):
    return orc.from_limbs(arr)


def rescue():
    with open(os.path.join(orc.ROOT, "tests", "golden", "rescue_prime_m128.json")) as f:
        rp = mm.RescuePrime(json.load(f))
    g, omega, omicron = mm.M128_GEN, mm.m128_root(9), mm.m128_root(7)
    model = sm.FastStark(P, g, omega, omicron, 4, 2, rp.m, rp.n + 1, 2)
    return rp, model, rp.transition_constraints(omicron)


def prove_staged(env, fid, p, g, omega, omicron, e, checks, m, cycles, degree, cons, trace, boundary, randomizer, dbg=None, exact=True):
    """fast_stark.rs:177-396 over the library's entry points; returns the proof in the model's shape.  dbg: the model's intermediates to
    compare with on the way.  exact: every quotient meets its degree bound (False for a trace with a constant register, whose
    polynomials are shorter: the bounds then hold as bounds)."""
    meets = (lambda degrees, bounds: degrees == bounds) if exact else (lambda degrees, bounds: all(a <= b for a, b in zip(degrees, bounds)))
    torch, mz, dev, st = env
    nl = orc.LIMBS[fid]
    Lf = lambda vals: orc.to_limbs([int(v) for v in vals], nl)
    d = mz.stark_plan(fid, e, checks, m, cycles, degree, cons, boundary)
    olen, flen, rl = d["omicron_domain_length"], d["fri_domain_length"], d["randomized_trace_length"]
    assert (rl, d["randomizer_length"]) == (len(trace), len(randomizer))
    # interpolate every register (:197-215)
    domain = Lf([pow(omicron, i, p) for i in range(rl)])
    tps = mz.fast_interpolate_batch(fid, domain, np.stack([Lf([row[s] for row in trace]) for s in range(m)]), omicron, olen)
    # boundary quotients (:217-224): no interpolant, the roots alone
    roots = [[pow(omicron, c, p) for c, r, _ in boundary if r == s] for s in range(m)]
    bqs = mz.poly_div_roots(fid, tps, roots)
    assert meets([q.shape[0] - 1 for q in bqs], d["boundary_quotient_degree_bounds"])
    # extend and commit (:228-244)
    codewords = [mz.coset_lde(fid, q, g, omega, flen) for q in bqs]
    trees = [mz.MerkleTree(fid, cw) for cw in codewords]
    proof = {"bqc_roots": [bytes(mz.merkle_commit_field(fid, cw)) for cw in codewords]}
    stream = [[r] for r in proof["bqc_roots"]]
    # evaluate_symbolic of the AIR over (X, tp, tp.scale(omicron)) (:246-259)
    point = [Lf([0, 1])] + list(tps) + [mz.poly_scale(fid, q, omicron) for q in tps]
    tpolys = mz.mpoly_compose(fid, cons, point)
    assert all(q.shape[0] - 1 <= b for q, b in zip(tpolys, d["transition_degree_bounds"]))
    # every fast_coset_divide by the transition zerofier in one call (:261-273), numerators and denominator in HBM; fast_zerofier keeps
    # its padding, the division trims it on the device
    tz = mz.fast_zerofier(fid, domain[:cycles - 1], omicron, olen)
    stride = max(q.shape[0] for q in tpolys)
    flat = np.zeros((len(tpolys) * stride, nl), dtype=np.uint64)
    for a, q in enumerate(tpolys):
        flat[a * stride:a * stride + q.shape[0]] = q
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64).reshape(-1).copy()).to(dev)
    d_num, d_tz = to_dev(flat), to_dev(tz)
    d_tq = torch.full_like(d_num, -1)
    qlens = mz.fast_coset_divide_batch_dev(fid, d_num.data_ptr(), stride, [q.shape[0] for q in tpolys], d_tz.data_ptr(), tz.shape[0], g, omicron, olen,
                                           d_tq.data_ptr(), stride, st)
    torch.cuda.synchronize()
    out = d_tq.cpu().numpy().view(np.uint64).reshape(len(tpolys), stride, nl)
    tqs = [out[a, :qlens[a]].copy() for a in range(len(tpolys))]
    assert meets([n - 1 for n in qlens], d["transition_quotient_degree_bounds"])
    # the randomizer codeword and its root (:275-299), the weights over the library's roots
    r_cw = mz.coset_lde(fid, Lf(randomizer), g, omega, flen)
    proof["rdc_root"] = bytes(mz.merkle_commit_field(fid, r_cw))
    stream.append([proof["rdc_root"]])
    weights = sm.sample_weights(d["n_weights"], fm.fiat_shamir(stream), p)
    # the weighted sum (:301-326) with the plan's shifts, its codeword, FRI (:328-337)
    polys, shifts = [Lf(randomizer)], [0]
    for a, q in enumerate(tqs):
        polys += [q, q]
        shifts += [0, d["transition_shifts"][a]]
    for s, q in enumerate(bqs):
        polys += [q, q]
        shifts += [0, d["boundary_shifts"][s]]
    comb = mz.poly_lincomb(fid, polys, weights, shifts)
    assert comb.shape[0] <= d["max_degree"] + 1
    fri = mz.fri_prove(fid, mz.coset_lde(fid, comb, g, omega, flen), omega, g, e, checks)
    fri["last_codeword"] = orc.from_limbs(fri["last_codeword"])
    fri["top_level_indices"] = sorted(fri["top_level_indices"])                    # :338
    dup = list(fri["top_level_indices"]) + [(i + e) % flen for i in fri["top_level_indices"]]
    dup = sorted(dup + [(i + flen // 2) % flen for i in dup])
    assert len(dup) == 4 * checks == d["num_indices"]
    # open the boundary-quotient, randomizer and zerofier codewords at the duplicated indices in one pass (:338-383)
    tz_cw = mz.coset_lde(fid, tz, g, omega, flen)
    all_cw = codewords + [r_cw, tz_cw]
    paths = mz.merkle_open_multi(trees + [mz.MerkleTree(fid, r_cw), mz.MerkleTree(fid, tz_cw)], [dup] * (m + 2))
    pts = [orc.from_limbs(cw[dup]) for cw in all_cw]
    proof.update({"fri": fri, "bqc_points": [v for s in range(m) for v in pts[s]], "bqc_paths": [q for s in range(m) for q in paths[s]],
                  "rdc_points": pts[m], "rdc_paths": paths[m], "tzc_points": pts[m + 1], "tzc_paths": paths[m + 1]})
    if dbg is not None:
        I = orc.from_limbs
        assert [I(q) for q in tps] == dbg["trace_polynomials"] and [I(q) for q in bqs] == dbg["boundary_quotients"]
        assert [I(q) for q in tpolys] == dbg["transition_polynomials"] and [I(q) for q in tqs] == dbg["transition_quotients"]
        assert mm.trim(I(tz)) == sm.from_monomials([pow(omicron, i, p) for i in range(cycles - 1)], p)
        assert weights == dbg["weights"] and I(comb) == dbg["combination"] and dup == dbg["indices"]
    return proof, {"tps": tps, "bqs": bqs, "roots": roots, "tpolys": tpolys, "tqs": tqs, "tz": tz, "dims": d, "tz_root": bytes(mz.merkle_commit_field(fid, tz_cw))}


def test_golden_proofs_bit_for_bit_and_the_verifier(env):
    rp, model, air = rescue()
    cons = [mm.terms_of(a) for a in air]
    with open(os.path.join(orc.ROOT, "tests", "golden", "stark_vectors.json")) as f:
        gold = json.load(f)
    sys.path.insert(0, os.path.join(orc.ROOT, "tests", "golden"))
    import make_golden_stark as mg
    tz_root = bytes.fromhex(gold["transition_zerofier_root"])
    assert len(gold["cases"]) >= 4
    for case in gold["cases"]:
        tr = rp.trace(int(case["input"]))
        claimed = int(case["claimed_output"])
        true_output = claimed == tr[-1][0]
        boundary = [(0, 1, 0), (rp.n, 0, claimed)]
        trace = [list(r) for r in tr] + [[int(v) for v in row] for row in case["random_rows"]]
        randomizer = [int(v) for v in case["randomizer"]]
        dbg = model.prove(trace, boundary, air, randomizer)["_debug"]
        proof, extra = prove_staged(env, M128, P, model.generator, model.omega, model.omicron, 4, 2, rp.m, rp.n + 1, 2, cons, trace, boundary, randomizer, dbg)
        assert [r.hex() for r in proof["bqc_roots"]] == case["bqc_roots"] and proof["rdc_root"].hex() == case["rdc_root"], case["name"]
        assert extra["tz_root"] == tz_root
        assert sm.proof_digest(proof) == case["digest"], case["name"]
        if "proof" in case:
            assert mg.render(proof) == case["proof"]
        assert model.verify(proof, air, boundary, tz_root) == (True if true_output else "combination"), case["name"]
        if true_output:        # one changed value or path byte per section
            for key in ("bqc_points", "rdc_points", "tzc_points"):
                bad = dict(proof)
                bad[key] = [(proof[key][0] + 1) % P] + list(proof[key][1:])
                assert model.verify(bad, air, boundary, tz_root) is not True, key
            for key in ("bqc_paths", "rdc_paths", "tzc_paths"):
                bad = dict(proof)
                first = list(proof[key][0])
                first[-1] = bytes([first[-1][0] ^ 1]) + first[-1][1:]
                bad[key] = [first] + list(proof[key][1:])
                assert model.verify(bad, air, boundary, tz_root) is not True, key
            for key in ("bqc_roots",):
                bad = dict(proof)
                bad[key] = [bytes([proof[key][0][0] ^ 1]) + proof[key][0][1:]] + proof[key][1:]
                assert model.verify(bad, air, boundary, tz_root) is not True, key
            bad = dict(proof)
            bad["fri"] = dict(proof["fri"], last_codeword=[(proof["fri"]["last_codeword"][0] + 1) % P] + proof["fri"]["last_codeword"][1:])
            assert model.verify(bad, air, boundary, tz_root) == "fri"


def two_register(p, T, a, b, omicron):
    """trace of next0 = prev0^2 + prev1, next1 = prev0 prev1 + omicron^cycle, and the AIR over (X, prev0, prev1, next0, next1)"""
    rows, x = [[a % p, b % p]], 1
    for _ in range(T - 1):
        u, v = rows[-1]
        rows.append([(u * u + v) % p, (u * v + x) % p])
        x = x * omicron % p
    cons = [[(1, (0, 0, 0, 1, 0)), (p - 1, (0, 2, 0, 0, 0)), (p - 1, (0, 0, 1, 0, 0))],
            [(1, (0, 0, 0, 0, 1)), (p - 1, (0, 1, 1, 0, 0)), (p - 1, (1, 0, 0, 0, 0))]]
    return rows, cons


@pytest.mark.parametrize("fid,T", [(M128, 2000), (M128, 30000), (M128, 120000), (orc.FR, 2000)])
def test_quotient_stages_at_scale(env, fid, T):
    torch, mz, dev, st = env
    p, nl = orc.MOD[fid], orc.LIMBS[fid]
    checks, e = 17, 4
    lg = ((T + 4 * checks) * 2).bit_length()
    omicron, omega = orc.root_of(fid, lg), orc.root_of(fid, lg + 2)
    g = orc.M128_GEN if fid == M128 else 5
    rnd = random.Random(T + fid)
    rows, cons = two_register(p, T, 3, 4, omicron)
    boundary = [(0, 0, 3), (0, 1, 4), (T - 1, 0, rows[-1][0])]
    trace = rows + [[rnd.randrange(p) for _ in range(2)] for _ in range(4 * checks)]
    d = mz.stark_plan(fid, e, checks, 2, T, 2, cons, boundary)
    assert (d["omicron_domain_length"], d["fri_domain_length"]) == (1 << lg, 1 << (lg + 2))
    randomizer = [rnd.randrange(p) for _ in range(d["randomizer_length"])]
    proof, x = prove_staged(env, fid, p, g, omega, omicron, e, checks, 2, T, 2, cons, trace, boundary, randomizer)
    I = orc.from_limbs
    flen = d["fri_domain_length"]
    # (b) the committed boundary quotients: long division by the expanded zerofier in Python, the oracle's extension and Merkle commit
    for s in range(2):
        tp = I(x["tps"][s])
        q = sm.pdivmod(tp, sm.from_monomials(x["roots"][s], p), p)[0]
        assert I(x["bqs"][s]) == q
        rc, cw = orc.coset_ref(fid, orc.to_limbs(q, nl), g, omega, flen)
        assert rc == 0 and orc.merkle_commit_field_ref(fid, cw) == proof["bqc_roots"][s]
    # the trace polynomials interpolate the trace: spot values by Horner
    for k in (0, 1, T - 1, T + 4 * checks - 1):
        xk = pow(omicron, k, p)
        for s in range(2):
            assert orc.poly_eval(fid, x["tps"][s], xk) == trace[k][s]
    # the true boundary divides exactly: quotient * zerofier + interpolant = trace polynomial at a random point
    z = rnd.randrange(p)
    for s in range(2):
        pts = [(pow(omicron, c, p), v) for c, r, v in boundary if r == s]
        interp = mm.interpolate([a for a, _ in pts], [v for _, v in pts], p)
        zer = sm.from_monomials([a for a, _ in pts], p)
        assert (orc.poly_eval(fid, x["bqs"][s], z) * mm.peval(zer, z, p) + mm.peval(interp, z, p)) % p == orc.poly_eval(fid, x["tps"][s], z)
    # the transition quotients: quotient * zerofier = transition polynomial at random points (the division is exact for a real trace)
    for a in range(2):
        assert x["tqs"][a].shape[0] == x["tpolys"][a].shape[0] - (T - 1)
        for _ in range(2):
            z = rnd.randrange(p)
            assert orc.poly_eval(fid, x["tqs"][a], z) * orc.poly_eval(fid, x["tz"], z) % p == orc.poly_eval(fid, x["tpolys"][a], z)
    # (a) the model's verifier -- O(T) work per query -- accepts the proof and rejects one for a false boundary made by the same stages
    st_model = sm.FastStark(p, g, omega, omicron, e, checks, 2, T, 2)
    air = [{tuple(k): c for c, k in terms} for terms in cons]

    def zerofier_at(v):                         # prod_{i < T - 1} (v - omicron^i): the zerofier's value without its coefficients
        acc, w = 1, 1
        for _ in range(T - 1):
            acc, w = acc * (v - w) % p, w * omicron % p
        return acc
    assert orc.poly_eval(fid, x["tz"], 12345) == zerofier_at(12345)
    assert st_model.verify(proof, air, boundary, x["tz_root"], zerofier_at) is True
    false_boundary = boundary[:2] + [(T - 1, 0, (rows[-1][0] + 1) % p)]
    bad, _ = prove_staged(env, fid, p, g, omega, omicron, e, checks, 2, T, 2, cons, trace, false_boundary, randomizer)
    assert st_model.verify(bad, air, false_boundary, x["tz_root"], zerofier_at) == "combination"
    # (c) the stages are deterministic
    again, _ = prove_staged(env, fid, p, g, omega, omicron, e, checks, 2, T, 2, cons, trace, boundary, randomizer)
    assert sm.proof_digest(again) == sm.proof_digest(proof)
