"""FastStark (zkstark/fast_stark.rs) restated with Python integers on top of mpoly_model and fri_prove_model: the parameter
derivation (initialize_fast_stark_m128, the degree helpers), prove (fast_stark.rs:177-396) and verify (:398-571).  Literal where it
matters: the boundary quotient is (tp - interpolant) / zerofier by long division -- the library divides root by root and is checked
against this, not against itself -- fast_coset_divide is ntt.rs:271-330 step by step, the weights are sample_weights, the indices are
duplicated as the prover and the verifier each do it.  The caller supplies the random rows of the trace and the randomizer
polynomial, so prove is a pure function.  Needs no GPU and no library."""
import hashlib
import mpoly_model as mm
import fri_prove_model as fm

E_ARG, E_NOT_POW2, E_LENGTH = -1, -2, -5
MAX_REGISTERS, MAX_CONSTRAINTS = 3, 16
MAX_LOG = {mm.FR_P: 28, mm.M128_P: 32}


class PlanError(Exception):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


# ---- polynomial.rs -------------------------------------------------------------------------------------------------------------------
def pdivmod(a, b, p):
    """div_rem_ref (polynomial.rs:371-405): (quotient, remainder), both trimmed; the zero quotient when deg a < deg b"""
    a, b = mm.trim([v % p for v in a]), mm.trim([v % p for v in b])
    assert b, "division by the zero polynomial"
    if len(a) < len(b):
        return [], a
    rem, q = list(a), [0] * (len(a) - len(b) + 1)
    linv = pow(b[-1], -1, p)
    for d in range(len(a) - len(b), -1, -1):
        c = rem[d + len(b) - 1] * linv % p
        q[d] = c
        for i, v in enumerate(b):
            rem[d + i] = (rem[d + i] - c * v) % p
    return mm.trim(q), mm.trim(rem)


def from_monomials(roots, p):
    z = [1]
    for r in roots:
        z = mm.pmul(z, [(-r) % p, 1], p)
    return z


def div_roots(c, roots, p):
    """what mzk_poly_div_roots computes: one synthetic division per root, every remainder dropped"""
    c = mm.trim([v % p for v in c])
    for r in roots:
        if len(c) < 2:
            return []
        q, carry = [0] * (len(c) - 1), 0
        for k in range(len(c) - 1, 0, -1):
            carry = (c[k] + carry * r) % p
            q[k - 1] = carry
        c = q
    return mm.trim(c)


# ---- ntt.rs --------------------------------------------------------------------------------------------------------------------------
def ntt(root, values, p):
    """ntt (ntt.rs:7-48) as the transform it computes: out[i] = sum_j values[j] root^(i j)"""
    n = len(values)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * root % p
    return [sum(v * pw[i * j % n] for j, v in enumerate(values) if v) % p for i in range(n)]


def intt(root, values, p):
    n = len(values)
    ninv = pow(n, -1, p)
    return [v * ninv % p for v in ntt(pow(root, -1, p), values, p)]


def fast_coset_evaluate(poly, offset, generator, order, p):
    """ntt.rs:254-269"""
    return ntt(generator, mm.pscale(poly, offset, p) + [0] * (order - len(poly)), p)


def fast_coset_divide(lhs, rhs, offset, root, root_order, p):
    """ntt.rs:271-330; the result keeps lhs.degree() - rhs.degree() + 1 coefficients, as the reference's slice does"""
    lhs, rhs = mm.trim(lhs), mm.trim(rhs)
    assert pow(root, root_order, p) == 1 and pow(root, root_order // 2, p) != 1
    assert rhs and len(rhs) - 1 < len(lhs) - 1
    order = root_order
    degree = max(len(lhs), len(rhs)) - 1
    if degree < 8:
        return pdivmod(lhs, rhs, p)[0]
    while degree < order // 2:
        root, order = root * root % p, order // 2
    lc = ntt(root, mm.pscale(lhs, offset, p) + [0] * (order - len(lhs)), p)
    rc = ntt(root, mm.pscale(rhs, offset, p) + [0] * (order - len(rhs)), p)
    qc = [a * pow(b, p - 2, p) % p for a, b in zip(lc, rc)]                      # div_ref: el * r.inverse(), inverse(0) = 0
    q = intt(root, qc, p)[:len(lhs) - len(rhs) + 1]
    return mm.pscale(q, pow(offset, -1, p), p)


# ---- initialize_fast_stark_m128 and the degree helpers ---------------------------------------------------------------------------------
def plan(p, expansion_factor, checks, m, cycles, degree, constraints, boundary):
    """the numbers of mzk_stark_plan, in its words; constraints: lists of exponent tuples (or (coef, exps) terms, or MPolynomial dicts);
    boundary: (cycle, register[, value]).  Raises PlanError with the library's status code where the reference would panic."""
    if m > MAX_REGISTERS or not constraints or len(constraints) > MAX_CONSTRAINTS:
        raise PlanError(E_ARG, "registers / constraints out of range")
    if expansion_factor == 0 or expansion_factor & (expansion_factor - 1):
        raise PlanError(E_NOT_POW2, "expansion factor")
    nr = 4 * checks
    rl = cycles + nr
    if rl * degree >= 1 << 64 or cycles == 0:
        raise PlanError(E_LENGTH, "trace length")
    olen = 1 << (rl * degree).bit_length()
    flen = olen * expansion_factor
    if flen > 1 << MAX_LOG[p]:
        raise PlanError(E_LENGTH, "FRI domain beyond the transform size limit")
    exps = []
    for a in constraints:
        if isinstance(a, dict):
            exps.append(list(a.keys()))
        else:
            exps.append([t[1] if len(t) == 2 and isinstance(t[1], (tuple, list)) else t for t in a])
    pd = [1] + [rl - 1] * (2 * m)
    tdb = [max([sum(r * e for r, e in zip(pd, k)) for k in a] + [0]) for a in exps]
    if any(d >= 1 << 64 for d in tdb) or any(d < cycles - 1 for d in tdb):
        raise PlanError(E_LENGTH, "transition degree bound")
    tqdb = [d - (cycles - 1) for d in tdb]
    max_degree = (1 << len(format(max(tqdb), "b"))) - 1                          # format!("{:b}", md).len(): "0" has one digit
    if max_degree >= 1 << MAX_LOG[p]:
        raise PlanError(E_LENGTH, "max_degree")
    counts = [sum(1 for b in boundary if b[1] == s) for s in range(m)]
    if any(c > rl - 1 for c in counts):
        raise PlanError(E_LENGTH, "more boundary entries than the trace degree")
    bqdb = [rl - 1 - c for c in counts]
    if any(b > max_degree for b in bqdb):
        raise PlanError(E_LENGTH, "boundary quotient bound above max_degree")
    rounds = fm.num_rounds(flen, expansion_factor, checks)
    if rounds < 2:
        raise PlanError(E_LENGTH, "fewer than two FRI rounds")
    if checks > flen >> (rounds - 1):
        raise PlanError(E_ARG, "cannot sample more indices than available in last codeword")
    return {"num_randomizers": nr, "randomized_trace_length": rl, "omicron_domain_length": olen, "fri_domain_length": flen, "num_registers": m,
            "n_vars": 1 + 2 * m, "n_constraints": len(constraints), "max_degree": max_degree, "randomizer_length": max_degree + 1,
            "n_weights": 1 + 2 * len(constraints) + 2 * m, "fri_num_rounds": rounds, "fri_last_length": flen >> (rounds - 1), "num_indices": nr,
            "transition_degree_bounds": tdb, "transition_quotient_degree_bounds": tqdb, "transition_shifts": [max_degree - q for q in tqdb],
            "boundary_counts": counts, "boundary_quotient_degree_bounds": bqdb, "boundary_shifts": [max_degree - b for b in bqdb]}


def sample_weights(number, randomness, p):
    """fast_stark.rs:162-175: Blake2b-256(randomness || i as u64 LE), F::sample"""
    return [fm.sample(hashlib.blake2b(bytes(randomness) + fm.u64le(i), digest_size=32).digest()) % p for i in range(number)]


def fri_verify(p, proof, omega, offset, domain_length, expansion_factor, tests, points):
    """FRI::verify (fri.rs:262-400).  The reference does not compare proof.top_level_indices with its own sample (fri.rs:318-329) -- it
    uses the sample -- while fri_prove_model.verify compares the two; a FastStark proof carries the indices SORTED (fast_stark.rs:338),
    so the model is handed the sample it would draw itself."""
    rounds = fm.num_rounds(domain_length, expansion_factor, tests)
    stream = [[r] for r in proof["merkle_roots"]] + [[fm.leaf(int(v)) for v in proof["last_codeword"]]]
    own = dict(proof)
    own["top_level_indices"] = fm.sample_indices(fm.fiat_shamir(stream), domain_length >> 1, domain_length >> (rounds - 1), tests)
    return fm.verify(p, own, omega, offset, domain_length, expansion_factor, tests, points)


class FastStark:
    def __init__(self, p, generator, omega, omicron, expansion_factor, checks, m, cycles, degree):
        self.p, self.generator, self.e, self.t, self.m, self.T = p, generator, expansion_factor, checks, m, cycles
        self.nr = 4 * checks
        self.olen = 1 << ((cycles + self.nr) * degree).bit_length()
        self.flen = self.olen * expansion_factor
        self.omega, self.omicron = omega, omicron
        assert pow(omega, self.flen, p) == 1 and pow(omega, self.flen // 2, p) != 1
        assert pow(omicron, self.olen, p) == 1 and pow(omicron, self.olen // 2, p) != 1

    # preprocess (fast_stark.rs:52-75)
    def transition_zerofier(self):
        return from_monomials([pow(self.omicron, i, self.p) for i in range(self.T - 1)], self.p)

    def codeword(self, c):
        return fast_coset_evaluate(c, self.generator, self.omega, self.flen, self.p)

    def preprocess(self):
        tz = self.transition_zerofier()
        cw = self.codeword(tz)
        leaves = [fm.leaf(v) for v in cw]
        return tz, cw, fm.merkle_levels(leaves)[-1][0]

    def _bounds(self, air):
        pd = [1] + [self.T + self.nr - 1] * (2 * self.m)
        tdb = [max([sum(r * e for r, e in zip(pd, k)) for k in a] + [0]) for a in air]
        tqdb = [d - (self.T - 1) for d in tdb]
        return tqdb, (1 << len(format(max(tqdb), "b"))) - 1

    def boundary_roots(self, boundary):
        return [[pow(self.omicron, c, self.p) for c, r, _ in boundary if r == s] for s in range(self.m)]

    def boundary_interpolants(self, boundary):
        out = []
        for s in range(self.m):
            pts = [(pow(self.omicron, c, self.p), v) for c, r, v in boundary if r == s]
            out.append(mm.interpolate([x for x, _ in pts], [y for _, y in pts], self.p))
        return out

    def duplicate(self, top):
        """fast_stark.rs:338-346 on the sorted top-level indices"""
        dup = list(top) + [(i + self.e) % self.flen for i in top]
        return sorted(dup + [(i + self.flen // 2) % self.flen for i in dup])

    def prove(self, trace, boundary, air, randomizer):
        """trace: num_cycles + num_randomizers rows (the caller has appended the random ones); air: MPolynomial dicts; randomizer:
        max_degree + 1 coefficients.  Returns the FastStarkProof as a dict and, under "_debug", the intermediates a test may compare."""
        p = self.p
        assert len(trace) == self.T + self.nr
        stream = []
        dom = [pow(self.omicron, i, p) for i in range(len(trace))]
        tps = [mm.interpolate(dom, [row[s] for row in trace], p) for s in range(self.m)]
        roots, interp = self.boundary_roots(boundary), self.boundary_interpolants(boundary)
        bqs, exact = [], True
        for s in range(self.m):
            num = mm.padd(tps[s], [(-v) % p for v in interp[s]], p)
            q, rem = pdivmod(num, from_monomials(roots[s], p), p)
            exact = exact and not rem
            bqs.append(q)
        trees = []
        for q in bqs:
            cw = self.codeword(q)
            leaves = [fm.leaf(v) for v in cw]
            levels = fm.merkle_levels(leaves)
            trees.append((cw, leaves, levels))
            stream.append([levels[-1][0]])
        point = [[0, 1]] + tps + [mm.pscale(tp, self.omicron, p) for tp in tps]
        tpolys = [mm.evaluate_symbolic(a, point, p) for a in air]
        tz = self.transition_zerofier()
        tqs = [fast_coset_divide(tp, tz, self.generator, self.omicron, self.olen, p) for tp in tpolys]
        tqdb, max_degree = self._bounds(air)
        assert len(randomizer) == max_degree + 1
        r_cw = self.codeword(randomizer)
        r_leaves = [fm.leaf(v) for v in r_cw]
        r_levels = fm.merkle_levels(r_leaves)
        stream.append([r_levels[-1][0]])
        weights = sample_weights(1 + 2 * len(tqs) + 2 * len(bqs), fm.fiat_shamir(stream), p)
        polys, shifts = [list(randomizer)], [0]
        for i, q in enumerate(tqs):
            polys += [q, q]
            shifts += [0, max_degree - tqdb[i]]
        for s, q in enumerate(bqs):
            polys += [q, q]
            shifts += [0, max_degree - (len(trace) - 1 - len(roots[s]))]
        comb = mm.lincomb_reference(polys, weights, shifts, p)
        fri, _ = fm.prove(p, self.codeword(comb), self.omega, self.generator, self.e, self.t)
        fri["top_level_indices"] = sorted(fri["top_level_indices"])                # fast_stark.rs:338
        dup = self.duplicate(fri["top_level_indices"])
        tz_cw = self.codeword(tz)
        tz_leaves = [fm.leaf(v) for v in tz_cw]
        tz_levels = fm.merkle_levels(tz_leaves)
        pr = {"fri": fri, "bqc_roots": [t[2][-1][0] for t in trees], "bqc_points": [], "bqc_paths": [], "rdc_root": r_levels[-1][0]}
        for cw, leaves, levels in trees:
            for i in dup:
                pr["bqc_points"].append(cw[i])
                pr["bqc_paths"].append(fm.merkle_open(i, leaves, levels))
        pr["rdc_points"] = [r_cw[i] for i in dup]
        pr["rdc_paths"] = [fm.merkle_open(i, r_leaves, r_levels) for i in dup]
        pr["tzc_points"] = [tz_cw[i] for i in dup]
        pr["tzc_paths"] = [fm.merkle_open(i, tz_leaves, tz_levels) for i in dup]
        pr["_debug"] = {"trace_polynomials": tps, "boundary_quotients": bqs, "boundary_roots": roots, "boundary_exact": exact,
                        "transition_polynomials": tpolys, "transition_quotients": tqs, "weights": weights, "combination": comb, "indices": dup,
                        "max_degree": max_degree, "transition_zerofier_root": tz_levels[-1][0]}
        return pr

    def verify(self, pr, air, boundary, transition_zerofier_root, zerofier_at=None):
        """fast_stark.rs:398-571: True, or the name of the check that failed.  zerofier_at: x -> transition_zerofier().eval(x) by other means
        (the product over the roots: O(T) per query) for traces too long to expand the zerofier with quadratic Python products"""
        p = self.p
        stream = [[r] for r in pr["bqc_roots"]] + [[pr["rdc_root"]]]
        rl = 1 + max(c for c, _, _ in boundary) + self.nr                          # fast_stark.rs:412-416
        weights = sample_weights(1 + 2 * len(air) + 2 * self.m, fm.fiat_shamir(stream), p)
        pts = []
        if not fri_verify(p, pr["fri"], self.omega, self.generator, self.flen, self.e, self.t, pts):
            return "fri"
        pts.sort(key=lambda iv: iv[0])
        idx = [i for i, _ in pts]
        dup = sorted(idx + [(i + self.e) % self.flen for i in idx])
        ctr, leafs = 0, []
        for r in range(len(pr["bqc_roots"])):
            tmp = {}
            for i in dup:
                if ctr >= len(pr["bqc_points"]):
                    return "bqc length"
                tmp[i] = pr["bqc_points"][ctr]
                if not fm.merkle_verify(pr["bqc_roots"][r], i, pr["bqc_paths"][ctr], fm.leaf(tmp[i])):
                    return "bqc path"
                ctr += 1
            leafs.append(tmp)
        rz, tzv = {}, {}
        for c, i in enumerate(dup):
            rz[i] = pr["rdc_points"][c]
            if not fm.merkle_verify(pr["rdc_root"], i, pr["rdc_paths"][c], fm.leaf(rz[i])):
                return "rdc path"
        for c, i in enumerate(dup):
            tzv[i] = pr["tzc_points"][c]
            if not fm.merkle_verify(transition_zerofier_root, i, pr["tzc_paths"][c], fm.leaf(tzv[i])):
                return "tzc path"
        bz = [from_monomials(z, p) for z in self.boundary_roots(boundary)]
        bi = self.boundary_interpolants(boundary)
        bdb = [rl - 1 - (len(z) - 1) for z in bz]
        tqdb, max_degree = self._bounds(air)
        tz = self.transition_zerofier() if zerofier_at is None else None
        for ci, val in pts:
            x = self.generator * pow(self.omega, ci, p) % p
            ni = (ci + self.e) % self.flen
            xn = self.generator * pow(self.omega, ni, p) % p
            cur = [(leafs[s][ci] * mm.peval(bz[s], x, p) + mm.peval(bi[s], x, p)) % p for s in range(self.m)]
            nxt = [(leafs[s][ni] * mm.peval(bz[s], xn, p) + mm.peval(bi[s], xn, p)) % p for s in range(self.m)]
            point = [x] + cur + nxt
            terms = [rz[ci]]
            for s, a in enumerate(air):
                v = 0
                for k, c in a.items():
                    t = c
                    for pv, e in zip(point, k):
                        t = t * pow(pv, e, p) % p
                    v = (v + t) % p
                q = v * pow(mm.peval(tz, x, p) if zerofier_at is None else zerofier_at(x), p - 2, p) % p                    # self.transition_zerofier().eval(..), not the opened point
                terms += [q, q * pow(x, max_degree - tqdb[s], p) % p]
            for s in range(self.m):
                b = leafs[s][ci]
                terms += [b, b * pow(x, max_degree - bdb[s], p) % p]
            if sum(t * w for t, w in zip(terms, weights)) % p != val % p:
                return "combination"
        return True


def proof_digest(pr):
    """SHA3-256 over a canonical rendering of a proof dict (everything but "_debug"): what the golden file pins for the proofs it does
    not spell out"""
    def norm(v):
        if isinstance(v, (bytes, bytearray)):
            return bytes(v).hex()
        if isinstance(v, dict):
            return {k: norm(x) for k, x in sorted(v.items()) if k != "_debug"}
        if isinstance(v, (list, tuple)):
            return [norm(x) for x in v]
        return str(int(v))
    import json
    return hashlib.sha3_256(json.dumps(norm(pr), sort_keys=True).encode()).hexdigest()


STARK_SECTIONS = ("status", "fri", "indices", "bqc_roots", "rdc_root", "bqc_points", "rdc_points", "tzc_points", "bqc_paths", "rdc_paths",
                  "tzc_paths", "path_lens")


def proof_layout(limbs, dims):
    """({section: (offset, size)}, total) of the packed proof of mzk_stark_prove (include/mzk.h), sections 8-byte aligned"""
    flen, m, k = dims["fri_domain_length"], dims["num_registers"], dims["num_indices"]
    e, t = flen // dims["omicron_domain_length"], dims["num_randomizers"] // 4
    depth = flen.bit_length() - 1
    esz = 8 * limbs
    _, _, fri_total = fm.layout(limbs, flen, e, t)
    sizes = [8, fri_total, 8 * k, 32 * m, 32, esz * m * k, esz * k, esz * k, fm.PATH_STRIDE * m * k * depth, fm.PATH_STRIDE * k * depth,
             fm.PATH_STRIDE * k * depth, 8 * (m + 2) * k * depth]
    out, at = {}, 0
    for name, sz in zip(STARK_SECTIONS, sizes):
        out[name] = (at, sz)
        at += (sz + 7) & ~7
    return out, at
