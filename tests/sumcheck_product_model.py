"""The product sum-check of examples/sumcheck (prover.rs:98-247 with the *_cpu twins of utils.rs, verifier.rs:15-76) restated with
Python integers and hashlib over BN254 Fr: k multilinear factors as evaluation tables over {0,1}^el (variable 0 = the most
significant index bit), the reference's proof stream (fri_prove_model: bincode 1.x of Vec<Vec<Vec<u8>>>, SHAKE256, F::sample), and
evals_over_boolean_hypercube for dense multilinear coefficients.  Values are canonical representatives in [0, p).  No GPU, no library."""
import fri_prove_model as fm

P = fm.P_FR
SECTIONS = ("status", "sum", "evals", "challenges", "finals", "transcript_len", "transcript")
RECORD_MAX = 16 + 41


# ---- the stream ----------------------------------------------------------------------------------------------------------
def reference_header(max_degree, num_factors, num_variables, factor_bytes):
    """the objects the reference pushes before round 0: three bincode(usize), then bincode(MPolynomial) of every factor (any bytes)"""
    return [[fm.u64le(max_degree)], [fm.u64le(num_factors)], [fm.u64le(num_variables)]] + [[bytes(b)] for b in factor_bytes]


def frame_header(objects):
    """objects (lists of byte strings) in stream form, concatenated: the serialization without the leading object count"""
    return fm.serialize_stream(objects)[8:]


def deserialize_stream(raw):
    raw = bytes(raw)
    at = 8
    objects = []
    for _ in range(int.from_bytes(raw[:8], "little")):
        cnt = int.from_bytes(raw[at:at + 8], "little")
        at += 8
        obj = []
        for _ in range(cnt):
            ln = int.from_bytes(raw[at:at + 8], "little")
            at += 8
            assert at + ln <= len(raw)
            obj.append(raw[at:at + ln])
            at += ln
        objects.append(obj)
    assert at == len(raw)
    return objects


def unleaf(b):
    """bincode(FiniteFieldElement) back to the int"""
    sign, cnt = b[0], int.from_bytes(b[1:9], "little")
    assert len(b) == 9 + 4 * cnt
    mag = sum(int.from_bytes(b[9 + 4 * i:13 + 4 * i], "little") << (32 * i) for i in range(cnt))
    return -mag if sign == 0xFF else mag


def challenge(stream):
    return fm.sample(fm.fiat_shamir(stream, 32))


# ---- tables --------------------------------------------------------------------------------------------------------------
def evals_over_boolean_hypercube(coef, el):
    """dense multilinear coefficients (coef[t] multiplies prod of x_i over the set bits (el-1-i) of t) -> evals[b] = sum_{t subset b}"""
    x = [c % P for c in coef]
    assert len(x) == 1 << el
    for s in range(el):
        bit = 1 << s
        for i in range(len(x)):
            if i & bit:
                x[i] = (x[i] + x[i ^ bit]) % P
    return x


def eval_monomials_direct(coef, el, b):
    """the polynomial of `coef` at the boolean point whose variable i is bit (el-1-i) of b, monomial by monomial"""
    total = 0
    for t, c in enumerate(coef):
        term = c
        for i in range(el):
            if (t >> (el - 1 - i)) & 1:
                term = term * ((b >> (el - 1 - i)) & 1)
        total += term
    return total % P


def fold(table, r):
    h = len(table) // 2
    return [(a + r * (b - a)) % P for a, b in zip(table[:h], table[h:])]


def claimed_sum(tables):
    total = 0
    for x in range(len(tables[0])):
        prod = 1
        for t in tables:
            prod = prod * t[x] % P
        total += prod
    return total % P


def round_evals(tables, d):
    h = len(tables[0]) // 2
    out = []
    for c in range(d + 1):
        total = 0
        for i in range(h):
            prod = 1
            for t in tables:
                prod = prod * (t[i] + c * (t[i + h] - t[i])) % P
            total += prod
        out.append(total % P)
    return out


# ---- prover / verifier ---------------------------------------------------------------------------------------------------
def prove(tables, d, header=()):
    """tables: k lists of 2^el ints in [0, p).  header: the objects pushed before round 0.  Returns the packed proof's contents."""
    n = len(tables[0])
    el = n.bit_length() - 1
    assert el >= 1 and all(len(t) == n for t in tables)
    stream = [list(o) for o in header]
    cur = [list(t) for t in tables]
    evals, challenges, lengths = [], [], []
    for _ in range(el):
        s = round_evals(cur, d)
        evals.append(s)
        for v in s:
            stream.append([fm.leaf(v)])
        lengths.append(len(fm.serialize_stream(stream)))
        r = challenge(stream)
        challenges.append(r)
        cur = [fold(t, r) for t in cur]
    return {"sum": claimed_sum(tables), "evals": evals, "challenges": challenges, "finals": [t[0] for t in cur],
            "transcript": fm.serialize_stream(stream), "hashed_lengths": lengths}


def interpolate_eval(ys, x):
    """the polynomial through (0, ys[0]) .. (d, ys[d]) at x"""
    total = 0
    for i, y in enumerate(ys):
        num, den = 1, 1
        for j in range(len(ys)):
            if j != i:
                num = num * (x - j) % P
                den = den * (i - j) % P
        total += y * num * pow(den, -1, P)
    return total % P


def verify(tables, d, header, claimed, proof, finals=None):
    """verifier.rs:15-76; the factors are given as their tables (the product is evaluated at the challenges by folding).  finals: the
    factors at the proof's challenges when the caller has folded the tables already (the challenges are then not re-folded)"""
    el = len(tables[0]).bit_length() - 1
    try:
        objects = deserialize_stream(proof)
    except AssertionError:
        return False
    header = [list(o) for o in header]
    if len(objects) != len(header) + el * (d + 1) or objects[:len(header)] != header:
        return False
    at = len(header)
    challenges, prev = [], None
    for i in range(el):
        try:
            s = [unleaf(objects[at + c][0]) % P for c in range(d + 1)]
        except (AssertionError, IndexError):
            return False
        at += d + 1
        r = challenge(objects[:at])
        want = claimed % P if i == 0 else interpolate_eval(prev, challenges[-1])
        if (s[0] + s[1]) % P != want:
            return False
        challenges.append(r)
        prev = s
    if finals is None:
        cur = [list(t) for t in tables]
        for r in challenges:
            cur = [fold(t, r) for t in cur]
        finals = [t[0] for t in cur]
    prod = 1
    for v in finals:
        prod = prod * v % P
    return prod == interpolate_eval(prev, challenges[-1])


# ---- the packed proof of mzk_sumcheck_product_prove (include/mzk.h) ----------------------------------------------------------
def transcript_cap(el, d, header_len):
    return 8 + header_len + el * (d + 1) * RECORD_MAX


def layout(el, k, d, header_len):
    sizes = [8, 32, 32 * el * (d + 1), 32 * el, 32 * k, 8, transcript_cap(el, d, header_len)]
    sec, at = {}, 0
    for name, s in zip(SECTIONS, sizes):
        sec[name] = (at, s)
        at += (s + 7) & ~7
    return sec, at
