"""Shapes and tables shared by the tests of the product sum-check (test_sumcheck_product_cases.py without a GPU,
test_gpu_sumcheck_product_matrix.py with one): the thresholds of mzk_sumcheck.hip and mzk_sumcheck_tx.h as the sources state them, the
launches a proof makes at a given size, and tables whose round-0 polynomial has a chosen shape -- differences at the field's edges, a
zero at one point between non-zero ones, a zero claimed sum.  Every builder takes a fixed seed.  No GPU, no library."""
import functools, os, random, re
import sumcheck_product_model as sm

P = sm.P
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myzkp_amd", "csrc")


# ---- thresholds ----------------------------------------------------------------------------------------------------------
def constexpr_ints(path):
    """{name: value} of every `constexpr int NAME = <decimal>` (several to a line allowed) of a source file"""
    out = {}
    for line in open(path):
        m = re.match(r"\s*constexpr\s+int\s+(.*);", line)
        if m:
            for name, value in re.findall(r"\b([A-Za-z_]\w*)\s*=\s*(\d+)\s*(?=,|$)", m.group(1).split("//")[0].strip()):
                out[name] = int(value)
    return out


def _need(table, path, names):
    missing = [n for n in names if n not in table]
    assert not missing, "%s no longer states %s as `constexpr int NAME = <decimal>`" % (os.path.basename(path), missing)
    return [table[n] for n in names]


_HIP, _TX = os.path.join(CSRC, "mzk_sumcheck.hip"), os.path.join(CSRC, "mzk_sumcheck_tx.h")
SC_TAIL_LOG, SC_THREADS, SC_MAX_WG, MLE_TILE_LOG = _need(constexpr_ints(_HIP), _HIP, ["SC_TAIL_LOG", "SC_THREADS", "SC_MAX_WG", "MLE_TILE_LOG"])
SCP_MAX_FACTORS, SCP_MAX_DEGREE, SCP_MAX_VARS = _need(constexpr_ints(_TX), _TX, ["SCP_MAX_FACTORS", "SCP_MAX_DEGREE", "SCP_MAX_VARS"])


def schedule(el):
    """((round-0 launches, later grid rounds, round ends, tail launches), trips): what one proof over 2^el entries per factor
    launches, and for every grid round j the iterations a lane of k_sc_round makes over the 2^(el-1-j) index pairs"""
    j0 = max(el - SC_TAIL_LOG, 0)
    trips = []
    for j in range(j0):
        h = 1 << (el - 1 - j)
        nwg = min(-(-h // SC_THREADS), SC_MAX_WG)
        trips.append(-(-h // (nwg * SC_THREADS)))
    return (1 if j0 > 0 else 0, max(j0 - 1, 0), j0, 1), trips


# (el, k, d, the grid rounds in which a lane must make more than one trip): round 0 strides without a fold, the later ones fold and
# store inside the loop
STRIDE_CASES = ((20, 2, 2, (0,)), (21, 2, 2, (0, 1)), (21, 5, 4, (0, 1)))


# ---- tables --------------------------------------------------------------------------------------------------------------
def uniform(el, k, seed):
    rng = random.Random(seed)
    return [[rng.randrange(P) for _ in range(1 << el)] for _ in range(k)]


CORNERS = (0, 1, P - 2, P - 1)


def corners(el, k, seed):
    """every entry one of 0, 1, p - 2, p - 1: the differences of round 0 are 0, +-1, +-(p - 2), +-(p - 1), +-(p - 3)"""
    rng = random.Random(seed)
    return [[CORNERS[rng.randrange(4)] for _ in range(1 << el)] for _ in range(k)]


def root_at(el, k, c, seed):
    """uniform tables with factor c mod k bent so that its round-0 line vanishes at c for every index pair: s_0(c) = 0 exactly"""
    tables = uniform(el, k, seed)
    t, h = tables[c % k], 1 << (el - 1)
    if c == 0:
        t[:h] = [0] * h
    elif c == 1:
        t[h:] = [0] * h
    else:
        q = (c - 1) * pow(c, -1, P) % P              # a + c (a q - a) = a (1 + (c - 1) - c) = 0
        t[h:] = [a * q % P for a in t[:h]]
    return tables


def zero_sum(el, seed):
    """one factor with T[i + h] = -T[i]: the claimed sum s_0(0) + s_0(1) is 0, s_0(c) = (1 - 2 c) s_0(0) is not"""
    lower = uniform(el - 1, 1, seed)[0]
    return [lower + [(P - a) % P for a in lower]]


def impulse(el, t):
    """the coefficient vector of the single monomial t: its table is 1 at every b that contains t and 0 elsewhere"""
    coef = [0] * (1 << el)
    coef[t] = 1
    return coef


def impulse_indices(el):
    """monomials on every side of the passes of k_mle_pass: the lowest and highest bit of each pass, and one spread over all of them"""
    a, b = MLE_TILE_LOG, 2 * MLE_TILE_LOG - 2         # the first bit of the second and of the third pass (cb = 2 from the second on)
    ts = (0, 1, 1 << (a - 1), 1 << a, 1 << (b - 1), 1 << b, 1 << (el - 1), (1 << el) - 1, (1 << a) + (1 << b) + 1)
    return tuple(dict.fromkeys(ts))                   # 2^b is 2^(el - 1) at the smallest size with three passes


# ---- bytes ---------------------------------------------------------------------------------------------------------------
def packed(values):
    """canonical values as the library takes them: 32 bytes each, little-endian (np.frombuffer(..., uint64).reshape(-1, 4))"""
    return b"".join(v.to_bytes(32, "little") for v in values)


ZERO_RECORD = (1).to_bytes(8, "little") + (9).to_bytes(8, "little") + bytes(9)      # vec![bincode(0)]: NoSign, no digit


def zero_objects(transcript, header_objects=0):
    """the indices, counted from the first round's first object, of the pushed values that are zero"""
    objs = sm.deserialize_stream(transcript)[header_objects:]
    return [i for i, o in enumerate(objs) if o == [bytes(9)]]


def record_offset(transcript, index, header_objects=0):
    """the byte offset in the stream of pushed value `index` (every object after the header is one string)"""
    objs = sm.deserialize_stream(transcript)
    return 8 + sum(8 + sum(8 + len(s) for s in o) for o in objs[:header_objects + index])


# ---- a verifier for every (k, d) ---------------------------------------------------------------------------------------------
def product_sum(tables):
    """sum over the index of the product of the factors, linear in the table size"""
    total = 0
    for vals in zip(*tables):
        prod = vals[0]
        for v in vals[1:]:
            prod = prod * v % P
        total += prod
    return total % P


def verify_exact(tables, d, header, claimed, proof, full_below=0):
    """sm.verify for any (k, d).  The reference's verifier stands in for s_j(r_j) with the polynomial through the d + 1 pushed
    points, which is s_j only when d >= k: below that it rejects the honest prover's stream (the model's own proofs included;
    test_sumcheck_product_cases.py shows it).  Here s_j(r_j) is what it is by definition, the product sum of the tables folded with
    r_0 .. r_j, at linear cost in all; where d >= k the interpolated value must agree with it as well, so nothing sm.verify asks is
    dropped.  Rounds with at most full_below live entries per factor have all d + 1 points compared with sm.round_evals.
    Returns None on any mismatch, else {"challenges", "finals"} as recomputed from the stream and the tables."""
    el = len(tables[0]).bit_length() - 1
    k = len(tables)
    try:
        objects = sm.deserialize_stream(proof)
    except AssertionError:
        return None
    header = [list(o) for o in header]
    if len(objects) != len(header) + el * (d + 1) or objects[:len(header)] != header:
        return None
    at, want, cur, challenges = len(header), claimed % P, tables, []
    for _ in range(el):
        try:
            s = [sm.unleaf(o[0]) for o in objects[at:at + d + 1]]
        except AssertionError:
            return None
        if any(len(o) != 1 for o in objects[at:at + d + 1]) or any(not 0 <= v < P for v in s) or (s[0] + s[1]) % P != want:
            return None
        if len(cur[0]) <= full_below and s != sm.round_evals(cur, d):
            return None
        at += d + 1
        r = sm.challenge(objects[:at])
        challenges.append(r)
        cur = [sm.fold(t, r) for t in cur]
        want = product_sum(cur)
        if d >= k and sm.interpolate_eval(s, r) != want:
            return None
    return {"challenges": challenges, "finals": [t[0] for t in cur]}


# ---- model proofs, computed once and never modified ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables_of(kind, el, k, arg=0):
    """the tables of a named case; arg is the root for "root", unused otherwise.  The seed is a function of the shape alone."""
    seed = 7919 * el + 31 * k + arg
    if kind == "uniform":
        return uniform(el, k, seed)
    if kind == "corners":
        return corners(el, k, seed)
    if kind == "root":
        return root_at(el, k, arg, seed)
    if kind == "zero_sum":
        assert k == 1
        return zero_sum(el, seed)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def proof_of(kind, el, k, d, arg=0, header_kind="none"):
    """(tables, header objects, sm.prove of them)"""
    tables = tables_of(kind, el, k, arg)
    header = ()
    if header_kind == "reference":
        rng = random.Random(el + 100 * k + 10000 * d)
        header = tuple(tuple(o) for o in sm.reference_header(d, k, el, [bytes(rng.randrange(256) for _ in range(3 + 5 * f)) for f in range(k)]))
    return tables, header, sm.prove(tables, d, header)


# the value cases of test_gpu_sumcheck_product_matrix.py, section c: (kind, el, k, d, arg)
CORNER_CASES = tuple(("corners", el, k, d, 0) for el in (5, 9) for k, d in ((8, 8), (3, 5)))
ROOT_CASES = tuple(("root", el, 3, 4, c) for el in (6, 9) for c in range(5))
ZERO_SUM_CASES = tuple(("zero_sum", el, 1, 2, 0) for el in (6, 9))
