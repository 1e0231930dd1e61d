"""FRI::prove and FRI::verify (zkstark/fri.rs:19-400) restated with Python integers and hashlib, with the reference's REAL proof
stream: FiatShamirTransformer (algebra/fiat_shamir.rs) = bincode 1.x of Vec<Vec<Vec<u8>>> hashed with SHAKE256, F::sample
(field.rs:272-278), sample_indices with Blake2b-256 (fri.rs:19-62).  Merkle trees are SHA3-256 over bincode(FiniteFieldElement)
leaves (algebra/merkle.rs:15-46) in the library's restatement of that layout (sign byte, u64 digit count, u32 digits; not pinned
against a Rust vector).  Used by tests/golden/make_golden_fri_prove.py and the FRI prove tests; needs no GPU and no library."""
import hashlib

P_FR = 21888242871839275222246405745257275088548364400416034343698204186575808495617
P_M128 = 270497897142230380135924736767050121217
MASK64 = (1 << 64) - 1


# ---- bincode -----------------------------------------------------------------------------------------------------------
def u64le(x):
    return int(x).to_bytes(8, "little")


def leaf(v):
    """bincode(FiniteFieldElement) of the BigInt v: Sign (Minus = 0xff, NoSign = 0, Plus = 1), u64 digit count, u32 LE digits"""
    mag = abs(v)
    digits = []
    while mag:
        digits.append(mag & 0xFFFFFFFF)
        mag >>= 32
    sign = 0 if v == 0 else (0xFF if v < 0 else 1)
    return bytes([sign]) + u64le(len(digits)) + b"".join(d.to_bytes(4, "little") for d in digits)


def serialize_stream(objects):
    """bincode::serialize(&Vec<Vec<Vec<u8>>>): u64 object count, per object u64 string count, per string u64 length + bytes"""
    out = [u64le(len(objects))]
    for obj in objects:
        out.append(u64le(len(obj)))
        for s in obj:
            out.append(u64le(len(s)) + bytes(s))
    return b"".join(out)


def fiat_shamir(objects, num_bytes=32):                 # prover_fiat_shamir / verifier_fiat_shamir on the pulled prefix
    return hashlib.shake_256(serialize_stream(objects)).digest(num_bytes)


def sample(byte_array):                                  # F::sample / sample_index before `% size`: usize wraps at 2^64
    acc = 0
    for b in byte_array:
        acc = ((acc << 8) ^ b) & MASK64
    return acc


def num_rounds(domain_length, expansion_factor, num_colinearity_tests):      # fri.rs:86-97
    n, r = domain_length, 0
    while n > expansion_factor and 4 * num_colinearity_tests < n:
        n //= 2
        r += 1
    return r


def sample_indices(seed, size, reduced_size, number, limit=None):           # fri.rs:27-62
    assert number <= reduced_size, "cannot sample more indices than available in last codeword"
    indices, reduced, counter = [], set(), 0
    while len(indices) < number:
        if limit is not None and counter >= limit:
            return None
        h = hashlib.blake2b(bytes(seed) + u64le(counter), digest_size=32).digest()
        index = sample(h) % size
        counter += 1
        if index % reduced_size not in reduced:
            indices.append(index)
            reduced.add(index % reduced_size)
    return indices


# ---- Merkle (merkle.rs) ------------------------------------------------------------------------------------------------
def _h(b):
    return hashlib.sha3_256(b).digest()


def merkle_levels(leaves):
    """power-of-two leaf count >= 2: [level 1, level 2, ..., [root]]"""
    lv = [_h(leaves[2 * i] + leaves[2 * i + 1]) for i in range(len(leaves) // 2)]
    out = [lv]
    while len(lv) > 1:
        lv = [_h(lv[2 * i] + lv[2 * i + 1]) for i in range(len(lv) // 2)]
        out.append(lv)
    return out


def merkle_open(index, leaves, levels):                  # Merkle::open: sibling leaf, then sibling digests bottom-up
    path = [leaves[index ^ 1]]
    for l in range(1, len(levels)):
        path.append(levels[l - 1][(index >> l) ^ 1])
    return path


def merkle_verify(root, index, path, lf):                # Merkle::verify (merkle.rs:48-66)
    if len(path) == 1:
        return root == (_h(lf + path[0]) if index == 0 else _h(path[0] + lf))
    nxt = _h(lf + path[0]) if index % 2 == 0 else _h(path[0] + lf)
    return merkle_verify(root, index >> 1, path[1:], nxt)


# ---- FRI::prove (fri.rs:99-260) -----------------------------------------------------------------------------------------
def prove(p, codeword, omega, offset, expansion_factor, tests):
    """codeword: list of ints; a negative int is an element the reference left negative (Sign::Minus, magnitude -v).  Returns
    (proof dict in fri_unpack_proof's shape, the serialized proof stream)."""
    n = len(codeword)
    rounds = num_rounds(n, expansion_factor, tests)
    assert rounds >= 2
    stream, roots, codewords, trees = [], [], [], []
    two_inv = pow(2, -1, p)
    cw = list(codeword)
    for r in range(rounds):                                                      # commit, fri.rs:144-209
        leaves = [leaf(v) for v in cw]
        levels = merkle_levels(leaves)
        root = levels[-1][0]
        roots.append(root)
        stream.append([root])
        codewords.append(cw)
        trees.append((leaves, levels))
        if r == rounds - 1:
            break
        alpha = sample(fiat_shamir(stream)) % p
        h = len(cw) // 2
        nxt = []
        for i in range(h):
            q = alpha * pow(offset * pow(omega, i, p) % p, -1, p) % p
            nxt.append(two_inv * ((1 + q) * cw[i] + (1 - q) * cw[h + i]) % p)   # % p: sanitize
        cw, omega, offset = nxt, omega * omega % p, offset * offset % p
    stream.append([leaf(v) for v in cw])                                         # send the last codeword
    top = sample_indices(fiat_shamir(stream), n // 2, len(cw), tests)
    layers, indices = [], list(top)
    for i in range(rounds - 1):                                                   # query phase + reveal, fri.rs:127-137, 211-260
        half = len(codewords[i]) // 2
        indices = [idx % half for idx in indices]
        a, b = list(indices), [idx + half for idx in indices]
        (lc, vc), (ln, vn) = trees[i], trees[i + 1]
        layers.append({"a": ([codewords[i][j] for j in a], [merkle_open(j, lc, vc) for j in a]),
                       "b": ([codewords[i][j] for j in b], [merkle_open(j, lc, vc) for j in b]),
                       "c": ([codewords[i + 1][j] for j in a], [merkle_open(j, ln, vn) for j in a])})
    return {"top_level_indices": top, "last_codeword": cw, "merkle_roots": roots, "revealed_layers": layers}, serialize_stream(stream)


# ---- FRI::verify (fri.rs:262-400) ---------------------------------------------------------------------------------------
def _interpolate_degree(p, xs, ys):
    """degree of the Lagrange interpolant through (xs, ys) -- the last codeword's low-degree check (fri.rs:300-318)"""
    n = len(xs)
    coef = [0] * n
    full = [1]                                                                   # prod_j (X - x_j), ascending
    for x in xs:
        full = [(a - x * b) % p for a, b in zip([0] + full, full + [0])]
    for i in range(n):
        num, carry, den = [0] * n, 0, 1                                          # full / (X - x_i) by synthetic division (quadratic in all)
        for k in range(n, 0, -1):
            carry = (full[k] + carry * xs[i]) % p
            num[k - 1] = carry
        for j in range(n):
            if j != i:
                den = den * (xs[i] - xs[j]) % p
        s = ys[i] * pow(den, -1, p) % p
        coef = [(c + s * t) % p for c, t in zip(coef, num)]
    d = n - 1
    while d >= 0 and coef[d] == 0:
        d -= 1
    return d


def verify(p, proof, omega, offset, domain_length, expansion_factor, tests, points=None):
    rounds = num_rounds(domain_length, expansion_factor, tests)
    roots = proof["merkle_roots"]
    stream, alphas = [], []
    for root in roots:                                                           # fri.rs:268-276
        stream.append([root])
        alphas.append(sample(fiat_shamir(stream)) % p)
    last = [int(v) for v in proof["last_codeword"]]
    stream.append([leaf(v) for v in last])
    if merkle_levels([leaf(v) for v in last])[-1][0] != roots[-1]:
        return False
    degree = len(last) // expansion_factor - 1
    last_omega, last_offset = pow(omega, 1 << (rounds - 1), p), pow(offset, 1 << (rounds - 1), p)
    xs = [last_offset * pow(last_omega, i, p) % p for i in range(len(last))]
    if _interpolate_degree(p, xs, last) > degree:
        return False
    top = sample_indices(fiat_shamir(stream), domain_length >> 1, domain_length >> (rounds - 1), tests)
    if top != proof["top_level_indices"]:
        return False
    for r in range(rounds - 1):
        c_idx = [i % (domain_length >> (r + 1)) for i in top]
        a_idx, b_idx = c_idx, [i + (domain_length >> (r + 1)) for i in c_idx]
        L = proof["revealed_layers"][r]
        for s in range(tests):
            ay, by, cy = L["a"][0][s] % p, L["b"][0][s] % p, L["c"][0][s] % p
            if r == 0 and points is not None:
                points += [(a_idx[s], ay), (b_idx[s], by)]
            ax, bx, cx = offset * pow(omega, a_idx[s], p) % p, offset * pow(omega, b_idx[s], p) % p, alphas[r]
            if (by - ay) * (cx - ax) % p != (cy - ay) * (bx - ax) % p:
                return False
        for s in range(tests):
            if not merkle_verify(roots[r], a_idx[s], L["a"][1][s], leaf(L["a"][0][s])):
                return False
            if not merkle_verify(roots[r], b_idx[s], L["b"][1][s], leaf(L["b"][0][s])):
                return False
            if not merkle_verify(roots[r + 1], c_idx[s], L["c"][1][s], leaf(L["c"][0][s])):
                return False
        omega, offset = omega * omega % p, offset * offset % p
    return True


# ---- the packed proof of mzk_fri_prove (include/mzk.h) ------------------------------------------------------------------
SECTIONS = ("status", "top_indices", "roots", "last_codeword", "values", "signs", "paths", "path_lens")
PATH_STRIDE = 48


def layout(limbs, n, expansion_factor, tests):
    """(num_rounds, {section: (offset, size)}, total): the packed proof's sections, each 8-byte aligned"""
    R = num_rounds(n, expansion_factor, tests)
    m, L = n >> (R - 1), R - 1
    d = [(n >> r).bit_length() - 1 for r in range(R)]
    entries = sum(tests * (2 * d[i] + d[i + 1]) for i in range(L))
    sizes = [8, 8 * tests, 32 * R, 8 * limbs * m, 8 * limbs * 3 * tests * L, 3 * tests * L, PATH_STRIDE * entries, 8 * entries]
    out, at = {}, 0
    for k, s in zip(SECTIONS, sizes):
        out[k] = (at, s)
        at += (s + 7) & ~7
    return R, out, at
