"""ctypes loader + thin wrappers for include/mzk.h.  Arrays are numpy uint64, shape (n, limbs)."""
import ctypes, os
import numpy as np
from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.environ.get("MZK_HIP_LIB") or os.path.join(HERE, "libmzk_hip.so")   # MZK_HIP_LIB: experimental builds (tools/)

_C = _abi.constants()        # every NAME = integer of the header's enums
FIELD_FR, FIELD_M128, FIELD_FQ = _C["MZK_FIELD_FR"], _C["MZK_FIELD_M128"], _C["MZK_FIELD_FQ"]
# Goldilocks (p = 2^64 - 2^32 + 1) and its cubic extension F_p[x] / (x^3 - x + 1): one / three canonical u64 per element.  A scalar
# extension element is an int packed as c0 + c1 * 2^64 + c2 * 2^128 (what to_limbs / from_limbs do with three limbs).
FIELD_M64, FIELD_M64X3 = _C["MZK_FIELD_M64"], _C["MZK_FIELD_M64X3"]
LIMBS = {FIELD_FR: 4, FIELD_M128: 2, FIELD_FQ: 4, FIELD_M64: 1, FIELD_M64X3: 3}
MODULUS = {
    FIELD_FR: 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    FIELD_M128: 270497897142230380135924736767050121217,
    FIELD_FQ: 21888242871839275222246405745257275088696311157297823662689037894645226208583,
    FIELD_M64: (1 << 64) - (1 << 32) + 1,
    FIELD_M64X3: (1 << 64) - (1 << 32) + 1,        # of every coefficient
}


def _leaf_stride(fid):
    """bytes that hold any leaf of the field: 41 for Fr, 59 for an M64X3 element"""
    return 64 if fid == FIELD_M64X3 else 48
ERRORS = {v: k for k, v in _C.items() if k == "MZK_OK" or k.startswith("MZK_E_")}


class MzkError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERRORS.get(code, "?"), code, msg))
        self.code = code
        self.message = msg


_lib = None


DECLARED_SYMBOLS = sorted(name for name, _, _ in _abi.c_prototypes())


def lib():
    """Load the HIP library; fail loudly if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(SO):
            raise ImportError("myzkp_amd/libmzk_hip.so is missing: run `python -m myzkp_amd.build` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64.  Two HIP runtimes in one process
        # cannot both own the GPU, and whichever is loaded first wins the SONAME: load torch's first (when torch
        # is installed) so that this library binds to the same runtime and device tensors can be shared.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        _lib = _abi.bind(ctypes.CDLL(SO))       # argtypes and restype of every entry point, from the header: callers pass plain values
    return _lib


def exported_symbols():
    l = lib()
    return [s for s in DECLARED_SYMBOLS if hasattr(l, s)]


def _check(rc):
    if rc != 0:
        raise MzkError(rc, lib().mzk_last_error().decode())


def init(device=0):
    _check(lib().mzk_init(int(device)))


def set_workspace_budget(nbytes):
    """bytes of scratch a context may keep between calls (0 = no limit); idle buffers above it are released at once"""
    _check(lib().mzk_set_workspace_budget(int(nbytes)))


def trim_workspace():
    """release every workspace buffer and cached transform plan of every context; returns the workspace bytes given back"""
    out = ctypes.c_size_t(0)
    _check(lib().mzk_trim_workspace(ctypes.byref(out)))
    return out.value


def workspace_bytes():
    out = ctypes.c_size_t(0)
    _check(lib().mzk_workspace_bytes(ctypes.byref(out)))
    return out.value


def shutdown():
    lib().mzk_shutdown()


def init_devices(ordinals):
    """One process driving several GPUs: context r = ordinals[r] (duplicates allowed).  Context 0 becomes current."""
    arr = (ctypes.c_int * len(ordinals))(*[int(o) for o in ordinals])
    _check(lib().mzk_init_devices(arr, len(ordinals)))


def ctx_count():
    return int(lib().mzk_ctx_count())


def ctx_select(index):
    _check(lib().mzk_ctx_select(int(index)))


def shard_range(n, rank, world):
    lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
    lib().mzk_shard_range(n, int(rank), int(world), ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def to_limbs(vals, nl):
    a = np.zeros((len(vals), nl), dtype=np.uint64)
    for i, v in enumerate(vals):
        v = int(v)
        for j in range(nl):
            a[i, j] = (v >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
    return a


def from_limbs(a):
    a = np.asarray(a, dtype=np.uint64)
    a = a.reshape(-1, a.shape[-1])
    return [sum(int(a[i, j]) << (64 * j) for j in range(a.shape[1])) for i in range(a.shape[0])]


def points_to_array(pts):
    a = np.zeros((len(pts), 8), dtype=np.uint64)
    for i, p in enumerate(pts):
        a[i, :4] = to_limbs([p[0]], 4)[0]
        a[i, 4:] = to_limbs([p[1]], 4)[0]
    return a


def array_to_points(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 8)
    return [(from_limbs(a[i:i + 1, :4])[0], from_limbs(a[i:i + 1, 4:])[0]) for i in range(a.shape[0])]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _one(fid, v):
    return to_limbs([v], LIMBS[fid])


def _arr(fid, a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a.reshape(-1, LIMBS[fid])


def ntt(fid, root, values, inverse=False):
    """ntt::ntt / ntt::intt (algebra/ntt.rs:7-64)."""
    v = _arr(fid, values)
    out = np.empty_like(v)
    r = _one(fid, root)
    _check(lib().mzk_ntt(fid, _p(r), _p(v), _p(out), v.shape[0], int(bool(inverse))))
    return out


def intt(fid, root, values):
    return ntt(fid, root, values, inverse=True)


def merkle_commit_field_batch(fid, codewords):
    """Merkle::commit of every row of `codewords` (batch x n x limbs, n a power of two): list of 32-byte roots."""
    c = np.ascontiguousarray(codewords, dtype=np.uint64)
    batch = c.shape[0]
    if batch == 0:
        return []
    c = c.reshape(batch, -1, LIMBS[fid])
    roots = (ctypes.c_uint8 * (32 * batch))()
    _check(lib().mzk_merkle_commit_field_batch(fid, _p(c), c.shape[1], batch, roots))
    raw = bytes(roots)
    return [raw[32 * k: 32 * k + 32] for k in range(batch)]


def coset_lde_batch(fid, coefs, offset, generator, order):
    """ntt::fast_coset_evaluate of every row of `coefs` (batch x n_coef x limbs) onto one coset: mzk_coset_lde_batch."""
    c = np.ascontiguousarray(coefs, dtype=np.uint64)
    batch = c.shape[0]
    c = c.reshape(batch, -1, LIMBS[fid]) if batch else c.reshape(0, 0, LIMBS[fid])
    out = np.empty((batch, order, LIMBS[fid]), dtype=np.uint64)
    _check(lib().mzk_coset_lde_batch(fid, _p(c), c.shape[1], _p(_one(fid, offset)), _p(_one(fid, generator)), _p(out), order, batch))
    return out


def ntt_batch(fid, root, columns, inverse=False):
    """ntt::ntt / ntt::intt of every row of `columns` (batch x n x limbs) in one launch per pass: mzk_ntt_batch."""
    v = np.ascontiguousarray(columns, dtype=np.uint64)
    batch = v.shape[0]
    if batch == 0:
        return v.copy()
    v = v.reshape(batch, -1, LIMBS[fid])
    out = np.empty_like(v)
    r = _one(fid, root)
    _check(lib().mzk_ntt_batch(fid, _p(r), _p(v), _p(out), v.shape[1], batch, int(bool(inverse))))
    return out


def coset_lde(fid, coef, offset, generator, order):
    """ntt::fast_coset_evaluate (algebra/ntt.rs:254-269)."""
    c = _arr(fid, coef)
    out = np.empty((order, LIMBS[fid]), dtype=np.uint64)
    o, g = _one(fid, offset), _one(fid, generator)
    _check(lib().mzk_coset_lde(fid, _p(c), c.shape[0], _p(o), _p(g), _p(out), order))
    return out


def poly_scale(fid, coef, ratio, lead=None):
    """Polynomial::scale (algebra/polynomial.rs:167-174), optionally times a leading constant: lead * coef[i] * ratio^i."""
    c = _arr(fid, coef)
    out = np.empty_like(c)
    _check(lib().mzk_poly_scale(fid, _p(c), c.shape[0], _p(_one(fid, ratio)), _p(_one(fid, lead)) if lead is not None else None, _p(out)))
    return out


def fft_multiply(fid, a, b, omega):
    """Polynomial::fft_multiply (algebra/polynomial.rs:242-276)."""
    a, b = _arr(fid, a), _arr(fid, b)
    out = np.zeros((max(a.shape[0] + b.shape[0], 1), LIMBS[fid]), dtype=np.uint64)
    n = ctypes.c_size_t(0)
    w = _one(fid, omega)
    _check(lib().mzk_fft_multiply(fid, _p(a), a.shape[0], _p(b), b.shape[0], _p(w), _p(out), ctypes.byref(n)))
    return out[:n.value]


def fast_multiply(fid, a, b, root, root_order):
    """ntt::fast_multiply (algebra/ntt.rs:66-116)."""
    a, b = _arr(fid, a), _arr(fid, b)
    out = np.zeros((max(root_order, a.shape[0] + b.shape[0], 1), LIMBS[fid]), dtype=np.uint64)
    n = ctypes.c_size_t(0)
    w = _one(fid, root)
    _check(lib().mzk_fast_multiply(fid, _p(a), a.shape[0], _p(b), b.shape[0], _p(w), root_order, _p(out), ctypes.byref(n)))
    return out[:n.value]


def root_of_unity(fid, log2n):
    out = np.zeros((1, LIMBS[fid]), dtype=np.uint64)
    _check(lib().mzk_root_of_unity(fid, int(log2n), _p(out)))
    return from_limbs(out)[0]


def msm_g1(scalars, points):
    """Polynomial::eval_with_powers_on_curve (algebra/polynomial.rs:156-165) / commit_kzg (kzg.rs:57-59)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    if p.shape[0] < s.shape[0]:
        raise MzkError(-5, "index out of bounds: the len is %d but the index is %d" % (p.shape[0], p.shape[0]))
    out = np.zeros((1, 8), dtype=np.uint64)
    _check(lib().mzk_msm_g1_bn254(_p(s), _p(p), s.shape[0], _p(out)))
    return array_to_points(out)[0]


kzg_commit = msm_g1


def msm_g1_multi(scalars, points):
    """The same MSM sharded over every context of init_devices (contiguous shards, gather of 128-byte partials, fold)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
    if p.shape[0] < s.shape[0]:
        raise MzkError(-5, "index out of bounds: the len is %d but the index is %d" % (p.shape[0], p.shape[0]))
    out = np.zeros((1, 8), dtype=np.uint64)
    _check(lib().mzk_msm_g1_bn254_multi(_p(s), _p(p), s.shape[0], _p(out)))
    return array_to_points(out)[0]


LAYOUT_CONTIGUOUS, LAYOUT_CYCLIC = _C["MZK_LAYOUT_CONTIGUOUS"], _C["MZK_LAYOUT_CYCLIC"]


def ntt_multi(fid, root, values, inverse=False):
    """ntt::ntt / ntt::intt of ONE vector spread over every context of init_devices (four-step layout, mzk_ntt_multi)."""
    v = _arr(fid, values)
    out = np.empty_like(v)
    _check(lib().mzk_ntt_multi(fid, _p(_one(fid, root)), _p(v), _p(out), v.shape[0], int(bool(inverse))))
    return out


def ntt_multi_dev(fid, root, in_ptrs, out_ptrs, n, inverse=False, layout_in=LAYOUT_CONTIGUOUS, layout_out=LAYOUT_CONTIGUOUS):
    """The same with the parts resident in HBM: in_ptrs[r] / out_ptrs[r] = device pointers (ints) on context r's GPU."""
    W = len(in_ptrs)
    ins = (ctypes.c_void_p * W)(*[int(p) for p in in_ptrs])
    outs = (ctypes.c_void_p * W)(*[int(p) for p in out_ptrs])
    _check(lib().mzk_ntt_multi_dev(fid, _p(_one(fid, root)), ins, outs, n, int(bool(inverse)), int(layout_in), int(layout_out)))


class SrsMulti:
    """PublicKeyKZG.powers_1 sharded over the contexts of init_devices (kzg.rs:8-11): from host points, or built on
    the GPUs from (alpha, g1) like setup_kzg (kzg.rs:27-40)."""

    def __init__(self, powers=None, alpha=None, max_d=None, g1=(1, 2), with_tables=1):
        self._h = ctypes.c_void_p()
        if powers is not None:
            p = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, 8)
            self.n = p.shape[0]
            _check(lib().mzk_srs_upload_multi(_p(p), self.n, ctypes.byref(self._h)))
        else:
            a, g = _one(FIELD_FR, alpha), points_to_array([g1])
            self.n = max_d + 1
            _check(lib().mzk_kzg_setup_srs_multi(_p(a), _p(g), max_d, int(with_tables), ctypes.byref(self._h)))
        self.world = int(lib().mzk_srs_multi_world(self._h))
        self.lo = [int(lib().mzk_srs_multi_shard_lo(self._h, r)) for r in range(self.world + 1)]

    def commit(self, coef):
        c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((1, 8), dtype=np.uint64)
        _check(lib().mzk_kzg_commit_srs_multi(self._h, _p(c), c.shape[0], _p(out)))
        return array_to_points(out)[0]

    def commit_dev(self, shard_ptrs, n):
        """shard_ptrs[r]: device pointer (int) on context r's GPU to coefficients [lo[r], min(lo[r+1], n))."""
        arr = (ctypes.c_void_p * self.world)(*[int(x) for x in shard_ptrs])
        out = np.zeros((1, 8), dtype=np.uint64)
        _check(lib().mzk_kzg_commit_srs_multi_dev(self._h, arr, n, _p(out)))
        return array_to_points(out)[0]

    def close(self):
        if self._h:
            lib().mzk_srs_multi_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kzg_setup_g1(alpha, max_d, g1=(1, 2)):
    """setup_kzg (algebra/kzg.rs:27-40), G1 powers for a caller-supplied trapdoor."""
    out = np.zeros((max_d + 1, 8), dtype=np.uint64)
    a, g = _one(FIELD_FR, alpha), points_to_array([g1])
    _check(lib().mzk_kzg_setup_g1(_p(a), _p(g), max_d, _p(out)))
    return out


def kzg_open(coef, u, powers):
    """open_kzg (algebra/kzg.rs:61-72) -> (y, w)."""
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, 8)
    if c.shape[0] > 1 and p.shape[0] < c.shape[0] - 1:
        raise MzkError(-5, "index out of bounds: the len is %d but the index is %d" % (p.shape[0], p.shape[0]))
    y = np.zeros((1, 4), dtype=np.uint64)
    w = np.zeros((1, 8), dtype=np.uint64)
    uu = _one(FIELD_FR, u)
    _check(lib().mzk_kzg_open(_p(c), c.shape[0], _p(uu), _p(p), _p(y), _p(w)))
    return from_limbs(y)[0], array_to_points(w)[0]


def kzg_batch_open(coef, us, powers):
    """batch_open_kzg (algebra/kzg.rs:74-88) -> (ys, w)."""
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, 8)
    u = to_limbs(list(us), 4)
    k = u.shape[0]
    nq = max(c.shape[0] - k, 0)
    if p.shape[0] < nq:
        raise MzkError(-5, "index out of bounds: the len is %d but the index is %d" % (p.shape[0], p.shape[0]))
    ys = np.zeros((max(k, 1), 4), dtype=np.uint64)
    w = np.zeros((1, 8), dtype=np.uint64)
    _check(lib().mzk_kzg_batch_open(_p(c), c.shape[0], _p(u), k, _p(p), _p(ys), _p(w)))
    return from_limbs(ys[:k]), array_to_points(w)[0]


def kzg_prove_degree_bound(coef, powers, d):
    """prove_degree_bound (algebra/kzg.rs:121-134)."""
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, 8)
    out = np.zeros((1, 8), dtype=np.uint64)
    _check(lib().mzk_kzg_prove_degree_bound(_p(c), c.shape[0], _p(p), p.shape[0], d, _p(out)))
    return array_to_points(out)[0]


def fri_fold(fid, codeword, alpha, offset, omega):
    """FRI split-and-fold (zkstark/fri.rs:182-193)."""
    c = _arr(fid, codeword)
    out = np.zeros((max(c.shape[0] // 2, 1), LIMBS[fid]), dtype=np.uint64)
    a, o, w = _one(fid, alpha), _one(fid, offset), _one(fid, omega)
    _check(lib().mzk_fri_fold(fid, _p(c), c.shape[0], _p(a), _p(o), _p(w), _p(out)))
    return out[:c.shape[0] // 2]


class Srs:
    """Device-resident PublicKeyKZG.powers_1 (algebra/kzg.rs:8-11) for repeated commits."""

    def __init__(self, powers):
        p = np.ascontiguousarray(powers, dtype=np.uint64).reshape(-1, 8)
        self._h = ctypes.c_void_p()
        self.n = p.shape[0]
        _check(lib().mzk_srs_upload(_p(p), self.n, ctypes.byref(self._h)))

    def commit(self, coef):
        c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros((1, 8), dtype=np.uint64)
        _check(lib().mzk_kzg_commit_srs(self._h, _p(c), c.shape[0], _p(out)))
        return array_to_points(out)[0]

    def commit_batch(self, coefs):
        """commit_kzg of every row of `coefs` (count x n x 4 limbs; all polynomials of one length), one commit in flight
        per context of this GPU (init_devices([d, d, d, d])): mzk_kzg_commit_srs_batch."""
        c = np.ascontiguousarray(coefs, dtype=np.uint64)
        count = c.shape[0]
        if count == 0:
            return []
        c = c.reshape(count, -1, 4)
        out = np.zeros((max(count, 1), 8), dtype=np.uint64)
        _check(lib().mzk_kzg_commit_srs_batch(self._h, _p(c), c.shape[1], count, _p(out)))
        return array_to_points(out[:count])

    def commit_many(self, coefs):
        """commit_kzg of every row of `coefs` as ONE grid-batched pass (mzk_kzg_commit_srs_many_dev): the reference's per-row /
        per-chunk loops (das/avail.rs:88-98, das/eigenda.rs:92-101, algebra/gemini.rs:112-114)."""
        import torch
        c = np.ascontiguousarray(coefs, dtype=np.uint64)
        count = c.shape[0]
        if count == 0:
            return []
        c = c.reshape(count, -1, 4)
        st = torch.cuda.current_stream().cuda_stream
        d_c = torch.from_numpy(c.view(np.int64).reshape(-1).copy()).cuda() if c.size else torch.zeros(4, dtype=torch.int64, device="cuda")
        d_o = torch.zeros(count * 8, dtype=torch.int64, device="cuda")
        _check(lib().mzk_kzg_commit_srs_many_dev(self._h, d_c.data_ptr(), c.shape[1], count, d_o.data_ptr(), st))
        torch.cuda.synchronize()
        return array_to_points(d_o.cpu().numpy().view(np.uint64).reshape(count, 8))

    def gemini_commit(self, levels):
        """commit_gemini (algebra/gemini.rs:112-114) of the fold levels (gemini_split_fold's list, or the packed 2n - 1 rows)."""
        return _gemini_commit(self._h, levels)

    def gemini_open(self, levels, beta):
        """open_gemini (algebra/gemini.rs:116-144) -> (ys, ws, deg): ys[i] = (f_i(beta), f_i(-beta), f_i(beta^2)) and ws[i] for
        i < el, deg[i] = prove_degree_bound(f_i, pk, 2^(el - i)) for i <= el."""
        return _gemini_open(self._h, levels, beta)

    def sumcheck_prove(self, coef, challenge):
        """prove_sumcheck (algebra/sumcheck.rs:128-167) of a multilinear g.  challenge(round, g) -> int, with g = (A_j, B_j) of
        g_j(X) = A_j + B_j X for round j < el and None for round el (beta).  Returns a dict: gs, rs, beta, commits, ys, ws, deg."""
        return _sumcheck_prove(self._h, coef, challenge)

    def build_direct(self, window_bits=0, max_bytes=0):
        """Direct tables for batches of short polynomials (mzk_srs_build_direct); returns the width built."""
        _check(lib().mzk_srs_build_direct(self._h, int(window_bits), max_bytes, None))
        return int(lib().mzk_srs_direct_bits(self._h))

    def drop_direct(self):
        lib().mzk_srs_drop_direct(self._h)

    def save(self, path, with_tables=False):
        """Raw little-endian dump of powers_1 (+ optionally the window tables): mzk_srs_save."""
        _check(lib().mzk_srs_save(self._h, os.fsencode(path), int(bool(with_tables))))

    @classmethod
    def load(cls, path, with_tables=1):
        self = cls.__new__(cls)
        self._h = ctypes.c_void_p()
        _check(lib().mzk_srs_load(os.fsencode(path), int(with_tables), ctypes.byref(self._h)))
        self.n = int(lib().mzk_srs_len(self._h))
        return self

    def download(self):
        """powers_1 back as an (n, 8) limb array."""
        out = np.zeros((max(self.n, 1), 8), dtype=np.uint64)
        _check(lib().mzk_srs_download(self._h, _p(out), self.n))
        return out[:self.n]

    def close(self):
        if self._h:
            lib().mzk_srs_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MerkleTree:
    """Merkle::commit / Merkle::open (algebra/merkle.rs:15-46) over a codeword, resident in HBM.

    Leaves are bincode(FiniteFieldElement) of the elements (zkstark/fri.rs:160-166) or arbitrary byte strings."""

    def __init__(self, fid=None, elems=None, leaves=None, negative=None):
        self._h = ctypes.c_void_p()
        self.fid = fid if leaves is None else None
        if negative is not None:       # (magnitude, Sign::Minus flag) pairs: unsanitized elements (field.rs:98-110)
            e = _arr(fid, elems)
            ng = np.ascontiguousarray(negative, dtype=np.uint8)
            self.n = e.shape[0]
            self.stride = 48
            _check(lib().mzk_merkle_build_field_signed(fid, _p(e), _p(ng), self.n, ctypes.byref(self._h)))
        elif leaves is not None:
            blob = b"".join(leaves)
            off = np.zeros(len(leaves) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(x) for x in leaves], dtype=np.uint64) if leaves else []
            buf = (ctypes.c_uint8 * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
            self.n = len(leaves)
            self.stride = max([32] + [len(x) for x in leaves])
            _check(lib().mzk_merkle_build_bytes(buf, _p(off), self.n, ctypes.byref(self._h)))
        else:
            e = _arr(fid, elems)
            self.n = e.shape[0]
            self.stride = _leaf_stride(fid)
            _check(lib().mzk_merkle_build_field(fid, _p(e), self.n, ctypes.byref(self._h)))

    def root(self):
        buf = (ctypes.c_uint8 * max(self.stride, 64))()
        ln = ctypes.c_size_t()
        _check(lib().mzk_merkle_root(self._h, buf, len(buf), ctypes.byref(ln)))
        return bytes(buf[:ln.value])

    def open(self, index):
        depth_cap = max(self.n.bit_length(), 1)
        buf = (ctypes.c_uint8 * (self.stride * depth_cap))()
        lens = (ctypes.c_uint64 * depth_cap)()
        depth = ctypes.c_size_t()
        _check(lib().mzk_merkle_open(self._h, index, buf, self.stride, lens, ctypes.byref(depth)))
        raw = bytes(buf)
        return [raw[k * self.stride:k * self.stride + lens[k]] for k in range(depth.value)]

    def open_many(self, indices):
        """Merkle::open for every index in one gather (mzk_merkle_open_batch): list of paths as `open` returns them."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        count = idx.shape[0]
        depth_cap = max(self.n.bit_length(), 1)
        buf = (ctypes.c_uint8 * max(self.stride * depth_cap * count, 1))()
        lens = (ctypes.c_uint64 * max(depth_cap * count, 1))()
        depth = ctypes.c_size_t()
        _check(lib().mzk_merkle_open_batch(self._h, _p(idx), count, buf, self.stride, lens, ctypes.byref(depth)))
        raw, d = bytes(buf), depth.value
        return [[raw[(q * d + k) * self.stride:(q * d + k) * self.stride + lens[q * d + k]] for k in range(d)] for q in range(count)]

    def leaves(self, indices, with_sign=False):
        """The elements the tree was built over at `indices` (mzk_merkle_leaves): (n, limbs) magnitudes[, Sign::Minus flags]."""
        idx = np.ascontiguousarray(indices, dtype=np.uint64)
        nl = LIMBS[self.fid] if getattr(self, "fid", None) is not None else None
        if nl is None:
            raise MzkError(-1, "leaves: field-element trees only")
        out = np.zeros((idx.shape[0], nl), dtype=np.uint64)
        neg = np.zeros(idx.shape[0], dtype=np.uint8)
        _check(lib().mzk_merkle_leaves(self._h, _p(idx), idx.shape[0], _p(out), _p(neg) if with_sign else None))
        return (out, neg) if with_sign else out

    def close(self):
        if self._h:
            lib().mzk_merkle_free(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def merkle_open_multi(trees, index_lists):
    """Openings of several trees in ONE call (mzk_merkle_open_multi): index_lists[t] are the indices to open in trees[t] (a
    MerkleTree or None with an empty list).  Returns, per tree, the list of paths `MerkleTree.open` would return."""
    T = len(trees)
    counts = [len(ix) for ix in index_lists]
    flat = np.ascontiguousarray([i for ix in index_lists for i in ix], dtype=np.uint64)
    handles = (ctypes.c_void_p * max(T, 1))(*[t._h if t is not None else None for t in trees])
    cnt = (ctypes.c_size_t * max(T, 1))(*counts)
    depths = (ctypes.c_size_t * max(T, 1))()
    entries = sum(c * max(t.n.bit_length(), 1) for t, c in zip(trees, counts) if t is not None)
    stride = max([48] + [t.stride for t, c in zip(trees, counts) if t is not None and c])
    buf = (ctypes.c_uint8 * max(stride * entries, 1))()
    lens = (ctypes.c_uint64 * max(entries, 1))()
    _check(lib().mzk_merkle_open_multi(handles, T, _p(flat) if flat.size else None, cnt, buf, stride, lens, depths))
    raw, out, at = memoryview(buf), [], 0
    for t in range(T):
        d, paths = depths[t], []
        for q in range(counts[t]):
            paths.append([bytes(raw[(at + k) * stride:(at + k) * stride + lens[at + k]]) for k in range(d)])
            at += d
        out.append(paths)
    return out


def merkle_commit_field(fid, elems):
    """Merkle::commit(&codeword.map(bincode::serialize)) (fri.rs:160-166)."""
    e = _arr(fid, elems)
    buf = (ctypes.c_uint8 * 64)()
    ln = ctypes.c_size_t()
    _check(lib().mzk_merkle_commit_field(fid, _p(e), e.shape[0], buf, 64, ctypes.byref(ln)))
    return bytes(buf[:ln.value])


# ---- Gemini / sum-check (algebra/gemini.rs, algebra/sumcheck.rs) ----------------------------------------------------
def _levels_split(packed, n):
    out, at = [], 0
    while n >= 1:
        out.append(packed[at:at + n].copy())
        at += n
        n //= 2
    return out


def _levels_packed(levels):
    """a list of fold levels (as gemini_split_fold returns) or the packed (2n - 1, 4) array -> (packed array, n)"""
    if isinstance(levels, (list, tuple)):
        arr = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.uint64).reshape(-1, 4) for l in levels]), dtype=np.uint64)
        return arr, np.asarray(levels[0]).reshape(-1, 4).shape[0]
    arr = np.ascontiguousarray(levels, dtype=np.uint64).reshape(-1, 4)
    return arr, (arr.shape[0] + 1) // 2


def gemini_split_fold(coef, rhos):
    """split_and_fold (algebra/gemini.rs:51-100): the el + 1 fold levels f_0 = coef .. f_el = [mu], as (len, 4) limb arrays."""
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    n = c.shape[0]
    r = to_limbs(list(rhos), 4) if len(rhos) else np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros((max(2 * n - 1, 1), 4), dtype=np.uint64)
    _check(lib().mzk_gemini_split_fold(_p(c) if n else None, n, _p(r), len(rhos), _p(out)))
    return _levels_split(out, n)


def gemini_split_fold_dev(d_coef, n, rhos, d_out, stream=None):
    """mzk_gemini_split_fold_dev: device pointers (ints), the 2n - 1 packed levels written at d_out; only enqueues."""
    r = to_limbs(list(rhos), 4) if len(rhos) else np.zeros((1, 4), dtype=np.uint64)
    _check(lib().mzk_gemini_split_fold_dev(int(d_coef), n, _p(r), len(rhos), int(d_out), stream))


def sumcheck_sum(coef):
    """sum_over_boolean_hypercube (algebra/sumcheck.rs:57-66) of the multilinear g with these coefficients (get_coefs_in_order)."""
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    h = np.zeros((1, 4), dtype=np.uint64)
    _check(lib().mzk_sumcheck_sum(_p(c) if c.shape[0] else None, c.shape[0], _p(h)))
    return from_limbs(h)[0]


SCP_SECTIONS = _abi.index_names("MZK_SCP_SECTIONS")


def sumcheck_product_layout(num_vars, num_factors, max_degree, header_len=0):
    """mzk_sumcheck_product_layout: ({section: (byte offset, byte size)}, total bytes) of the packed proof (host only)."""
    off = (ctypes.c_uint64 * len(SCP_SECTIONS))()
    size = (ctypes.c_uint64 * len(SCP_SECTIONS))()
    total = ctypes.c_uint64()
    _check(lib().mzk_sumcheck_product_layout(num_vars, num_factors, max_degree, header_len, off, size, ctypes.byref(total)))
    return {k: (off[i], size[i]) for i, k in enumerate(SCP_SECTIONS)}, total.value


def sumcheck_frame_header(objects):
    """Objects of the proof stream (each a list of byte strings) in the form mzk_sumcheck_product_prove takes as `header`: per object
    its u64 LE string count, then u64 LE length + bytes per string.  The reference's header (prover.rs:108-122) is
    [[bincode(max_degree)], [bincode(num_factors)], [bincode(num_variables)]] + [[bincode(factor)] for every factor]."""
    out = []
    for obj in objects:
        out.append(len(obj).to_bytes(8, "little"))
        for s in obj:
            out.append(len(s).to_bytes(8, "little") + bytes(s))
    return b"".join(out)


def sumcheck_product_unpack(num_vars, num_factors, max_degree, header_len, raw):
    """The packed proof as a dict: sum (int), evals (num_vars lists of max_degree + 1 ints), challenges, finals, transcript (bytes)."""
    raw = bytes(raw)
    sec, _ = sumcheck_product_layout(num_vars, num_factors, max_degree, header_len)

    def part(k):
        o, s = sec[k]
        return raw[o:o + s]

    def vals(k):
        return from_limbs(np.frombuffer(part(k), dtype=np.uint64).reshape(-1, 4))
    status = int.from_bytes(part("status"), "little")
    if status != 0:
        raise MzkError(-6, "sumcheck_product_prove: status %d" % status)
    ev = vals("evals")
    tlen = int.from_bytes(part("transcript_len"), "little")
    return {"sum": vals("sum")[0], "evals": [ev[j * (max_degree + 1):(j + 1) * (max_degree + 1)] for j in range(num_vars)],
            "challenges": vals("challenges"), "finals": vals("finals"), "transcript": part("transcript")[:tlen]}


def sumcheck_product_prove(tables, max_degree, header_objects=(), device_ptr=None, num_vars=None, num_factors=None, raw=False):
    """SumCheckProverGPU::prove (examples/sumcheck/src/prover.rs:98-247) over evaluation tables in one call, the transcript on the
    device (mzk_sumcheck_product_prove).  tables: (k, 2^el, 4) limbs, factor by factor, variable 0 the most significant index bit.
    header_objects: the objects pushed before round 0 (sumcheck_frame_header's input).  device_ptr / num_vars / num_factors: the
    tables are already in HBM (mzk_sumcheck_product_prove_dev on torch's current stream); `tables` is ignored.  Returns
    sumcheck_product_unpack's dict, or the packed bytes with raw=True."""
    header = sumcheck_frame_header(header_objects)
    hbuf = (ctypes.c_uint8 * max(len(header), 1)).from_buffer_copy(header or b"\0")
    if device_ptr is None:
        t = np.ascontiguousarray(tables, dtype=np.uint64)
        if t.ndim != 3 or t.shape[2] != 4:
            raise ValueError("tables: (factors, 2^num_vars, 4) limbs")
        num_factors, n = t.shape[0], t.shape[1]
        num_vars = max(n.bit_length() - 1, 0)
        if n != 1 << num_vars:
            raise ValueError("tables: 2^num_vars values per factor")
    _, total = sumcheck_product_layout(num_vars, num_factors, max_degree, len(header))
    args = (num_vars, num_factors, max_degree, hbuf, len(header), len(header_objects))
    if device_ptr is None:
        buf = (ctypes.c_uint8 * total)()
        _check(lib().mzk_sumcheck_product_prove(_p(t), *args, buf, total))
        packed = bytes(buf)
    else:
        import torch
        proof = torch.empty(total, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        _check(lib().mzk_sumcheck_product_prove_dev(int(device_ptr), *args, proof.data_ptr(), total, stream.cuda_stream))
        stream.synchronize()
        packed = proof.cpu().numpy().tobytes()
    return packed if raw else sumcheck_product_unpack(num_vars, num_factors, max_degree, len(header), packed)


def mle_evals_from_coeffs(coef, device_ptr=None, num_vars=None, out_ptr=None, stream=None):
    """evals_over_boolean_hypercube (examples/sumcheck/src/utils.rs) of a dense multilinear polynomial (mzk_mle_evals_from_coeffs):
    coef[t] multiplies the x_i whose bit (el-1-i) of t is set; returns the (2^el, 4) table.  device_ptr / num_vars / out_ptr: device
    buffers (out_ptr may equal device_ptr), only enqueues on `stream`."""
    if device_ptr is not None:
        _check(lib().mzk_mle_evals_from_coeffs_dev(int(device_ptr), num_vars, int(out_ptr), stream))
        return None
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    n = c.shape[0]
    num_vars = max(n.bit_length() - 1, 0)
    if n != 1 << num_vars:
        raise ValueError("coef: 2^num_vars values")
    out = np.empty_like(c)
    _check(lib().mzk_mle_evals_from_coeffs(_p(c), num_vars, _p(out)))
    return out


HYPER_AUTO, HYPER_TILE, HYPER_SCATTER = _C["MZK_HYPER_AUTO"], _C["MZK_HYPER_TILE"], _C["MZK_HYPER_SCATTER"]
HYPER_PLAN_FACTORS = _C["MZK_HYPER_PLAN_FACTORS"]


def _struct_fields(name):
    """the header's struct `name` (uint64_t scalars and arrays) as ctypes _fields_"""
    return [(f, ctypes.c_uint64 if k is None else ctypes.c_uint64 * k) for f, k in _abi.c_structs(names=(name,))[0][1]]


class _HypercubePlan(ctypes.Structure):
    """mzk_hypercube_plan (include/mzk.h)"""
    _fields_ = _struct_fields("mzk_hypercube_plan")


_HYPER_PLAN_SCALARS = tuple(f for f, t in _HypercubePlan._fields_ if t is ctypes.c_uint64)


def hypercube_term_table(factors, num_vars=None):
    """Sparse Fr factors -> the flat term table of mzk_mpoly_hypercube_evals: (coefficients (T, 4) limbs, exponents (T, num_vars)
    uint32, offsets (size_t), num_vars).  A factor is an MPolynomial's dictionary {exponent tuple: int} or a pair of arrays
    (coefs (T, 4) limbs, exps (T, n) uint32); num_vars defaults to the longest key, shorter keys are padded with zeros."""
    parts = []
    for f in factors:
        if isinstance(f, dict):
            keys = list(f)
            width = max([len(k) for k in keys], default=0)
            e = np.zeros((len(keys), width), dtype=np.uint32)
            for t, key in enumerate(keys):
                e[t, :len(key)] = [int(x) for x in key]
            c = to_limbs([f[key] for key in keys], 4)
        else:
            c = np.ascontiguousarray(f[0], dtype=np.uint64).reshape(-1, 4)
            e = np.ascontiguousarray(f[1], dtype=np.uint32)
            if e.ndim != 2 or e.shape[0] != c.shape[0]:
                e = e.reshape(c.shape[0], e.size // c.shape[0]) if c.shape[0] else np.zeros((0, 0), dtype=np.uint32)
        parts.append((c, e))
    widest = max([e.shape[1] for _, e in parts], default=0)
    nv = widest if num_vars is None else int(num_vars)
    if nv < widest:
        raise MzkError(-5, "a term has %d exponents, num_vars is %d" % (widest, nv))
    total = sum(c.shape[0] for c, _ in parts)
    tc, te, offs = np.zeros((total, 4), dtype=np.uint64), np.zeros((total, nv), dtype=np.uint32), [0]
    for c, e in parts:
        at = offs[-1]
        tc[at:at + c.shape[0]] = c
        te[at:at + c.shape[0], :e.shape[1]] = e
        offs.append(at + c.shape[0])
    return tc, te, (ctypes.c_size_t * len(offs))(*offs), nv


def mpoly_hypercube_plan(factors, num_vars=None, form=HYPER_AUTO):
    """mzk_mpoly_hypercube_plan (host only): what mpoly_hypercube_evals does for these factors, as a dict -- the form that runs, the
    distinct masks and groups (totals, maxima and per factor), launches, grid, bytes uploaded, workspace and table bytes."""
    _, te, toff, nv = hypercube_term_table(factors, num_vars)
    out = _HypercubePlan()
    _check(lib().mzk_mpoly_hypercube_plan(_p(te), toff, len(factors), nv, int(form), ctypes.byref(out)))
    d = {n: int(getattr(out, n)) for n in _HYPER_PLAN_SCALARS}
    shown = min(len(factors), HYPER_PLAN_FACTORS)
    d["factor_masks"] = [int(out.factor_masks[f]) for f in range(shown)]
    d["factor_groups"] = [int(out.factor_groups[f]) for f in range(shown)]
    return d


def mpoly_hypercube_evals(factors, num_vars=None, form=HYPER_AUTO, out_ptr=None, stream=None):
    """evals_over_boolean_hypercube of sparse factors (mzk_mpoly_hypercube_evals): the (k, 2^num_vars, 4) tables, variable 0 the most
    significant index bit, as sumcheck_product_prove takes them.  out_ptr: the tables are written to that device buffer
    (mzk_mpoly_hypercube_evals_dev, enqueued on `stream`) and None is returned."""
    tc, te, toff, nv = hypercube_term_table(factors, num_vars)
    args = (_p(tc), _p(te), toff, len(factors), nv, int(form))
    if out_ptr is not None:
        _check(lib().mzk_mpoly_hypercube_evals_dev(*args, int(out_ptr), stream))
        return None
    out = np.empty((len(factors), 1 << nv, 4), dtype=np.uint64)
    _check(lib().mzk_mpoly_hypercube_evals(*args, _p(out)))
    return out


def sumcheck_product_prove_terms(factors, max_degree, header_objects=(), num_vars=None, device=False, raw=False):
    """SumCheckProverGPU::prove from the reference's own inputs (mzk_sumcheck_product_prove_terms): sparse factors as in
    hypercube_term_table, their tables built on the device and never seen by the host.  device=True: the proof is written to a torch
    buffer on torch's current stream (the _dev form).  Returns what sumcheck_product_prove returns."""
    tc, te, toff, nv = hypercube_term_table(factors, num_vars)
    k = len(factors)
    header = sumcheck_frame_header(header_objects)
    hbuf = (ctypes.c_uint8 * max(len(header), 1)).from_buffer_copy(header or b"\0")
    _, total = sumcheck_product_layout(nv, k, max_degree, len(header))
    args = (_p(tc), _p(te), toff, k, nv, max_degree, hbuf, len(header), len(header_objects))
    if not device:
        buf = (ctypes.c_uint8 * total)()
        _check(lib().mzk_sumcheck_product_prove_terms(*args, buf, total))
        packed = bytes(buf)
    else:
        import torch
        proof = torch.empty(total, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        _check(lib().mzk_sumcheck_product_prove_terms_dev(*args, proof.data_ptr(), total, stream.cuda_stream))
        stream.synchronize()
        packed = proof.cpu().numpy().tobytes()
    return packed if raw else sumcheck_product_unpack(nv, k, max_degree, len(header), packed)


_SUMCHECK_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64))


def _gemini_commit(h, levels):
    arr, n = _levels_packed(levels)
    el = max(n.bit_length() - 1, 0)
    out = np.zeros((el + 1, 8), dtype=np.uint64)
    _check(lib().mzk_gemini_commit_srs(h, _p(arr), n, _p(out)))
    return array_to_points(out)


def _gemini_open(h, levels, beta):
    arr, n = _levels_packed(levels)
    el = max(n.bit_length() - 1, 0)
    ys = np.zeros((max(3 * el, 1), 4), dtype=np.uint64)
    ws = np.zeros((max(el, 1), 8), dtype=np.uint64)
    deg = np.zeros((el + 1, 8), dtype=np.uint64)
    b = to_limbs([beta], 4)
    _check(lib().mzk_gemini_open_srs(h, _p(arr), n, _p(b), _p(ys), _p(ws), _p(deg)))
    y = from_limbs(ys[:3 * el]) if el else []
    return [tuple(y[3 * i:3 * i + 3]) for i in range(el)], (array_to_points(ws[:el]) if el else []), array_to_points(deg)


def _sumcheck_prove(h, coef, challenge):
    c = np.ascontiguousarray(coef, dtype=np.uint64).reshape(-1, 4)
    n = c.shape[0]
    el = max(n.bit_length() - 1, 0)
    failure = []

    def cb(user, rnd, g, r_out):
        # An exception must not escape into C: keep it, stop the prover (non-zero status -> MZK_E_CALLBACK), re-raise below.
        try:
            gg = None
            if g:
                v = [int(g[k]) for k in range(8)]
                gg = (sum(v[k] << (64 * k) for k in range(4)), sum(v[4 + k] << (64 * k) for k in range(4)))
            r = challenge(rnd, gg)
            if r is None:
                raise ValueError("challenge(%d) returned no value" % rnd)
            r = int(r)
            for j in range(4):
                r_out[j] = (r >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
            return 0
        except BaseException as ex:      # noqa: BLE001 -- re-raised by sumcheck_prove
            failure.append(ex)
            return 1

    k = max(el, 1)
    gs, rs = np.zeros((k, 8), dtype=np.uint64), np.zeros((k, 4), dtype=np.uint64)
    beta = np.zeros((1, 4), dtype=np.uint64)
    commits, deg = np.zeros((el + 1, 8), dtype=np.uint64), np.zeros((el + 1, 8), dtype=np.uint64)
    ys, ws = np.zeros((3 * k, 4), dtype=np.uint64), np.zeros((k, 8), dtype=np.uint64)
    fn = _SUMCHECK_CB(cb)
    rc = lib().mzk_sumcheck_prove_srs(h, _p(c) if n else None, n, fn, None, _p(gs), _p(rs), _p(beta), _p(commits), _p(ys), _p(ws), _p(deg))
    if failure:
        raise failure[0]
    _check(rc)
    y = from_limbs(ys[:3 * el])
    return {"gs": list(zip(from_limbs(gs[:el, :4]), from_limbs(gs[:el, 4:]))), "rs": from_limbs(rs[:el]), "beta": from_limbs(beta)[0],
            "commits": array_to_points(commits), "ys": [tuple(y[3 * i:3 * i + 3]) for i in range(el)], "ws": array_to_points(ws[:el]),
            "deg": array_to_points(deg)}

_FRI_CB = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_uint8), ctypes.c_size_t,
                           ctypes.POINTER(ctypes.c_uint64))


def fri_commit(fid, codeword, omega, offset, num_rounds, challenge, negative=None, keep_trees=False, codewords=True, device_ptr=None, n=None):
    """FRI::commit (zkstark/fri.rs:144-209), codewords resident in HBM.  challenge(round, last, root_bytes) -> alpha
    (int; ignored when last).  Returns (codewords, roots).  negative: optional Sign::Minus flags of the initial
    codeword, then given as magnitudes (round 0 commits to the unsanitized elements, fri.rs:160-166).
    keep_trees: also return the rounds' Merkle trees (MerkleTree objects on the device, None for a one-element round)
    for the query phase: (codewords, roots, trees).  codewords=False (with keep_trees): nothing but the roots comes back to
    the host -- (None, roots, trees); the query phase reads values and paths from the trees (MerkleTree.leaves,
    merkle_open_multi).  device_ptr / n: the initial codeword is already in HBM (mzk_fri_commit_keep_trees_dev); `codeword`
    is then ignored."""
    nl = LIMBS[fid]
    if device_ptr is None:
        c = _arr(fid, codeword)
        n = c.shape[0]
    elif not keep_trees:
        raise MzkError(-1, "fri_commit: a device-resident codeword needs keep_trees=True")

    failure = []

    def cb(user, rnd, last, root, root_len, alpha_out):
        # An exception must not escape into C (ctypes would print it and carry on with whatever alpha_out holds):
        # keep it, make the C loop stop (non-zero status -> MZK_E_CALLBACK), re-raise below.
        try:
            a = challenge(rnd, bool(last), ctypes.string_at(root, root_len))      # (slicing the pointer builds a list first: ~4 us per round)
            if last:
                return 0
            if a is None:
                raise ValueError("challenge(%d) returned no alpha" % rnd)
            a = int(a)
            for j in range(nl):
                alpha_out[j] = (a >> (64 * j)) & 0xFFFFFFFFFFFFFFFF
            return 0
        except BaseException as ex:      # noqa: BLE001 -- re-raised by fri_commit
            failure.append(ex)
            return 1

    total = sum(n >> r for r in range(num_rounds))
    roots = (ctypes.c_uint8 * (48 * max(num_rounds, 1)))()
    lens = (ctypes.c_uint64 * max(num_rounds, 1))()
    allcw = np.zeros((max(total, 1) if (codewords or not keep_trees) else 1, nl), dtype=np.uint64)
    w, o = _one(fid, omega), _one(fid, offset)
    fn = _FRI_CB(cb)
    handles = (ctypes.c_void_p * max(num_rounds, 1))()
    if keep_trees:
        ng = None if negative is None else np.ascontiguousarray(negative, dtype=np.uint8)
        cw_out = _p(allcw) if codewords else None
        if device_ptr is not None:
            rc = lib().mzk_fri_commit_keep_trees_dev(fid, int(device_ptr), None if ng is None else _p(ng), n, _p(w), _p(o),
                                                     int(num_rounds), fn, None, roots, lens, cw_out, handles)
        else:
            rc = lib().mzk_fri_commit_keep_trees(fid, _p(c), None if ng is None else _p(ng), n, _p(w), _p(o), int(num_rounds), fn, None, roots, lens, cw_out, handles)
    elif negative is not None:
        ng = np.ascontiguousarray(negative, dtype=np.uint8)
        rc = lib().mzk_fri_commit_signed(fid, _p(c), _p(ng), n, _p(w), _p(o), int(num_rounds), fn, None, roots, lens, _p(allcw))
    else:
        rc = lib().mzk_fri_commit(fid, _p(c), n, _p(w), _p(o), int(num_rounds), fn, None, roots, lens, _p(allcw))
    if failure:
        raise failure[0]
    _check(rc)
    cws, rts, at = [], [], 0
    raw = bytes(roots)
    for r in range(num_rounds):
        if codewords or not keep_trees:
            cws.append(allcw[at:at + (n >> r)].copy())
        rts.append(raw[48 * r:48 * r + lens[r]])
        at += n >> r
    if keep_trees:
        trees = []
        for r in range(num_rounds):
            if not handles[r]:
                trees.append(None)
                continue
            t = MerkleTree.__new__(MerkleTree)
            t._h = ctypes.c_void_p(handles[r])
            t.n = n >> r
            t.stride = _leaf_stride(fid)
            t.fid = fid
            trees.append(t)
        return (cws if codewords else None), rts, trees
    return cws, rts


FRI_SECTIONS = _abi.index_names("MZK_FRI_SECTIONS")
FRI_PATH_STRIDE = _C["MZK_FRI_PATH_STRIDE"]


def fri_proof_layout(fid, n, expansion_factor, num_colinearity_tests):
    """mzk_fri_proof_layout: (num_rounds, {section: (byte offset, byte size)}, total bytes) of the packed proof (host only)."""
    rounds = ctypes.c_int()
    off = (ctypes.c_uint64 * len(FRI_SECTIONS))()
    size = (ctypes.c_uint64 * len(FRI_SECTIONS))()
    total = ctypes.c_uint64()
    _check(lib().mzk_fri_proof_layout(int(fid), n, expansion_factor, num_colinearity_tests, ctypes.byref(rounds), off, size, ctypes.byref(total)))
    return rounds.value, {k: (off[i], size[i]) for i, k in enumerate(FRI_SECTIONS)}, total.value


def _fri_unpack(layout, nl, stride, n, T, raw, rows):
    """the sections of a packed FRI proof (mzk_fri_proof_layout or _gl) as fri_unpack_proof's dict; rows: a layer's values stay a
    (T, nl) array (no signs) instead of becoming ints"""
    raw = bytes(raw)
    R, sec, _ = layout

    def part(k):
        o, s = sec[k]
        return raw[o:o + s]
    status = int.from_bytes(part("status"), "little")
    if status != 0:
        raise MzkError(-6, "fri_prove: sample_indices gave up (status %d)" % status)
    top = [int(x) for x in np.frombuffer(part("top_indices"), dtype=np.uint64)]
    roots = [part("roots")[32 * r:32 * r + 32] for r in range(R)]
    last = np.frombuffer(part("last_codeword"), dtype=np.uint64).reshape(-1, nl).copy()
    words = np.frombuffer(part("values"), dtype=np.uint64).reshape(-1, nl)
    vals = words if rows else (from_limbs(words) if T else [])
    signs = part("signs")
    paths, lens = part("paths"), np.frombuffer(part("path_lens"), dtype=np.uint64)
    layers, q, e = [], 0, 0
    for i in range(R - 1):
        layer = {}
        for kind in "abc":
            d = (n >> (i + (kind == "c"))).bit_length() - 1
            v, ps = [], []
            for _ in range(T):
                if not rows:
                    v.append(-vals[q] if signs[q] else vals[q])
                ps.append([paths[(e + k) * stride:(e + k) * stride + int(lens[e + k])] for k in range(d)])
                q += 1
                e += d
            layer[kind] = (vals[q - T:q].copy() if rows else v, ps)
        layers.append(layer)
    return {"top_level_indices": top, "last_codeword": last, "merkle_roots": roots, "revealed_layers": layers}


def fri_unpack_proof(fid, n, expansion_factor, num_colinearity_tests, raw):
    """The packed proof of mzk_fri_prove as the reference's FriProof (fri.rs:71-82): top_level_indices, last_codeword ((m, limbs)
    array), merkle_roots (bytes), revealed_layers ([{"a": (values, paths), "b": ..., "c": ...}]).  A value with Sign::Minus is the
    negative int -magnitude.  Raises MzkError when the status word is set."""
    return _fri_unpack(fri_proof_layout(fid, n, expansion_factor, num_colinearity_tests), LIMBS[fid], FRI_PATH_STRIDE, n, num_colinearity_tests,
                       raw, False)


def fri_prove(fid, codeword, omega, offset, expansion_factor, num_colinearity_tests, negative=None, device_ptr=None, n=None):
    """FRI::prove (zkstark/fri.rs:99-143) in one call (mzk_fri_prove): the reference's transcript, index sampling and query phase on
    the device.  Returns fri_unpack_proof's dict.  negative: Sign::Minus flags of the initial codeword, then given as magnitudes.
    device_ptr / n: the codeword is already in HBM (mzk_fri_prove_dev on torch's current stream; negative then a device pointer or
    None); `codeword` is ignored."""
    _, _, total = fri_proof_layout(fid, n if device_ptr is not None else _arr(fid, codeword).shape[0], expansion_factor, num_colinearity_tests)
    w, o = _one(fid, omega), _one(fid, offset)
    if device_ptr is None:
        c = _arr(fid, codeword)
        n = c.shape[0]
        ng = None if negative is None else np.ascontiguousarray(negative, dtype=np.uint8)
        buf = (ctypes.c_uint8 * total)()
        _check(lib().mzk_fri_prove(int(fid), _p(c), None if ng is None else _p(ng), n, _p(w), _p(o), expansion_factor, num_colinearity_tests, buf, total))
        raw = bytes(buf)
    else:
        import torch
        proof = torch.empty(total, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        _check(lib().mzk_fri_prove_dev(int(fid), int(device_ptr), None if negative is None else int(negative), n, _p(w), _p(o), expansion_factor, num_colinearity_tests,
                                       proof.data_ptr(), total, stream.cuda_stream))
        stream.synchronize()
        raw = proof.cpu().numpy().tobytes()
    return fri_unpack_proof(fid, n, expansion_factor, num_colinearity_tests, raw)


FRI_PATH_STRIDE_GL = _C["MZK_FRI_PATH_STRIDE_GL"]


def fri_proof_layout_gl(fid, n, expansion_factor, num_colinearity_tests):
    """mzk_fri_proof_layout_gl: fri_proof_layout's triple for the Goldilocks ids (1 or 3 words per element, 64-byte path entries)."""
    rounds = ctypes.c_int()
    off = (ctypes.c_uint64 * len(FRI_SECTIONS))()
    size = (ctypes.c_uint64 * len(FRI_SECTIONS))()
    total = ctypes.c_uint64()
    _check(lib().mzk_fri_proof_layout_gl(int(fid), n, expansion_factor, num_colinearity_tests, ctypes.byref(rounds), off, size, ctypes.byref(total)))
    return rounds.value, {k: (off[i], size[i]) for i, k in enumerate(FRI_SECTIONS)}, total.value


def fri_unpack_proof_gl(fid, n, expansion_factor, num_colinearity_tests, raw):
    """The packed proof of mzk_fri_prove_gl in fri_unpack_proof's shape; last_codeword and every layer's values are rows of 1 or 3
    words ((count, limbs) arrays), as the other Goldilocks wrappers return elements."""
    return _fri_unpack(fri_proof_layout_gl(fid, n, expansion_factor, num_colinearity_tests), LIMBS[fid], FRI_PATH_STRIDE_GL, n,
                       num_colinearity_tests, raw, True)


def fri_prove_gl(fid, codeword, omega, offset, expansion_factor, num_colinearity_tests, device_ptr=None, n=None):
    """FRI::prove over MZK_FIELD_M64 / MZK_FIELD_M64X3 in one call (mzk_fri_prove_gl), the transcript on the device.  Returns
    fri_unpack_proof_gl's dict.  device_ptr / n: the codeword is already in HBM (mzk_fri_prove_gl_dev on torch's current stream);
    `codeword` is ignored."""
    if device_ptr is None:
        c = _arr(fid, codeword)
        n = c.shape[0]
    _, _, total = fri_proof_layout_gl(fid, n, expansion_factor, num_colinearity_tests)
    w, o = _one(fid, omega), _one(fid, offset)
    if device_ptr is None:
        buf = (ctypes.c_uint8 * total)()
        _check(lib().mzk_fri_prove_gl(int(fid), _p(c), n, _p(w), _p(o), expansion_factor, num_colinearity_tests, buf, total))
        raw = bytes(buf)
    else:
        import torch
        proof = torch.empty(total, dtype=torch.uint8, device="cuda")
        stream = torch.cuda.current_stream()
        _check(lib().mzk_fri_prove_gl_dev(int(fid), int(device_ptr), n, _p(w), _p(o), expansion_factor, num_colinearity_tests, proof.data_ptr(), total,
                                          stream.cuda_stream))
        stream.synchronize()
        raw = proof.cpu().numpy().tobytes()
    return fri_unpack_proof_gl(fid, n, expansion_factor, num_colinearity_tests, raw)


def fast_coset_divide(fid, lhs, rhs, offset, root, root_order):
    """ntt::fast_coset_divide (algebra/ntt.rs:271-330)."""
    a, b = _arr(fid, lhs), _arr(fid, rhs)
    out = np.zeros((max(a.shape[0], 1), LIMBS[fid]), dtype=np.uint64)
    ln = ctypes.c_size_t()
    o, r = _one(fid, offset), _one(fid, root)
    _check(lib().mzk_fast_coset_divide(fid, _p(a), a.shape[0], _p(b), b.shape[0], _p(o), _p(r), root_order, _p(out), ctypes.byref(ln)))
    return out[:ln.value]


def _np2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def fast_coset_divide_batch_dev(fid, d_lhs_ptr, lhs_stride, lhs_lens, d_rhs_ptr, rhs_len, offset, root, root_order, d_out_ptr, out_stride, stream=0):
    """mzk_fast_coset_divide_batch_dev: numerators (rows of lhs_stride elements) and one denominator in HBM (raw device pointers), quotient
    rows of out_stride elements written at d_out_ptr; returns the quotient lengths."""
    count = len(lhs_lens)
    ln = (ctypes.c_size_t * max(count, 1))(*[int(x) for x in lhs_lens])
    out_lens = (ctypes.c_size_t * max(count, 1))()
    o, r = _one(fid, offset), _one(fid, root)
    _check(lib().mzk_fast_coset_divide_batch_dev(int(fid), d_lhs_ptr, lhs_stride, ln, count, d_rhs_ptr, rhs_len, _p(o), _p(r), root_order,
                                                 d_out_ptr, out_stride, out_lens, stream))
    return [int(out_lens[i]) for i in range(count)]


def fast_zerofier(fid, domain, root, root_order):
    """ntt::fast_zerofier (algebra/ntt.rs:118-144)."""
    d = _arr(fid, domain)
    n = d.shape[0]
    out = np.zeros((max(n + 1, _np2(n + 1)), LIMBS[fid]), dtype=np.uint64)
    ln = ctypes.c_size_t()
    r = _one(fid, root)
    _check(lib().mzk_fast_zerofier(fid, _p(d), n, _p(r), root_order, _p(out), ctypes.byref(ln)))
    return out[:ln.value]


def fast_evaluate(fid, coef, domain, root, root_order):
    """ntt::fast_evaluate (algebra/ntt.rs:146-189)."""
    c, d = _arr(fid, coef), _arr(fid, domain)
    out = np.zeros((max(d.shape[0], 1), LIMBS[fid]), dtype=np.uint64)
    r = _one(fid, root)
    _check(lib().mzk_fast_evaluate(fid, _p(c), c.shape[0], _p(d), d.shape[0], _p(r), root_order, _p(out)))
    return out[:d.shape[0]]


def fast_interpolate(fid, domain, values, root, root_order):
    """ntt::fast_interpolate (algebra/ntt.rs:191-252)."""
    d, v = _arr(fid, domain), _arr(fid, values)
    if d.shape[0] != v.shape[0]:
        raise MzkError(-5, "assertion `left == right` failed (domain.len(), values.len())")
    out = np.zeros((max(d.shape[0], 1), LIMBS[fid]), dtype=np.uint64)
    ln = ctypes.c_size_t()
    r = _one(fid, root)
    _check(lib().mzk_fast_interpolate(fid, _p(d), _p(v), d.shape[0], _p(r), root_order, _p(out), ctypes.byref(ln)))
    return out[:ln.value]


def fast_interpolate_batch(fid, domain, values, root, root_order):
    """ntt::fast_interpolate of every row of `values` (batch x n x limbs) over one domain: list of coefficient arrays."""
    d = _arr(fid, domain)
    v = np.ascontiguousarray(values, dtype=np.uint64)
    batch = v.shape[0]
    if batch == 0:
        return []
    v = v.reshape(batch, -1, LIMBS[fid])
    if d.shape[0] != v.shape[1]:
        raise MzkError(-5, "assertion `left == right` failed (domain.len(), values.len())")
    n = d.shape[0]
    out = np.zeros((batch, max(n, 1), LIMBS[fid]), dtype=np.uint64)
    lens = (ctypes.c_size_t * batch)()
    r = _one(fid, root)
    _check(lib().mzk_fast_interpolate_batch(fid, _p(d), _p(v), n, batch, _p(r), root_order, _p(out), lens))
    return [out[k, :lens[k]] for k in range(batch)]


def fast_interpolate_batch_dev(fid, domain, d_values_ptr, batch, root, root_order, d_out_ptr, stream=0):
    """mzk_fast_interpolate_batch_dev: values and coefficients in HBM (raw device pointers, batch rows of len(domain) elements each);
    returns the trimmed lengths."""
    d = _arr(fid, domain)
    n = d.shape[0]
    lens = (ctypes.c_size_t * max(batch, 1))()
    r = _one(fid, root)
    _check(lib().mzk_fast_interpolate_batch_dev(fid, _p(d), d_values_ptr, n, batch, _p(r), root_order, d_out_ptr, lens, stream))
    return [int(lens[k]) for k in range(batch)]


def mpoly_term_table(fid, constraints, n_vars):
    """[[(coef, exps), ...], ...] (one list of terms per constraint; an MPolynomial.dictionary is `[(c, k) for k, c in d.items()]`) ->
    the flat term table of mzk_mpoly_compose: coefficients (terms x limbs), exponents (terms x n_vars, uint32), offsets (size_t)."""
    coefs, exps, offs = [], [], [0]
    for terms in constraints:
        for c, k in terms:
            if len(k) != n_vars:
                raise MzkError(-5, "index out of bounds: a term has %d exponents, the point %d polynomials" % (len(k), n_vars))
            coefs.append(int(c))
            exps.append([int(e) for e in k])
        offs.append(len(coefs))
    tc = to_limbs(coefs, LIMBS[fid]) if coefs else np.zeros((0, LIMBS[fid]), dtype=np.uint64)
    te = np.ascontiguousarray(np.array(exps, dtype=np.uint32).reshape(len(coefs), n_vars))
    return tc, te, (ctypes.c_size_t * len(offs))(*offs)


def _offsets_of(lens):
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + int(n))
    return (ctypes.c_size_t * len(offs))(*offs)


def mpoly_compose_plan(fid, constraints, point_lens):
    """mzk_mpoly_compose_plan (host only): (N, out_stride_min, [D_a + 1]) for constraints as in mpoly_term_table over point
    polynomials of the given lengths."""
    nv, nc = len(point_lens), len(constraints)
    _, te, toff = mpoly_term_table(fid, constraints, nv)
    n, smin = ctypes.c_size_t(0), ctypes.c_size_t(0)
    bounds = (ctypes.c_size_t * max(nc, 1))()
    _check(lib().mzk_mpoly_compose_plan(int(fid), _p(te), toff, nc, nv, _offsets_of(point_lens), ctypes.byref(n), ctypes.byref(smin), bounds))
    return n.value, smin.value, [int(bounds[a]) for a in range(nc)]


def mpoly_compose(fid, constraints, point, out_stride=None):
    """MPolynomial::evaluate_symbolic (algebra/mpolynomials.rs:125-141) of every constraint over one point: `point` is a list of
    coefficient arrays (n_i x limbs, ascending degree); returns one trimmed coefficient array per constraint."""
    pts = [_arr(fid, q) for q in point]
    nv, nc = len(pts), len(constraints)
    tc, te, toff = mpoly_term_table(fid, constraints, nv)
    poff = _offsets_of([q.shape[0] for q in pts])
    flat = np.ascontiguousarray(np.concatenate(pts)) if nv else np.zeros((0, LIMBS[fid]), dtype=np.uint64)
    if out_stride is None:
        out_stride = mpoly_compose_plan(fid, constraints, [q.shape[0] for q in pts])[1]
    out = np.zeros((max(nc, 1), max(out_stride, 1), LIMBS[fid]), dtype=np.uint64)
    lens = (ctypes.c_size_t * max(nc, 1))()
    _check(lib().mzk_mpoly_compose(int(fid), _p(tc), _p(te), toff, nc, nv, _p(flat), poff, _p(out), out_stride, lens))
    return [out[a, :lens[a]].copy() for a in range(nc)]


def mpoly_compose_dev(fid, constraints, d_point_ptr, point_lens, d_out_ptr, out_stride, stream=0):
    """mzk_mpoly_compose_dev: the point polynomials back to back in HBM (raw device pointer), rows of out_stride elements written at
    d_out_ptr; returns the trimmed lengths."""
    nv, nc = len(point_lens), len(constraints)
    tc, te, toff = mpoly_term_table(fid, constraints, nv)
    lens = (ctypes.c_size_t * max(nc, 1))()
    _check(lib().mzk_mpoly_compose_dev(int(fid), _p(tc), _p(te), toff, nc, nv, d_point_ptr, _offsets_of(point_lens), d_out_ptr, out_stride, lens, stream))
    return [int(lens[a]) for a in range(nc)]


def poly_lincomb(fid, polys, weights, shifts, out_cap=None):
    """sum_i weights[i] * X^shifts[i] * polys[i] (fast_stark.rs:301-326), trimmed: mzk_poly_lincomb."""
    ps = [_arr(fid, q) for q in polys]
    count = len(ps)
    flat = np.ascontiguousarray(np.concatenate(ps)) if count else np.zeros((0, LIMBS[fid]), dtype=np.uint64)
    if out_cap is None:
        out_cap = max([q.shape[0] + int(sh) for q, sh in zip(ps, shifts)] + [0])
    w = to_limbs([int(x) for x in weights], LIMBS[fid]) if count else np.zeros((0, LIMBS[fid]), dtype=np.uint64)
    sh = (ctypes.c_size_t * max(count, 1))(*[int(x) for x in shifts])
    out = np.zeros((max(out_cap, 1), LIMBS[fid]), dtype=np.uint64)
    n = ctypes.c_size_t(0)
    _check(lib().mzk_poly_lincomb(int(fid), _p(flat), _offsets_of([q.shape[0] for q in ps]), count, _p(w), sh, _p(out), out_cap, ctypes.byref(n)))
    return out[:n.value].copy()


def poly_lincomb_dev(fid, d_polys_ptr, lens, weights, shifts, d_out_ptr, out_cap, stream=0):
    """mzk_poly_lincomb_dev: polynomials back to back in HBM, out_cap elements written at d_out_ptr; returns the trimmed length."""
    count = len(lens)
    w = to_limbs([int(x) for x in weights], LIMBS[fid]) if count else np.zeros((0, LIMBS[fid]), dtype=np.uint64)
    sh = (ctypes.c_size_t * max(count, 1))(*[int(x) for x in shifts])
    n = ctypes.c_size_t(0)
    _check(lib().mzk_poly_lincomb_dev(int(fid), d_polys_ptr, _offsets_of(lens), count, _p(w), sh, d_out_ptr, out_cap, ctypes.byref(n), stream))
    return n.value


def poly_div_roots(fid, polys, roots, stride=None):
    """Row i of `polys` (a list of (n_i, limbs) arrays, need not be trimmed) divided by prod (X - r) over roots[i] (a list of integers,
    may be empty or repeat): the trimmed quotients of Polynomial long division (polynomial.rs:371-405), remainder dropped --
    the boundary quotients of fast_stark.rs:217-224.  mzk_poly_div_roots."""
    ps = [_arr(fid, q) for q in polys]
    count, nl = len(ps), LIMBS[fid]
    if len(roots) != count:
        raise MzkError(-5, "poly_div_roots: %d rows, %d root lists" % (count, len(roots)))
    if stride is None:
        stride = max([q.shape[0] for q in ps] + [0])
    flat = np.zeros((max(count * stride, 1), nl), dtype=np.uint64)
    for i, q in enumerate(ps):
        flat[i * stride:i * stride + min(q.shape[0], stride)] = q[:stride]
    lens = (ctypes.c_size_t * max(count, 1))(*[q.shape[0] for q in ps])
    rs = [int(r) for row in roots for r in row]
    r = to_limbs(rs, nl) if rs else np.zeros((1, nl), dtype=np.uint64)
    out = np.zeros_like(flat)
    out_lens = (ctypes.c_size_t * max(count, 1))()
    _check(lib().mzk_poly_div_roots(int(fid), _p(flat), stride, lens, count, _p(r), _offsets_of([len(row) for row in roots]), _p(out), out_lens))
    return [out[i * stride:i * stride + int(out_lens[i])].copy() for i in range(count)]


def poly_div_roots_dev(fid, d_polys_ptr, stride, lens, roots, d_out_ptr, stream=0):
    """mzk_poly_div_roots_dev: rows of `stride` elements in HBM (raw device pointers, out rows at the same stride, not overlapping the
    input); roots[i] as in poly_div_roots; returns the trimmed quotient lengths."""
    count, nl = len(lens), LIMBS[fid]
    if len(roots) != count:
        raise MzkError(-5, "poly_div_roots: %d rows, %d root lists" % (count, len(roots)))
    rs = [int(r) for row in roots for r in row]
    r = to_limbs(rs, nl) if rs else np.zeros((1, nl), dtype=np.uint64)
    ln = (ctypes.c_size_t * max(count, 1))(*[int(x) for x in lens])
    out_lens = (ctypes.c_size_t * max(count, 1))()
    _check(lib().mzk_poly_div_roots_dev(int(fid), d_polys_ptr, stride, ln, count, _p(r), _offsets_of([len(row) for row in roots]), d_out_ptr, out_lens, stream))
    return [int(out_lens[i]) for i in range(count)]


STARK_MAX_REGISTERS, STARK_MAX_CONSTRAINTS = _C["MZK_STARK_MAX_REGISTERS"], _C["MZK_STARK_MAX_CONSTRAINTS"]


class StarkDims(ctypes.Structure):
    """mzk_stark_dims (include/mzk.h): scalars, then arrays per transition constraint and per register"""
    _fields_ = _struct_fields("mzk_stark_dims")
    _scalars = tuple(f for f, t in _fields_ if t is ctypes.c_uint64)
    _per_constraint = tuple(f for f, t in _fields_ if f.startswith("transition_"))
    _per_register = tuple(f for f, t in _fields_ if f.startswith("boundary_"))


def stark_plan(fid, expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree, constraints, boundary):
    """mzk_stark_plan (host only): the sizes FastStark derives from its parameters (fast_stark.rs:573-616, :77-111, :150-160) as a dict.
    constraints as in mpoly_term_table over 1 + 2 * num_registers variables (the coefficients are not used); boundary: (cycle, register[, value])."""
    nv = 1 + 2 * int(num_registers)
    _, te, toff = mpoly_term_table(fid, constraints, nv)
    nb = len(boundary)
    bc = (ctypes.c_size_t * max(nb, 1))(*[int(b[0]) for b in boundary])
    br = (ctypes.c_size_t * max(nb, 1))(*[int(b[1]) for b in boundary])
    d = StarkDims()
    _check(lib().mzk_stark_plan(int(fid), expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree, _p(te), toff,
                                len(constraints), bc, br, nb, ctypes.byref(d)))
    out = {k: int(getattr(d, k)) for k in StarkDims._scalars}
    out.update({k: [int(v) for v in getattr(d, k)][:len(constraints)] for k in StarkDims._per_constraint})
    out.update({k: [int(v) for v in getattr(d, k)][:int(num_registers)] for k in StarkDims._per_register})
    return out


STARK_SECTIONS = _abi.index_names("MZK_STARK_SECTIONS")


def _stark_dims_struct(dims):
    d = StarkDims()
    for k in StarkDims._scalars:
        setattr(d, k, int(dims[k]))
    for k in StarkDims._per_constraint + StarkDims._per_register:
        for i, v in enumerate(dims[k]):
            getattr(d, k)[i] = int(v)
    return d


def stark_proof_layout(fid, dims):
    """mzk_stark_proof_layout (host only): ({section: (offset, size)}, total bytes) for the dims dict of stark_plan."""
    off, size = (ctypes.c_uint64 * len(STARK_SECTIONS))(), (ctypes.c_uint64 * len(STARK_SECTIONS))()
    total = ctypes.c_uint64()
    d = _stark_dims_struct(dims)
    _check(lib().mzk_stark_proof_layout(ctypes.byref(d), int(fid), off, size, ctypes.byref(total)))
    return {k: (int(off[i]), int(size[i])) for i, k in enumerate(STARK_SECTIONS)}, int(total.value)


def stark_unpack_proof(fid, dims, raw):
    """The packed proof of mzk_stark_prove as the reference's FastStarkProof (fast_stark.rs:22-32), a dict: fri (fri_unpack_proof's dict
    with last_codeword as integers and the SORTED top_level_indices), bqc_roots, bqc_points, bqc_paths, rdc_root, rdc_points, rdc_paths,
    tzc_points, tzc_paths, and `indices` (the duplicated indices the openings are at).  Raises MzkError when the status word is set."""
    raw = bytes(raw)
    nl = LIMBS[fid]
    sec, _ = stark_proof_layout(fid, dims)
    part = lambda k: raw[sec[k][0]:sec[k][0] + sec[k][1]]
    if int.from_bytes(part("status"), "little") != 0:
        raise MzkError(-6, "stark_prove: sample_indices gave up")
    flen, e, t, m = dims["fri_domain_length"], dims["fri_domain_length"] // dims["omicron_domain_length"], dims["num_randomizers"] // 4, dims["num_registers"]
    fri = fri_unpack_proof(fid, flen, e, t, part("fri"))
    fri["last_codeword"] = from_limbs(fri["last_codeword"])
    k, depth = dims["num_indices"], flen.bit_length() - 1
    lens = np.frombuffer(part("path_lens"), dtype=np.uint64)
    out = {"fri": fri, "indices": [int(x) for x in np.frombuffer(part("indices"), dtype=np.uint64)],
           "bqc_roots": [part("bqc_roots")[32 * r:32 * r + 32] for r in range(m)], "rdc_root": part("rdc_root")}
    at = 0
    for name, count in (("bqc", m * k), ("rdc", k), ("tzc", k)):
        out[name + "_points"] = from_limbs(np.frombuffer(part(name + "_points"), dtype=np.uint64).reshape(-1, nl)) if count else []
        blob, paths = part(name + "_paths"), []
        for q in range(count):
            paths.append([blob[(q * depth + j) * 48:(q * depth + j) * 48 + int(lens[at + j])] for j in range(depth)])
            at += depth
        out[name + "_paths"] = paths
    return out


class Stark:
    """FastStark with what preprocess makes (mzk_stark_new) and prove in one call.  constraints as in mpoly_term_table over
    1 + 2 * num_registers variables; boundary: (cycle, register, value) triples."""

    def __init__(self, fid, expansion_factor, num_colinearity_checks, num_registers, num_cycles, transition_constraints_degree, generator, constraints):
        self._h = ctypes.c_void_p()
        self.fid, self.constraints = int(fid), constraints
        self.params = (int(expansion_factor), int(num_colinearity_checks), int(num_registers), int(num_cycles), int(transition_constraints_degree))
        tc, te, toff = mpoly_term_table(fid, constraints, 1 + 2 * int(num_registers))
        _check(lib().mzk_stark_new(self.fid, *self.params, _p(_one(fid, generator)), _p(tc), _p(te), toff, len(constraints), ctypes.byref(self._h)))

    def dims(self, boundary):
        """the sizes of a proof for this boundary (stark_plan)"""
        return stark_plan(self.fid, *self.params, self.constraints, boundary)

    def transition_zerofier_root(self):
        buf = (ctypes.c_uint8 * 32)()
        _check(lib().mzk_stark_transition_zerofier_root(self._h, buf))
        return bytes(buf)

    def _boundary(self, boundary):
        nb = len(boundary)
        sz = ctypes.c_size_t
        bc = (sz * max(nb, 1))(*[int(b[0]) for b in boundary])
        br = (sz * max(nb, 1))(*[int(b[1]) for b in boundary])
        bv = to_limbs([int(b[2]) for b in boundary], LIMBS[self.fid]) if nb else np.zeros((1, LIMBS[self.fid]), dtype=np.uint64)
        return bc, br, bv, nb

    def prove_raw(self, trace, boundary, randomizer):
        """mzk_stark_prove: trace (rows x registers x limbs, the random rows appended), randomizer (max_degree + 1 coefficients) -> packed bytes"""
        d = self.dims(boundary)
        _, total = stark_proof_layout(self.fid, d)
        t = np.ascontiguousarray(trace, dtype=np.uint64).reshape(-1, self.params[2], LIMBS[self.fid])
        r = _arr(self.fid, randomizer)
        bc, br, bv, nb = self._boundary(boundary)
        buf = (ctypes.c_uint8 * total)()
        _check(lib().mzk_stark_prove(self._h, _p(t), t.shape[0], bc, br, _p(bv), nb, _p(r), buf, total))
        return bytes(buf)

    def prove(self, trace, boundary, randomizer):
        return stark_unpack_proof(self.fid, self.dims(boundary), self.prove_raw(trace, boundary, randomizer))

    def prove_dev(self, d_trace_ptr, n_rows, boundary, d_randomizer_ptr, d_proof_ptr, proof_cap, stream=0):
        """mzk_stark_prove_dev: raw device pointers; returns when the proof at d_proof_ptr is complete"""
        bc, br, bv, nb = self._boundary(boundary)
        _check(lib().mzk_stark_prove_dev(self._h, d_trace_ptr, n_rows, bc, br, _p(bv), nb, d_randomizer_ptr, d_proof_ptr, proof_cap, stream))

    def close(self):
        if self._h:
            lib().mzk_stark_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def g2_points_to_array(pts):
    """[((x0, x1), (y0, y1)), ...] -> (n, 16) limbs; infinity = ((0, 0), (0, 0))."""
    a = np.zeros((len(pts), 16), dtype=np.uint64)
    for i, (x, y) in enumerate(pts):
        a[i] = to_limbs([x[0], x[1], y[0], y[1]], 4).reshape(-1)
    return a


def array_to_g2_points(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 16)
    out = []
    for row in a:
        v = from_limbs(row.reshape(4, 4))
        out.append(((v[0], v[1]), (v[2], v[3])))
    return out


def msm_g2(scalars, points):
    """Polynomial::eval_with_powers_on_curve over G2 (kzg.rs:114)."""
    s = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    p = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 16)
    if p.shape[0] < s.shape[0]:
        raise MzkError(-5, "index out of bounds: powers.len() < coef.len() (polynomial.rs:162)")
    out = np.zeros(16, dtype=np.uint64)
    _check(lib().mzk_msm_g2_bn254(_p(s), _p(p), s.shape[0], _p(out)))
    return array_to_g2_points(out)[0]


def kzg_setup_g2(alpha, max_d, g2):
    """powers_2 of setup_kzg_with_full_g2 (kzg.rs:42-55) for a given alpha."""
    a = to_limbs([alpha], 4)
    g = g2_points_to_array([g2])
    out = np.zeros((max_d + 1, 16), dtype=np.uint64)
    _check(lib().mzk_kzg_setup_g2(_p(a), _p(g), max_d, _p(out)))
    return out


# ---- Reed-Solomon over GF(2^8) (algebra/reedsolomon.rs): symbols are bytes, arrays numpy uint8 ---------------------------------------
RS_NONE = 255      # the status of a word the reference's decoder returns None for


def _bytes2d(a, width, what):
    a = np.ascontiguousarray(a, dtype=np.uint8)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.ndim != 2 or a.shape[1] != width:
        raise MzkError(-5, "%s: expected rows of %d bytes, got shape %s" % (what, width, a.shape))
    return a


def rs_generator_poly(n, k):
    """generator_polynomial (reedsolomon.rs:34-37): n - k + 1 coefficients from the constant term up.  Host arithmetic: no GPU needed."""
    g = np.zeros(max(int(n) - int(k), 0) + 1, dtype=np.uint8)
    _check(lib().mzk_rs_generator_poly(int(n), int(k), _p(g)))
    return g


def rs_encode(n, k, messages):
    """encode (reedsolomon.rs:54-78) of every row of `messages` (batch x k bytes): batch x n bytes, fixed length (the reference's
    vector is this one without its trailing zeros)."""
    m = _bytes2d(messages, k, "rs_encode")
    out = np.empty((m.shape[0], n), dtype=np.uint8)
    _check(lib().mzk_rs_encode(int(n), int(k), _p(m), m.shape[0], _p(out)))
    return out


def rs_encode_dev(n, k, d_messages, batch, d_codewords, d_columns_fr=None, stream=None):
    """mzk_rs_encode_dev: device pointers (ints); d_columns_fr (optional): n x batch Fr elements, symbol-major.  Only enqueues."""
    _check(lib().mzk_rs_encode_dev(int(n), int(k), int(d_messages), int(batch), int(d_codewords), int(d_columns_fr) if d_columns_fr else None, stream))


def rs_encode_view_dev(n, k, d_messages, msg_symbol_stride, msg_stride, batch, d_codewords, cw_symbol_stride, cw_stride, d_columns_fr=None, stream=None):
    """mzk_rs_encode_view_dev: symbol s of item b at base + b * stride + s * symbol_stride on both sides.  Only enqueues."""
    _check(lib().mzk_rs_encode_view_dev(int(n), int(k), int(d_messages), int(msg_symbol_stride), int(msg_stride), int(batch),
                                        int(d_codewords), int(cw_symbol_stride), int(cw_stride),
                                        int(d_columns_fr) if d_columns_fr else None, stream))


def rs_syndromes(n, k, words):
    """compute_syndromes (reedsolomon.rs:90-102) of every row of `words` (batch x n bytes): batch x (n - k) bytes."""
    w = _bytes2d(words, n, "rs_syndromes")
    out = np.zeros((w.shape[0], n - k), dtype=np.uint8)
    _check(lib().mzk_rs_syndromes(int(n), int(k), _p(w), w.shape[0], _p(out)))
    return out


def rs_syndromes_dev(n, k, d_words, batch, d_syndromes, stream=None):
    _check(lib().mzk_rs_syndromes_dev(int(n), int(k), int(d_words), int(batch), int(d_syndromes), stream))


def rs_decode(n, k, received, with_corrected=False):
    """decode (reedsolomon.rs:80-86) of every row of `received` (batch x n bytes): (messages batch x k, status batch) -- status 0
    clean, else the number of corrected symbols, RS_NONE (255) where the reference returns None (that row of messages is then the
    received one).  with_corrected: (corrected batch x n, messages, status)."""
    r = _bytes2d(received, n, "rs_decode")
    batch = r.shape[0]
    msgs = np.empty((batch, k), dtype=np.uint8)
    status = np.empty(batch, dtype=np.uint8)
    corr = np.empty((batch, n), dtype=np.uint8) if with_corrected else None
    _check(lib().mzk_rs_decode(int(n), int(k), _p(r), batch, _p(corr) if with_corrected else None, _p(msgs), _p(status)))
    return (corr, msgs, status) if with_corrected else (msgs, status)


def rs_decode_dev(n, k, d_received, batch, d_corrected, d_messages, d_status, stream=None):
    """mzk_rs_decode_dev: device pointers (ints); d_corrected or d_messages may be None.  Only enqueues."""
    opt = lambda p: int(p) if p else None
    _check(lib().mzk_rs_decode_dev(int(n), int(k), int(d_received), int(batch), opt(d_corrected), opt(d_messages), int(d_status), stream))


def rs2d_encode(col_n, row_n, data):
    """ReedSolomon2D::encode (reedsolomon.rs:274-295) of `data` (message_len bytes): col_n x row_n bytes."""
    d = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    out = np.empty((col_n, row_n), dtype=np.uint8)
    _check(lib().mzk_rs2d_encode(int(col_n), int(row_n), _p(d), d.shape[0], _p(out)))
    return out


def rs2d_encode_dev(col_n, row_n, d_data, message_len, d_code, stream=None):
    _check(lib().mzk_rs2d_encode_dev(int(col_n), int(row_n), int(d_data), int(message_len), int(d_code), stream))


def rs2d_decode(col_n, row_n, code, message_len, with_status=False):
    """ReedSolomon2D::decode (reedsolomon.rs:297-324) of `code` (col_n x row_n bytes): message_len bytes, or None where the reference
    returns None.  with_status: (data or None, column statuses, row statuses)."""
    c = _bytes2d(code, row_n, "rs2d_decode")
    if c.shape[0] != col_n:
        raise MzkError(-5, "rs2d_decode: expected %d rows, got %d" % (col_n, c.shape[0]))
    size = 0
    while size * size < message_len:
        size += 1
    data = np.empty(message_len, dtype=np.uint8)
    ok = ctypes.c_int(0)
    cs, rs = np.empty(row_n, dtype=np.uint8), np.empty(size, dtype=np.uint8)
    _check(lib().mzk_rs2d_decode(int(col_n), int(row_n), _p(c), int(message_len), _p(data), ctypes.byref(ok), _p(cs), _p(rs)))
    res = data if ok.value else None
    return (res, cs, rs) if with_status else res


def rs2d_decode_dev(col_n, row_n, d_code, message_len, d_data, d_ok, d_col_status=None, d_row_status=None, stream=None):
    opt = lambda p: int(p) if p else None
    _check(lib().mzk_rs2d_decode_dev(int(col_n), int(row_n), int(d_code), int(message_len), int(d_data), int(d_ok), opt(d_col_status), opt(d_row_status), stream))


# ---- Celestia's commitment (das/celestia.rs over algebra/merkle.rs): squares are numpy uint8, roots 32 bytes ---------------------------
DAS_PATH_MAX = _C["MZK_DAS_PATH_MAX"]      # entries a path can have: floor(log2 255) + 1
DAS_OUT_OF_RANGE = 255     # depths[s] of a position outside the grid (open_dev)


DAS_PLAN_FIELDS = _abi.index_names("MZK_DAS_PLAN_WORDS")


def das_plan(rows, cols, squares=1):
    """What the commitment of `squares` squares of rows x cols symbols launches, as a dict keyed after the MZK_DAS_PLAN_* constants
    (mzk_das_plan_get).  Host only: no GPU needed."""
    p = np.zeros(len(DAS_PLAN_FIELDS), dtype=np.uint64)
    _check(lib().mzk_das_plan_get(int(rows), int(cols), int(squares), _p(p)))
    return {n: int(v) for n, v in zip(DAS_PLAN_FIELDS, p)}


def _squares3d(code, what):
    a = np.ascontiguousarray(code, dtype=np.uint8)
    if a.ndim == 2:
        a = a.reshape((1,) + a.shape)
    if a.ndim != 3:
        raise MzkError(-5, "%s: expected squares x rows x cols bytes, got shape %s" % (what, a.shape))
    return a


def das_commit(code):
    """Celestia::commit (das/celestia.rs:73-113) of every square of `code` (squares x rows x cols bytes, or one rows x cols square):
    (row_roots squares x rows x 32, col_roots squares x cols x 32, data_roots squares x 32)."""
    a = _squares3d(code, "das_commit")
    q, r, c = a.shape
    rr, cr, dr = np.empty((q, r, 32), dtype=np.uint8), np.empty((q, c, 32), dtype=np.uint8), np.empty((q, 32), dtype=np.uint8)
    _check(lib().mzk_das_commit(_p(a), r, c, q, _p(rr), _p(cr), _p(dr)))
    return rr, cr, dr


def das_commit_dev(d_code, rows, cols, row_stride, square_stride, squares, d_row_roots, d_col_roots, d_data_roots, stream=None):
    """mzk_das_commit_dev: device pointers (ints); d_row_roots / d_col_roots may be None.  Only enqueues."""
    opt = lambda p: int(p) if p else None
    _check(lib().mzk_das_commit_dev(int(d_code), int(rows), int(cols), int(row_stride), int(square_stride), int(squares), opt(d_row_roots),
                                    opt(d_col_roots), int(d_data_roots), stream))


class DasGrid:
    """mzk_das_grid: the row and column trees of a batch of squares kept on the device.  DasGrid(code) builds from host bytes;
    DasGrid.from_device(...) from a view in device memory on a caller stream (only enqueues)."""

    def __init__(self, code=None, _handle=None, _shape=None):
        if _handle is not None:
            self._h, self.shape = _handle, _shape
            return
        a = _squares3d(code, "DasGrid")
        h = ctypes.c_void_p()
        _check(lib().mzk_das_grid_build(_p(a), a.shape[1], a.shape[2], a.shape[0], ctypes.byref(h)))
        self._h, self.shape = h, a.shape

    @classmethod
    def from_device(cls, d_code, rows, cols, row_stride, square_stride, squares, stream=None):
        h = ctypes.c_void_p()
        _check(lib().mzk_das_grid_build_dev(int(d_code), int(rows), int(cols), int(row_stride), int(square_stride), int(squares), ctypes.byref(h), stream))
        return cls(_handle=h, _shape=(int(squares), int(rows), int(cols)))

    def roots(self):
        """(row_roots, col_roots, data_roots) as das_commit returns them"""
        q, r, c = self.shape
        rr, cr, dr = np.empty((q, r, 32), dtype=np.uint8), np.empty((q, c, 32), dtype=np.uint8), np.empty((q, 32), dtype=np.uint8)
        _check(lib().mzk_das_grid_roots(self._h, _p(rr), _p(cr), _p(dr)))
        return rr, cr, dr

    def open(self, positions):
        """Merkle::open of every (square, row, col, is_row) of `positions` (count x 4): (paths count x 8 x 32, entry_lens count x 8,
        depths count, leaves count).  depths[s] = 0: the reference does not terminate on that sample."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64).reshape(-1, 4)
        n = pos.shape[0]
        paths, lens = np.zeros((n, DAS_PATH_MAX, 32), dtype=np.uint8), np.zeros((n, DAS_PATH_MAX), dtype=np.uint8)
        depths, leaves = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        _check(lib().mzk_das_grid_open(self._h, _p(pos), n, _p(paths), _p(lens), _p(depths), _p(leaves)))
        return paths, lens, depths, leaves

    def open_dev(self, d_positions, count, d_paths, d_entry_lens, d_depths, d_leaves, stream=None):
        """mzk_das_grid_open_dev: device pointers (ints).  Only enqueues, behind the build."""
        _check(lib().mzk_das_grid_open_dev(self._h, int(d_positions), int(count), int(d_paths), int(d_entry_lens), int(d_depths), int(d_leaves), stream))

    def close(self):
        if self._h:
            lib().mzk_das_grid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- Rescue-Prime (zkstark/rescueprime.rs): batched hashes, chains and traces, one chain per lane ----------------------------------------
RESCUE_MAX_M, RESCUE_MAX_ROUNDS = _C["MZK_RESCUE_MAX_M"], _C["MZK_RESCUE_MAX_ROUNDS"]
RESCUE_PLAN_FIELDS = _abi.index_names("MZK_RESCUE_PLAN_WORDS")


def _exp4(e):
    e = int(e)
    if e < 0 or e >> 256:
        raise MzkError(-1, "rescue: alphainv = %d is outside 0 .. 2^256 - 1" % e)
    return to_limbs([e], 4)


def rescue_plan(fid, m, n, alpha, alphainv, batch=0):
    """What a handle of these parameters runs for `batch` chains, as a dict keyed after the MZK_RESCUE_PLAN_* constants
    (mzk_rescue_plan_get).  Host only: no GPU needed."""
    p = np.zeros(len(RESCUE_PLAN_FIELDS), dtype=np.uint64)
    _check(lib().mzk_rescue_plan_get(int(fid), int(m), int(n), int(alpha), _p(_exp4(alphainv)), int(batch), _p(p)))
    return {k: int(v) for k, v in zip(RESCUE_PLAN_FIELDS, p)}


class RescuePrime:
    """mzk_rescue: Rescue-Prime over field `fid` with state width m and n rounds; mds m x m (nested or flat, row-major) and 2 n m round
    constants as ints.  Elements travel as numpy uint64 (count x limbs); the _dev forms take device pointers (ints) and only enqueue."""

    def __init__(self, fid, m, n, alpha, alphainv, mds, round_constants):
        self.fid, self.m, self.n, self.alpha, self.alphainv = int(fid), int(m), int(n), int(alpha), int(alphainv)
        self.rows = self.n + 1
        flat = [int(v) for row in mds for v in (row if isinstance(row, (list, tuple)) else [row])]
        self._h = ctypes.c_void_p()
        _check(lib().mzk_rescue_new(self.fid, int(m), int(n), self.alpha, _p(_exp4(alphainv)), _p(to_limbs(flat, LIMBS[self.fid])),
                                    _p(to_limbs([int(v) for v in round_constants], LIMBS[self.fid])), ctypes.byref(self._h)))

    def _inputs(self, inputs):
        if isinstance(inputs, np.ndarray):
            return _arr(self.fid, inputs)
        return to_limbs([int(v) for v in inputs], LIMBS[self.fid])

    def hash(self, inputs, links=1):
        """outputs (batch * links x limbs): row b * links + l is the output of link l of the chain from inputs[b]"""
        x = self._inputs(inputs)
        out = np.zeros((x.shape[0] * int(links), LIMBS[self.fid]), dtype=np.uint64)
        _check(lib().mzk_rescue_hash(self._h, _p(x), x.shape[0], int(links), _p(out)))
        return out

    def trace(self, inputs, links=1, trace_stride=None, traces=None, with_outputs=True):
        """(traces (batch * links x trace_stride x limbs), outputs or None).  traces: an array to write into -- elements of a slot past
        the last row keep what they hold."""
        x = self._inputs(inputs)
        stride = self.rows * self.m if trace_stride is None else int(trace_stride)
        slots = x.shape[0] * int(links)
        if traces is None:
            traces = np.zeros((slots, stride, LIMBS[self.fid]), dtype=np.uint64)
        assert traces.dtype == np.uint64 and traces.flags["C_CONTIGUOUS"] and traces.size >= slots * stride * LIMBS[self.fid]
        out = np.zeros((slots, LIMBS[self.fid]), dtype=np.uint64) if with_outputs else None
        _check(lib().mzk_rescue_trace(self._h, _p(x), x.shape[0], int(links), _p(traces), int(stride), _p(out) if with_outputs else None))
        return traces, out

    def hash_dev(self, d_inputs, batch, links, d_outputs, stream=None):
        _check(lib().mzk_rescue_hash_dev(self._h, int(d_inputs), int(batch), int(links), int(d_outputs), stream))

    def trace_dev(self, d_inputs, batch, links, d_traces, trace_stride, d_outputs=None, stream=None):
        _check(lib().mzk_rescue_trace_dev(self._h, int(d_inputs), int(batch), int(links), int(d_traces), int(trace_stride),
                                          int(d_outputs) if d_outputs else None, stream))

    def close(self):
        if self._h:
            lib().mzk_rescue_free(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
