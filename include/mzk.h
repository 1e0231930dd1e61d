/* mzk.h -- C ABI of the MI355X-native MSM / NTT prover path for MyZKP.
 *
 * The reference has no FFI for this path; this header defines the seam.  Each entry
 * point names the reference call site it stands behind (paths relative to myzkp/src/modules/).
 * A Rust maintainer binds these with an `extern "C"` block (INTEGRATION.md shows the shim).
 *
 * Conventions (taken from the reference's only device boundary, examples/sumcheck):
 *   - field elements cross the boundary in STANDARD form as little-endian u64 limbs, canonical in
 *     [0, p): 4 limbs for BN254 Fr/Fq, 2 limbs for M128      (examples/sumcheck/src/utils.rs:51-72)
 *   - an affine G1 point is x||y (8 limbs); the all-zero encoding is the point at infinity
 *     ((0,0) is not on y^2 = x^3 + 3)
 *   - every function returns MZK_OK (0) or a negative MZK_E_* code; mzk_last_error() has the text.
 *     The Rust shim asserts the reference's own preconditions first so that panic messages stay
 *     identical (ntt.rs:8-23, curve.rs:174-176), then `expect()`s the status.
 *   - blocking, one in-flight call per process (the reference is single-threaded); one process per
 *     GPU.  The *_dev variants take device pointers + a hipStream_t and only enqueue work.
 *   - all entry points of a context share one grow-only workspace.  Calls on DIFFERENT streams are ordered by the
 *     library (each entry point waits on the previous one's completion event before touching the workspace and
 *     records its own), so results are correct on any stream; work on one context never overlaps.  Calls must
 *     still come from one host thread at a time: a call that arrives while another thread is inside the library returns
 *     MZK_E_BUSY without touching any state (calls nested on ONE thread -- the challenge callback of mzk_fri_commit calling back
 *     in -- are fine; a nested call that needs scratch the running call holds is refused with MZK_E_ARG).
 */
#ifndef MZK_H
#define MZK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { MZK_FIELD_FR = 0,   /* ModEIP197 / FqOrder: algebra/field.rs:428-431, curve/bn128.rs:30 */
       MZK_FIELD_M128 = 1, /* M128 = 1 + 407*2^119: zkstark/fri.rs:408 */
       MZK_FIELD_FQ = 2,   /* BN128Modulus: curve/bn128.rs:19-22 (point coordinates only) */
       MZK_FIELD_M64 = 3,  /* Goldilocks, p = 2^64 - 2^32 + 1: zkstark/fri.rs:409 */
       MZK_FIELD_M64X3 = 4 /* ExtendedFieldElement<M64, Ip3>, Ip3 = x^3 - x + 1: zkstark/fri.rs:410-421 */ };
/* The Goldilocks ids (the second instantiation of the reference's FRI, test_fri_efield, fri.rs:546-594).
 *   Wire format: M64 = one canonical uint64_t (< p) per element; M64X3 = three consecutive canonical uint64_t c0, c1, c2 of
 *   c0 + c1 x + c2 x^2 (24 bytes, array of structures).  A scalar parameter of id 4 (root, offset, alpha) has the same three words.
 *   Served by: mzk_root_of_unity, mzk_ntt / _dev / _batch / _batch_dev, mzk_coset_lde / _dev / _batch / _batch_dev, mzk_fri_fold / _dev,
 *   mzk_merkle_build_field / _dev, mzk_merkle_commit_field / _dev and every call on a built tree (root, open, open_batch, open_multi,
 *   leaves, free), mzk_fri_commit, mzk_fri_commit_keep_trees / _dev, and mzk_fri_proof_layout_gl, mzk_fri_prove_gl / _dev, which
 *   serve no other id.  Every other call refuses them with MZK_E_ARG like any id it does not serve (mzk_fri_prove,
 *   mzk_fri_prove_dev, mzk_fri_proof_layout, mzk_stark_*, mzk_fast_*, mzk_fft_multiply, mzk_mpoly_*, mzk_poly_*, the *_signed Merkle
 *   and FRI forms, mzk_merkle_commit_field_batch*, mzk_ntt_multi*, mzk_ntt_columns_dev, the synth / selftest / probe calls).
 *   Restriction for id 4: omega, generator and offset must lie in the base field (c1 = c2 = 0), MZK_E_ARG otherwise -- every element
 *   of 2-power order does, and the reference's only instantiation passes base values for all three; a transform root with c1 or
 *   c2 != 0 fails the root-order check (MZK_E_ROOT_ORDER).  alpha and the data are unrestricted.
 *   Leaves: the library's restatement of bincode, unpinned against Rust like the leaves of the other fields.  Base element v: sign
 *   byte (0 for zero, else 1), u64 LE digit count, u32 LE digits (9 .. 17 bytes).  Extension element, as
 *   ExtendedFieldElement{poly: Polynomial{coef}}: u64 LE count k of coefficients after trimming trailing zero coefficients
 *   (0 <= k <= 3), then k base leaves (8 .. 59 bytes; a zero coefficient below a non-zero one is its 9-byte leaf).
 *   mzk_merkle_leaves returns 1 or 3 words per element, flags 0.  A path stride below the longest possible leaf is accepted, as for
 *   Fr: MZK_E_LENGTH only when a sibling leaf that is actually opened does not fit (64 holds every leaf of every field).
 *   mzk_fri_commit*: alpha_out takes 1 or 3 words; `negative` must be NULL (MZK_E_ARG): elements are canonical, the signs the
 *   reference's BigInt coefficients may carry are not represented; an id-4 round of ONE element is MZK_E_LENGTH (its 59-byte leaf
 *   does not fit the 48-byte root slot). */

enum { MZK_OK = 0,
       MZK_E_ARG = -1,        /* null pointer / bad field id */
       MZK_E_NOT_POW2 = -2,   /* ntt.rs:8-11 "cannot compute ntt of non-power-of-two sequence" */
       MZK_E_ROOT_ORDER = -3, /* ntt.rs:15-18 "primitive root must be nth root of unity" */
       MZK_E_ROOT_PRIM = -4,  /* ntt.rs:19-22 "primitive root is not primitive nth root of unity" */
       MZK_E_LENGTH = -5,     /* slice-index / usize-underflow panics (ntt.rs:265, polynomial.rs:162) */
       MZK_E_RANGE = -6,      /* operand not canonical (>= modulus) where the ABI requires it */
       MZK_E_HIP = -7,        /* HIP runtime error */
       MZK_E_NOGPU = -8,      /* no gfx950 device visible: there is NO CPU fallback */
       MZK_E_CALLBACK = -9,   /* a caller-supplied callback reported failure (mzk_fri_commit's challenge) */
       MZK_E_IO = -10,        /* file could not be opened / read / written, or is not a valid dump (mzk_srs_save/load) */
       MZK_E_BUSY = -11,      /* another host thread is inside a call: the library serves one call at a time (see above);
                                 nothing was enqueued, the call may simply be repeated */
       MZK_E_NOMEM = -12      /* the device has no memory left for this call even after every idle workspace buffer of the context
                                 was released (see mzk_set_workspace_budget / mzk_trim_workspace); nothing was enqueued */ };

/* Select the device for this process, create streams/workspace.  Idempotent: when context 0 already drives
 * `device_ordinal` nothing is torn down (contexts made by mzk_init_devices, their streams and every handle stay valid);
 * use mzk_init_devices(&ordinal, 1) to go back to exactly one context.  (SURVEY 8b sketched mzk_init(n_devices);
 * one process per GPU is the primary model, so the argument is the ordinal -- mzk_init_devices is the n-device form.) */
int mzk_init(int device_ordinal);
/* One process driving several GPUs: context r = (device_ordinals[r], its own stream, workspace and table caches).
 * Duplicate ordinals are allowed (several contexts on one GPU).  Context 0 is current afterwards; every entry point
 * of this header works on the CURRENT context (mzk_ctx_select), the *_multi entry points walk all of them. */
int mzk_init_devices(const int* device_ordinals, int n_devices);
int mzk_ctx_count(void);
int mzk_ctx_select(int index);
int mzk_ctx_device(int index);   /* device ordinal of a context, -1 if it does not exist */
/* 1 when the devices of contexts a and b can reach each other's memory directly (mzk_init_devices calls
 * hipDeviceCanAccessPeer / hipDeviceEnablePeerAccess for every pair of distinct ordinals; same device = 1), else 0:
 * mzk_ntt_multi's exchanges then stage through host memory inside the runtime -- correct, slower. */
int mzk_ctx_peer_enabled(int index_a, int index_b);
void* mzk_ctx_stream(int index); /* the context's own hipStream_t (non-blocking), usable as the `stream` of its *_dev calls */
/* Two contexts on ONE device keep two calls in flight (each has its own stream and workspace; an mzk_srs handle is
 * plain device memory and serves every context of its device): alternating commits between them overlaps the
 * latency-bound tail of one MSM with the sort / accumulate of the next -- 2^20 pairs: 1.72 -> 1.55 ms per commit. */
void mzk_shutdown(void);
const char* mzk_last_error(void);
/* ABI version: bump on any signature change. */
int mzk_abi_version(void);

/* Size limits (tests/test_gpu_max_sizes.py runs them on one MI355X; profiles/r02u_max_sizes.txt has the timings):
 *   MSM / commit / open / SRS handles   n <= 2^27 pairs (MZK_E_ARG above; 2^27 pairs x 16 windows = 2^31 sort records, and an
 *                                       SRS handle with 16-bit window tables holds 16 n points = 128 GiB at 2^27 -- pass
 *                                       with_tables = 0 to mzk_srs_from_device_ex to keep only the prepared points)
 *   transforms                          n <= 2^28 over Fr (its 2-adicity); over M128 up to 2^32 nominally, memory-bound in
 *                                       practice: in + out + (passes - 1) twiddle tables of n elements each; over M64 / M64X3
 *                                       up to 2^32 (the 2-adicity), in + out + one scratch copy (no n-sized twiddle table)
 *   Merkle leaves / path entries        at most 41 bytes over Fr, 59 over M64X3: a stride of 64 holds every leaf; FRI root slots are 48
 *   subproduct trees (mzk_fast_*)       n <= 2^27 points (the internal products are transforms of 2 n <= 2^28 points) */
/* ---- NTT family ------------------------------------------------------------------------------- */
/* ntt::ntt (algebra/ntt.rs:7-48) when inverse == 0: out[k] = sum_j in[j] * root^(j k), natural order
 * in and out, n a power of two, root a primitive n-th root.  n <= 1 copies the input.
 * ntt::intt (ntt.rs:50-64) when inverse != 0: n^-1 * ntt(root^-1, in); n == 1 copies the input.
 * `root` is the forward root in both cases, exactly as the reference's callers pass it. */
int mzk_ntt(int field_id, const uint64_t* root, const uint64_t* in, uint64_t* out, size_t n, int inverse);

/* ntt::fast_coset_evaluate (ntt.rs:254-269) incl. Polynomial::scale (polynomial.rs:167-174):
 * evaluations of the polynomial on { offset * generator^i : i < order }.  n_coef > order is the
 * reference's usize underflow -> MZK_E_LENGTH. */
int mzk_coset_lde(int field_id, const uint64_t* coef, size_t n_coef, const uint64_t* offset,
                  const uint64_t* generator, uint64_t* out, size_t order);

/* Polynomial::fft_multiply (polynomial.rs:242-276): m = la+lb-1 and n = next_pow2(m) come from the stored lengths,
 * trailing zeros included.  omega must be a primitive n-th root of unity.  The reference's private fft takes any
 * omega unchecked; the transforms here check theirs like ntt::ntt: MZK_E_ROOT_ORDER when omega^n != 1,
 * MZK_E_ROOT_PRIM when omega^(n/2) == 1, MZK_E_RANGE when it is not canonical, MZK_E_ARG when it is NULL.  omega is
 * not read when n == 1 (1 x 1) or when an operand is empty.  An empty operand (la == 0 or lb == 0, not both) gives the
 * empty product, *out_len = 0, as the reference's resize(n) and trim do; la == lb == 0 is its usize underflow,
 * MZK_E_LENGTH.  out holds la+lb-1 elements; *out_len = length after the reference's truncate(m) and
 * trailing-zero trim (0 for an all-zero operand). */
int mzk_fft_multiply(int field_id, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                     const uint64_t* omega, uint64_t* out, size_t* out_len);

/* ntt::fast_multiply (ntt.rs:66-116): root must be canonical (MZK_E_RANGE) and primitive of order root_order
 * (MZK_E_ROOT_ORDER / MZK_E_ROOT_PRIM, the assertions :75-76, made before anything else).  A zero operand (empty or
 * all zero coefficients) gives *out_len = 0.  With degree = the sum of the operands' degrees after trimming: below 8
 * the trimmed schoolbook product (`lhs * rhs`), whatever root_order is; else order = root_order halved while
 * degree < order / 2, the sub-root picked here, and the result is the `order` coefficients of the cyclic convolution,
 * NOT trimmed (*out_len = order; it wraps around when degree >= order, i.e. when nothing could be halved).  The stored
 * lengths, trailing zeros included, must not exceed `order`: the reference hands a longer operand to ntt as it is and
 * panics there, MZK_E_LENGTH; an order that is no power of two is MZK_E_NOT_POW2.  out must hold
 * max(root_order, la+lb) elements. */
int mzk_fast_multiply(int field_id, const uint64_t* a, size_t la, const uint64_t* b, size_t lb,
                      const uint64_t* root, size_t root_order, uint64_t* out, size_t* out_len);

/* get_nth_root_of_m128 (zkstark/fri.rs:423-447) and the Fr analogue the reference lacks
 * (omega_2^28 = 5^((r-1)/2^28)).  Pure host parameter math. */
int mzk_root_of_unity(int field_id, unsigned log2_n, uint64_t* out);

/* ---- MSM / KZG -------------------------------------------------------------------------------- */
/* Polynomial::eval_with_powers_on_curve (algebra/polynomial.rs:156-165) = commit_kzg
 * (algebra/kzg.rs:57-59): sum_i scalars[i] * points[i].  Scalars need not be canonical (the
 * reference sanitizes, polynomial.rs:162): any 256-bit value is reduced mod r.  n == 0 -> infinity.
 * Points must lie on y^2 = x^3 + 3 (every G1Point the reference produces does): the kernels use the curve's
 * endomorphism (k P = k1 P + k2 phi(P), GLV), an identity of the prime-order group, not of arbitrary (x, y) pairs. */
int mzk_msm_g1_bn254(const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t out_xy[8]);

/* setup_kzg (kzg.rs:27-40), G1 part, trapdoor supplied by the caller: powers[i] = alpha^i * g1,
 * i = 0..=max_d  ((max_d+1) * 8 limbs out). */
int mzk_kzg_setup_g1(const uint64_t alpha[4], const uint64_t g1_xy[8], size_t max_d, uint64_t* powers_xy);

/* open_kzg (kzg.rs:61-72): y = f(u); w = MSM((f - y)/(X - u), powers). */
int mzk_kzg_open(const uint64_t* coef, size_t n, const uint64_t u[4], const uint64_t* powers_xy,
                 uint64_t y[4], uint64_t w_xy[8]);

/* ---- "next" rows of the path -------------------------------------------------------- */
/* batch_open_kzg (kzg.rs:74-88): ys[i] = f(us[i]); w = MSM((f - I)/prod(X - us[i]), powers) where I
 * interpolates (us, ys).  The us must be distinct (the reference's interpolate divides by their
 * differences).  ys: k*4 limbs out. */
int mzk_kzg_batch_open(const uint64_t* coef, size_t n, const uint64_t* us, size_t k, const uint64_t* powers_xy,
                       uint64_t* ys, uint64_t w_xy[8]);
/* prove_degree_bound (kzg.rs:121-134): MSM(f * X^(max_d - d), powers), max_d = n_powers - 1.
 * d > max_d (usize underflow) or a product longer than the SRS (index panic) -> MZK_E_LENGTH. */
int mzk_kzg_prove_degree_bound(const uint64_t* coef, size_t n, const uint64_t* powers_xy, size_t n_powers,
                               size_t d, uint64_t out_xy[8]);
/* ntt::fast_coset_divide (algebra/ntt.rs:271-330; FastStark::prove's quotients, zkstark/fast_stark.rs:265):
 * both polynomials scaled onto the coset offset*<root>, forward transforms, pointwise el * r.inverse()
 * (inverse(0) = 0, field.rs:209-232), inverse transform, first lhs.degree() - rhs.degree() + 1 coefficients scaled
 * back by offset^-1.  degree < 8 returns lhs / rhs (true long division, trimmed).  The reference's assertions map to
 * MZK_E_ROOT_ORDER / MZK_E_ROOT_PRIM (ntt.rs:282-283), MZK_E_ARG (rhs zero, :284), MZK_E_LENGTH (rhs.degree() >=
 * lhs.degree(), :285 -- a zero lhs included).  out must hold ll coefficients; *out_len receives the count. */
int mzk_fast_coset_divide(int field_id, const uint64_t* lhs, size_t ll, const uint64_t* rhs, size_t lr, const uint64_t* offset,
                          const uint64_t* root, size_t root_order, uint64_t* out, size_t* out_len);
/* The same division for `count` numerators in HBM over ONE denominator in HBM (FastStark::prove divides every transition polynomial by
 * the one transition zerofier, fast_stark.rs:261-273).  Numerator i = d_lhs[i * lhs_stride ..], lhs_lens[i] coefficients (need not be
 * trimmed: the trimmed lengths of the numerators and of the denominator are found on the device first, one wait); quotient i =
 * d_out[i * out_stride ..], out_lens[i] coefficients and zeros behind them up to out_stride.  Every row is bit-identical to
 * mzk_fast_coset_divide of that row, with the same error mapping (the first offending row decides) and the same degree < 8 branch (at
 * most 8 coefficients of such a row visit the host).  Rows whose squared-down order (ntt.rs:298-302) agrees share one batched forward
 * transform, one denominator transform, one division launch whose inversion chain serves all of them, one batched inverse transform and
 * one scale-back launch.  Also MZK_E_LENGTH: lhs_lens[i] > lhs_stride, a quotient longer than out_stride.  lhs_lens, offset, root and
 * out_lens are host memory; d_lhs and d_rhs complete on `stream` before the call (canonical, not checked); d_out must not overlap them;
 * returns when d_out is complete.  On an error d_out and out_lens are undefined (every assertion is checked before any quotient is
 * enqueued).  Rows of degree < 8 cost two more waits for all of them together.  count == 0: MZK_OK. */
int mzk_fast_coset_divide_batch_dev(int field_id, const void* d_lhs, size_t lhs_stride, const size_t* lhs_lens, size_t count, const void* d_rhs,
                                    size_t rhs_len, const uint64_t* offset, const uint64_t* root, size_t root_order, void* d_out, size_t out_stride,
                                    size_t* out_lens, void* stream);

/* ntt::fast_zerofier / fast_evaluate / fast_interpolate (algebra/ntt.rs:118-252; FastStark::prove interpolates every
 * trace register with fast_interpolate, zkstark/fast_stark.rs:209, and builds its transition zerofier with
 * fast_zerofier, :53).  Subproduct trees on the device (O(n log^2 n); the reference's remainders are O(n^2)).
 *   zerofier:    prod (X - domain[i]).  n = 0 -> empty; n < 8 -> n + 1 coefficients (the schoolbook branch trims);
 *                n >= 8 -> next_pow2(n + 1) coefficients, zero padded (fast_multiply does not trim its NTT branch).
 *                out must hold max(n + 1, next_pow2(n + 1)) elements.  Over the first n points of a power-of-two subgroup with
 *                at most 64 of its points missing (FastStark's transition zerofier, fast_stark.rs:53-57) the coefficients
 *                come from one launch: Z = (X^N - 1) / prod over the missing points, expanded by partial fractions.
 *   evaluate:    out[i] = f(domain[i]), i < n (m coefficients, any m).
 *   interpolate: the polynomial of degree < n through (domain[i], values[i]), trimmed like the reference's final sum;
 *                n = 1 -> [values[0]] untrimmed.  A repeated domain point gets weight inverse(0) = 0, as in the
 *                reference (field.rs:209-232 via ntt.rs:233-242).  out must hold n elements.
 *                When the domain is the first n points 1, g, g^2 ... of a subgroup of order next_pow2(n) with at most 64 of its
 *                points missing -- FastStark's trace_domain = omicron^i (fast_stark.rs:197-215) -- the same coefficients come from
 *                ONE inverse transform of the values extended by the interpolant's values at the missing points (a dot product
 *                each, weights kept with the cached plan); every other domain goes through the tree.
 * root / root_order: the two reference assertions (MZK_E_ROOT_ORDER / MZK_E_ROOT_PRIM); where the reference's
 * internal zerofier products would exceed root_order (it then wraps around or panics inside ntt) -> MZK_E_LENGTH. */
int mzk_fast_zerofier(int field_id, const uint64_t* domain, size_t n, const uint64_t* root, size_t root_order, uint64_t* out, size_t* out_len);
int mzk_fast_evaluate(int field_id, const uint64_t* coef, size_t m, const uint64_t* domain, size_t n, const uint64_t* root, size_t root_order,
                      uint64_t* out);
int mzk_fast_interpolate(int field_id, const uint64_t* domain, const uint64_t* values, size_t n, const uint64_t* root, size_t root_order,
                         uint64_t* out, size_t* out_len);
/* fast_interpolate of `batch` value vectors over ONE domain -- the registers of a trace (fast_stark.rs:203-215 calls it
 * once per register with the same trace_domain): the subproduct tree and the derivative values Z'(d_i), ~80 % of one
 * interpolation, are built once, and the registers share the launches of the up-sweep.  values: batch * n elements; out: batch rows of n elements (row r holds out_lens[r]
 * coefficients, zero-padded).  Each row bit-identical to the single call. */
int mzk_fast_interpolate_batch(int field_id, const uint64_t* domain, const uint64_t* values, size_t n, size_t batch, const uint64_t* root,
                               size_t root_order, uint64_t* out, size_t* out_lens);
/* The same with the values and the coefficients in HBM -- a prover uploads its trace once and the coefficients feed mzk_coset_lde_batch_dev
 * without visiting the host (fast_stark.rs:209-231: interpolate, then fast_coset_evaluate, per register).  d_values: batch rows of n
 * elements, canonical (not checked), complete on `stream` (a hipStream_t) before the call; d_out: batch rows of n elements, row r holds
 * out_lens[r] coefficients and zeros behind them.  domain and out_lens are host memory (the domain keys the cached plan, the lengths are
 * what the caller builds its Polynomial values from).  Returns when d_out is complete.  Rows bit-identical to mzk_fast_interpolate_batch. */
int mzk_fast_interpolate_batch_dev(int field_id, const uint64_t* domain, const void* d_values, size_t n, size_t batch, const uint64_t* root,
                                   size_t root_order, void* d_out, size_t* out_lens, void* stream);

/* FRI commit-loop split-and-fold (zkstark/fri.rs:182-193):
 * out[i] = 2^-1 ((1 + alpha/(offset omega^i)) c[i] + (1 - alpha/(offset omega^i)) c[n/2 + i]), i < n/2,
 * sanitized.  offset must be non-zero and omega a root of order n (as FRI::commit maintains). */
int mzk_fri_fold(int field_id, const uint64_t* codeword, size_t n, const uint64_t* alpha, const uint64_t* offset,
                 const uint64_t* omega, uint64_t* out);
int mzk_fri_fold_dev(int field_id, const void* d_codeword, size_t n, const uint64_t* alpha_host,
                     const uint64_t* offset_host, const uint64_t* omega_host, void* d_out, void* stream);

/* ---- SHA3-256 Merkle trees over codewords (algebra/merkle.rs:15-46 as called from zkstark/fri.rs:160-166,
 * 236-249 and fast_stark.rs:64-68, 237-241): leaves are bincode(FiniteFieldElement) of the canonical elements and
 * are not hashed themselves; a one-leaf tree commits to the leaf bytes.  n = 0 is an error (the reference recurses
 * forever).  Any n >= 1 is accepted like merkle.rs:15-25 does (mid = len / 2): the provers only commit to
 * power-of-two codewords, which take the fast path; other counts are reduced to the power-of-two tree over the
 * 2^floor(log2 n) one- or two-leaf subtrees at the bottom.  Merkle::open on a ragged tree only terminates when its
 * descent ends on a two-leaf slice (merkle.rs:32-34); for the one-leaf half of a three-leaf slice it recurses
 * forever, and mzk_merkle_open returns MZK_E_LENGTH there.  Paths have floor(log2 n) or floor(log2 n) + 1 entries.  A handle keeps its own copy of the leaves
 * and all node levels in HBM so that many paths can be opened against one codeword. */
typedef struct mzk_merkle mzk_merkle;
int mzk_merkle_build_field(int field_id, const uint64_t* elems, size_t n, mzk_merkle** out);
int mzk_merkle_build_field_dev(int field_id, const void* d_elems, size_t n, mzk_merkle** out, void* stream);
/* generic Merkle::commit input: leaf i = leaves[offsets[i] .. offsets[i+1]) (n + 1 offsets), any lengths */
int mzk_merkle_build_bytes(const uint8_t* leaves, const uint64_t* offsets, size_t n, mzk_merkle** out);
/* root: 32 bytes, or the leaf itself when n == 1 (merkle.rs:17-19); cap = capacity of `root` */
int mzk_merkle_root(const mzk_merkle* tree, uint8_t* root, size_t cap, size_t* root_len);
/* Merkle::open (merkle.rs:28-46): entry k of the bottom-up path goes to path + k * stride, its length to
 * path_len[k] (entry 0 is the sibling leaf verbatim, the rest are 32-byte digests); *depth = log2 n entries. */
int mzk_merkle_open(const mzk_merkle* tree, size_t index, uint8_t* path, size_t stride, uint64_t* path_len, size_t* depth);
/* `count` openings of one tree in one gather and one copy -- the FRI query phase opens three indices per colinearity test
 * and round (fri.rs:211-260; the reference's Merkle::open re-hashes the whole tree for each).  Path q, entry l:
 * paths[(q * depth + l) * stride ..], length path_lens[q * depth + l]; *depth entries per path, each path exactly what
 * mzk_merkle_open returns for indices[q].  Trees over field elements with a power-of-two leaf count (every codeword the
 * provers commit to); byte-leaf and ragged trees: MZK_E_ARG, open those one by one. */
int mzk_merkle_open_batch(const mzk_merkle* tree, const uint64_t* indices, size_t count, uint8_t* paths, size_t stride, uint64_t* path_lens,
                          size_t* depth);
/* Openings of SEVERAL trees in one call -- the query phase of FRI::prove (fri.rs:127-137 with reveal, :211-260) opens the a / b
 * indices in round i's tree and the c indices in round i+1's, for every round: with the trees of mzk_fri_commit_keep_trees one
 * call, one copy back and one synchronisation instead of two of each per round.  Tree t takes the next counts[t] entries of
 * `indices`; its paths follow tree t-1's in paths / path_lens, each tree laid out as mzk_merkle_open_batch lays it out, with
 * depths[t] entries per path.  counts[t] == 0 skips tree t.  Same kinds of trees as mzk_merkle_open_batch. */
int mzk_merkle_open_multi(const mzk_merkle* const* trees, size_t n_trees, const uint64_t* indices, const size_t* counts, uint8_t* paths,
                          size_t stride, uint64_t* path_lens, size_t* depths);
void mzk_merkle_free(mzk_merkle* tree);
/* one-shot Merkle::commit(codeword.map(bincode::serialize)) */
int mzk_merkle_commit_field(int field_id, const uint64_t* elems, size_t n, uint8_t* root, size_t cap, size_t* root_len);
int mzk_merkle_commit_field_dev(int field_id, const void* d_elems, size_t n, uint8_t* root_host, size_t cap, size_t* root_len,
                                void* stream);
/* Merkle::commit (merkle.rs:15-25) of `batch` codewords of n elements each, stored back to back -- the per-register loop of
 * the provers (fast_stark.rs:231-243: fast_coset_evaluate, serialize, Merkle::commit for every register) as one call.
 * roots: batch * 32 bytes (host).  n must be a power of two >= 2 (every codeword the provers commit to is; other leaf
 * counts: the single-tree calls).  The upper levels of a tree are one dependent hash per level on a nearly empty GPU; side
 * by side the trees share them: 16 codewords of 2^16 elements in 0.26 ms instead of 16 x 0.18. */
int mzk_merkle_commit_field_batch(int field_id, const uint64_t* elems, size_t n, size_t batch, uint8_t* roots);
int mzk_merkle_commit_field_batch_dev(int field_id, const void* d_elems, size_t n, size_t batch, uint8_t* roots, void* stream);
int mzk_merkle_commit_bytes(const uint8_t* leaves, const uint64_t* offsets, size_t n, uint8_t* root, size_t cap, size_t* root_len);

/* Elements whose BigInt the reference left NEGATIVE (F6: `%` keeps the sign, field.rs:98-110; only sanitize() folds
 * them into [0, p)): bincode writes Sign::Minus and the MAGNITUDE, so the leaf differs from the canonical element's.
 * The *_signed forms take the magnitudes (canonical limbs of |v|, |v| < p) plus one byte per element (1 = negative)
 * and hash exactly those bytes; all arithmetic afterwards uses the canonical representative p - |v|.
 * mzk_fri_commit_signed: round 0 commits to the unsanitized initial codeword like fri.rs:160-166 does (every later
 * codeword is sanitized by the fold, fri.rs:190); codewords_out[0..n) receives the canonical values. */
int mzk_merkle_build_field_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, mzk_merkle** out);
int mzk_merkle_commit_field_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, uint8_t* root, size_t cap,
                                   size_t* root_len);

/* FRI::commit (zkstark/fri.rs:144-209), codewords resident in HBM across all rounds.  Round r: the Merkle root of
 * codeword_r is handed to `challenge` (which owns the proof stream: push the root, and unless `last` sample
 * alpha = F::sample(prover_fiat_shamir(32)) into alpha_out, canonical limbs); then split-and-fold, omega and
 * offset squared.  roots: num_rounds x 48 bytes (root_len[r] = 32, or the leaf length once a codeword has one
 * element); codewords_out: the num_rounds codewords concatenated (n + n/2 + ... elements). */
/* The callback returns 0 on success; any other value aborts the loop with MZK_E_CALLBACK (a transcript error must
 * never let the prover fold with a default challenge).  alpha_out is pre-filled with all-ones (non-canonical). */
typedef int (*mzk_fri_challenge_fn)(void* user, int round, int last, const uint8_t* root, size_t root_len, uint64_t* alpha_out);
int mzk_fri_commit(int field_id, const uint64_t* codeword, size_t n, const uint64_t* omega, const uint64_t* offset, int num_rounds,
                   mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out);
int mzk_fri_commit_signed(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                          int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots, uint64_t* root_len, uint64_t* codewords_out);
/* The same loop (negative may be NULL: then `magnitudes` are the canonical elements), and the Merkle tree of every round
 * stays on the device for the query phase: trees_out[r] (num_rounds handles, NULL for a one-element round) opens with
 * mzk_merkle_open / mzk_merkle_open_batch exactly as Merkle::open on that round's codeword would (fri.rs:211-260); free each
 * with mzk_merkle_free. */
int mzk_fri_commit_keep_trees(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega,
                              const uint64_t* offset, int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots,
                              uint64_t* root_len, uint64_t* codewords_out, mzk_merkle** trees_out);

/* mzk_fri_commit_keep_trees with the initial codeword already in HBM (the output of mzk_coset_lde_dev), complete before the call;
 * negative: host flags as in mzk_fri_commit_signed, or NULL.  In both keep-trees forms codewords_out may be NULL: the codewords
 * then never leave the device -- the query phase takes what FRI::reveal sends (fri.rs:211-260) from the trees: the paths with
 * mzk_merkle_open_multi, the a / b / c values and the last codeword with mzk_merkle_leaves. */
int mzk_fri_commit_keep_trees_dev(int field_id, const void* d_magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega,
                                  const uint64_t* offset, int num_rounds, mzk_fri_challenge_fn challenge, void* user, uint8_t* roots,
                                  uint64_t* root_len, uint64_t* codewords_out, mzk_merkle** trees_out);
/* The elements a field-element tree was built over, at `count` positions: magnitudes (count x limbs) and, if negative != NULL,
 * their Sign::Minus flags (all 0 unless the tree was built from signed leaves). */
int mzk_merkle_leaves(const mzk_merkle* tree, const uint64_t* indices, size_t count, uint64_t* magnitudes, uint8_t* negative);

/* FRI::prove (zkstark/fri.rs:99-143) in one call: commit, the proof stream, sample_indices and reveal all run on the device; the
 * result is the reference's FriProof, packed.  The proof stream is the reference's FiatShamirTransformer started empty: bincode 1.x
 * (u64 LE lengths) of Vec<Vec<Vec<u8>>>; round r pushes vec![root_r] and, unless it is the last round, takes
 * alpha = F::sample(SHAKE256(stream)[0..32]) (the last 8 bytes big-endian); after the last root the last codeword is pushed as one
 * object of bincode(FiniteFieldElement) leaves and seed = SHAKE256(stream)[0..32]; top-level indices: Blake2b-256(seed || counter
 * as u64 LE), sample_index % (n/2), kept when their residue mod the last codeword's length is new (fri.rs:19-62).  The leaf bytes
 * are the library's restatement of bincode(FiniteFieldElement) (see the Merkle section), not pinned against a Rust vector.
 *
 * num_rounds = FRI::num_rounds(n, expansion_factor, num_colinearity_tests) (fri.rs:86-97).  Errors, before anything is enqueued:
 * bad field id, null pointer (MZK_E_ARG); n == 0 or num_rounds < 2 (MZK_E_LENGTH: the reference indexes codewords[1]);
 * n not a power of two (MZK_E_NOT_POW2); num_colinearity_tests > the last codeword's length (MZK_E_ARG, the reference's
 * "cannot sample more indices than available in last codeword" assertion); omega / offset not canonical (MZK_E_RANGE);
 * proof_cap below the layout's total (MZK_E_LENGTH).  negative (optional): Sign::Minus flags of the initial codeword, which is
 * then given as magnitudes (mzk_fri_commit_signed semantics: round 0 commits to and reveals the elements as given).
 *
 * Packed proof (mzk_fri_proof_layout gives num_rounds R and every section's byte offset and size; offsets are 8-byte aligned;
 * T = num_colinearity_tests, m = n >> (R-1), L = R-1 layers, NL = limbs per element, d_r = log2(n >> r)):
 *   MZK_FRI_STATUS         u64: 0, or 1 when sample_indices found no T distinct residues in 2^20 counters (the reference loops
 *                          forever; mzk_fri_prove then returns MZK_E_RANGE)
 *   MZK_FRI_TOP_INDICES    T x u64: top_level_indices
 *   MZK_FRI_ROOTS          R x 32 bytes: merkle_roots
 *   MZK_FRI_LAST_CODEWORD  m x NL u64: last_codeword (canonical)
 *   MZK_FRI_VALUES         for layer i, for a, b, c: T x NL u64 -- revealed_layers[i].{a,b,c}.0 (magnitudes)
 *   MZK_FRI_SIGNS          the same order, one byte per value: 1 = Sign::Minus (only round-0 values of a signed codeword)
 *   MZK_FRI_PATHS          for layer i: T paths of d_i entries for a, T of d_i for b, T of d_(i+1) for c; MZK_FRI_PATH_STRIDE
 *                          bytes per entry, zero-padded: entry 0 the sibling leaf's bytes, then 32-byte digests (Merkle::open)
 *   MZK_FRI_PATH_LENS      one u64 per path entry: its length in bytes */
enum { MZK_FRI_STATUS = 0, MZK_FRI_TOP_INDICES = 1, MZK_FRI_ROOTS = 2, MZK_FRI_LAST_CODEWORD = 3, MZK_FRI_VALUES = 4, MZK_FRI_SIGNS = 5,
       MZK_FRI_PATHS = 6, MZK_FRI_PATH_LENS = 7, MZK_FRI_SECTIONS = 8, MZK_FRI_PATH_STRIDE = 48 };
/* host only, no device work: offsets / sizes have MZK_FRI_SECTIONS entries (each may be NULL) */
int mzk_fri_proof_layout(int field_id, size_t n, size_t expansion_factor, size_t num_colinearity_tests, int* num_rounds, uint64_t* offsets,
                         uint64_t* sizes, uint64_t* total_bytes);
/* host memory in and out; returns when proof_out is complete */
int mzk_fri_prove(int field_id, const uint64_t* magnitudes, const uint8_t* negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                  size_t expansion_factor, size_t num_colinearity_tests, uint8_t* proof_out, size_t proof_cap);
/* device memory in and out (d_negative: device flags or NULL); only enqueues on `stream`: read MZK_FRI_STATUS after synchronizing */
int mzk_fri_prove_dev(int field_id, const void* d_magnitudes, const void* d_negative, size_t n, const uint64_t* omega, const uint64_t* offset,
                      size_t expansion_factor, size_t num_colinearity_tests, void* d_proof, size_t proof_cap, void* stream);

/* FRI::prove over the Goldilocks ids (MZK_FIELD_M64, MZK_FIELD_M64X3; the reference's test_fri_efield, fri.rs:546-594, calls
 * fri.prove): the same one-enqueue prover with entry points of its own, because the packed layout differs.  Field ids 0 .. 2 get
 * MZK_E_ARG ("fri_prove_gl: bad field id N").  There is no `negative` argument: these fields take canonical elements only.
 *
 * alpha_r = F::sample(SHAKE256(stream)[0..32]) is the wrapping accumulator (the last 8 digest bytes big-endian) reduced mod p --
 * it can exceed p --, embedded as (v, 0, 0) for id 4 (efield.rs:180-186).  The last codeword is pushed as one object of m strings,
 * each the element's leaf bytes (9 .. 17 bytes for M64, 8 .. 59 for M64X3; see the Goldilocks note at the top).
 *
 * Packed proof: the eight sections of mzk_fri_proof_layout in the same order, with NL = 1 or 3 words per element; MZK_FRI_SIGNS is
 * present and all zero (unpackers are shared); a path entry takes MZK_FRI_PATH_STRIDE_GL bytes, zero padded (an M64X3 sibling leaf
 * is up to 59 bytes).  Errors, before anything is enqueued: those of mzk_fri_prove, with the parameter rules of the Goldilocks
 * ids -- omega / offset not canonical MZK_E_RANGE, outside the base field for id 4 MZK_E_ARG.  With num_rounds >= 2 and an
 * expansion factor >= 1 the last codeword has at least two elements; expansion factor 0 without tests would halve down to one:
 * MZK_E_LENGTH. */
enum { MZK_FRI_PATH_STRIDE_GL = 64 };
/* gl_field_id: MZK_FIELD_M64 or MZK_FIELD_M64X3.  host only */
int mzk_fri_proof_layout_gl(int gl_field_id, size_t n, size_t expansion_factor, size_t num_colinearity_tests, int* num_rounds, uint64_t* offsets,
                            uint64_t* sizes, uint64_t* total_bytes);
/* host memory in and out; returns when proof_out is complete (MZK_E_RANGE when the sampler gave up, as mzk_fri_prove) */
int mzk_fri_prove_gl(int gl_field_id, const uint64_t* codeword, size_t n, const uint64_t* omega, const uint64_t* offset, size_t expansion_factor,
                     size_t num_colinearity_tests, uint8_t* proof_out, size_t proof_cap);
/* device memory in and out; only enqueues on `stream`: read MZK_FRI_STATUS after synchronizing */
int mzk_fri_prove_gl_dev(int gl_field_id, const void* d_codeword, size_t n, const uint64_t* omega, const uint64_t* offset, size_t expansion_factor,
                         size_t num_colinearity_tests, void* d_proof, size_t proof_cap, void* stream);

/* ---- G2 (BN254 twist over Fq2 = Fq[u]/(u^2+1); bn128.rs:33-49) ------------------------------------------------
 * A G2 point is 16 limbs: x.c0 | x.c1 | y.c0 | y.c1 (4 limbs each, canonical); all-zero = infinity.
 * mzk_msm_g2_bn254: Polynomial::eval_with_powers_on_curve over pk.powers_2 (polynomial.rs:156-165 as called from
 * batch_verify_kzg, kzg.rs:114).  mzk_kzg_setup_g2: powers_2 of setup_kzg_with_full_g2 (kzg.rs:42-55) for a
 * caller-supplied alpha: [alpha^i] g2, i = 0..=max_d ((max_d + 1) x 16 limbs). */
int mzk_msm_g2_bn254(const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t out_xy[16]);
int mzk_msm_g2_bn254_dev(const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_xy, void* stream);
int mzk_kzg_setup_g2(const uint64_t alpha[4], const uint64_t g2_xy[16], size_t max_d, uint64_t* powers2_xy);

/* Device-resident SRS for repeated commits against one PublicKeyKZG.powers_1 (kzg.rs:8-11). */
typedef struct mzk_srs mzk_srs;
int mzk_srs_upload(const uint64_t* powers_xy, size_t n, mzk_srs** out);
void mzk_srs_free(mzk_srs* srs);
int mzk_kzg_commit_srs(const mzk_srs* srs, const uint64_t* coef, size_t n, uint64_t out_xy[8]);
/* Persistence ("an SRS dump for PublicKeyKZG"; the reference only derives serde on its types and
 * never writes a key).  File = 64-byte header | n points exactly as at this ABI (x || y, little-endian u64 limbs,
 * canonical, all-zero = infinity) | optionally the window tables in the library's internal encoding; the header
 * holds an FNV-1a 64 of the point bytes, checked on load (MZK_E_IO).  mzk_srs_save(with_tables != 0) stores the tables
 * if the handle has them; mzk_srs_load(with_tables as in mzk_srs_from_device_ex) reads stored tables of the wanted
 * width and otherwise rebuilds them (which is faster than reading them from disk: see DESIGN.md).
 * mzk_srs_download returns powers_1 (n * 8 limbs) of a handle, e.g. one built by mzk_kzg_setup_g1_dev. */
int mzk_srs_save(const mzk_srs* srs, const char* path, int with_tables);
int mzk_srs_load(const char* path, int with_tables, mzk_srs** out);
int mzk_srs_download(const mzk_srs* srs, uint64_t* powers_xy, size_t cap_points);
size_t mzk_srs_len(const mzk_srs* srs);

/* ---- device-resident variants (inputs already in HBM; `stream` is a hipStream_t) --------------- */
int mzk_ntt_dev(int field_id, const uint64_t* root_host, const void* d_in, void* d_out, size_t n,
                int inverse, void* stream);
/* `batch` transforms of n points each, stored back to back (batch * n elements), all with the same root: what a prover
 * does column by column in a loop (ntt.rs:7-64 per column; fast_stark.rs interpolates and extends every register) as ONE
 * launch per pass, so that small transforms fill the GPU (2^12 points: 27 us for one transform, and about the same for
 * 64 of them).  Results are bit-identical to `batch` single calls.  In place allowed (d_in == d_out). */
int mzk_ntt_batch(int field_id, const uint64_t* root, const uint64_t* in, uint64_t* out, size_t n, size_t batch, int inverse);
int mzk_ntt_batch_dev(int field_id, const uint64_t* root, const void* d_in, void* d_out, size_t n, size_t batch, int inverse,
                      void* stream);
int mzk_coset_lde_dev(int field_id, const void* d_coef, size_t n_coef, const uint64_t* offset_host,
                      const uint64_t* generator_host, void* d_out, size_t order, void* stream);
/* `cols` transforms (ntt / intt, ntt.rs:7-64) of n_points = 2, 4, 8 or 16 points each, stored COLUMN-major: element i of
 * transform c at [i * cols + c], in and out (not in place).  One trip over the data; the step across the ranks of a transform
 * sharded over several GPUs (myzkp_amd/sharded.py), where after the first exchange a rank holds [source rank][its slice]. */
int mzk_ntt_columns_dev(int field_id, const uint64_t* root, const void* d_in, void* d_out, size_t n_points, size_t cols, int inverse,
                        void* stream);
/* Polynomial::scale (polynomial.rs:167-174) with an optional leading constant: out[i] = lead * coef[i] * ratio^i (lead == NULL: 1);
 * in place allowed.  Also the twiddle step between the local transforms of a transform sharded over several GPUs
 * (myzkp_amd/sharded.py: ratio = w^rank) and its n^-1 (ratio = 1). */
int mzk_poly_scale(int field_id, const uint64_t* coef, size_t n, const uint64_t* ratio, const uint64_t* lead, uint64_t* out);
int mzk_poly_scale_dev(int field_id, const void* d_coef, size_t n, const uint64_t* ratio_host, const uint64_t* lead_host, void* d_out,
                       void* stream);
/* fast_coset_evaluate (ntt.rs:254-269) of `batch` polynomials of n_coef coefficients each onto ONE coset -- the low-degree
 * extension of every column of a trace (fast_stark.rs:231,282,329 call it per polynomial) -- in one launch per pass:
 * coefs = batch * n_coef elements back to back, out = batch * order.  Bit-identical to `batch` single calls. */
int mzk_coset_lde_batch(int field_id, const uint64_t* coefs, size_t n_coef, const uint64_t* offset, const uint64_t* generator,
                        uint64_t* out, size_t order, size_t batch);
int mzk_coset_lde_batch_dev(int field_id, const void* d_coefs, size_t n_coef, const uint64_t* offset_host, const uint64_t* generator_host,
                            void* d_out, size_t order, size_t batch, void* stream);
/* d_out_xy: 8 limbs on the device */
int mzk_msm_g1_bn254_dev(const void* d_scalars, const void* d_points_xy, size_t n, void* d_out_xy, void* stream);
/* Multi-GPU sharding (one process per GPU): each rank reduces its shard to one XYZZ partial
 * (16 limbs, internal Montgomery encoding, opaque), the partials are exchanged with an all-gather
 * (RCCL has no elliptic-curve reduction operator), and every rank folds them. */
int mzk_msm_g1_bn254_partial_dev(const void* d_scalars, const void* d_points_xy, size_t n,
                                 void* d_partial16, void* stream);
int mzk_g1_fold_partials_dev(const void* d_partials16, int count, void* d_out_xy, void* stream);
/* ---- the same sharding inside ONE process (contexts of mzk_init_devices; BASELINE configs[3] without Python) ----
 * Context r owns the contiguous slice mzk_shard_range(n, r, world) of scalars and points, reduces it to one XYZZ
 * partial on its own GPU; the W 128-byte records are gathered on context 0 (pinned host buffer: no peer access or
 * collective library needed for 128 bytes per GPU) and folded there.  All W pipelines run concurrently.  Blocking. */
void mzk_shard_range(size_t n, int rank, int world, size_t* lo, size_t* hi);
int mzk_msm_g1_bn254_multi(const uint64_t* scalars, const uint64_t* points_xy, size_t n, uint64_t out_xy[8]);
/* ONE n-point transform (ntt / intt, ntt.rs:7-64; natural order) whose vector is spread over the W contexts -- the four-step
 * layout of SURVEY 8e: W-point transforms across the GPUs (mzk_ntt_columns_dev), the local n/W-point transform with the
 * twiddle fused into it (fast_coset_evaluate with offset root^rank), and all-to-all exchanges between them (peer copies,
 * each destination pulling its chunk of every source).  Layouts of a distributed vector: CONTIGUOUS = part r is
 * x[r n/W, (r+1) n/W); CYCLIC = part r is x[r], x[r + W], ...  contiguous -> cyclic and cyclic -> contiguous cost two
 * exchanges, contiguous -> contiguous three (cyclic -> cyclic: MZK_E_ARG); keep the cyclic layout between a forward and an
 * inverse transform.  W a power of two <= 16 with W^2 <= n.  d_in_parts[r] / d_out_parts[r]: n/W elements on context r's
 * GPU, inputs complete before the call, not overwritten; blocking.  One process per GPU: myzkp_amd/sharded.py runs the
 * same schedule over RCCL's all-to-all. */
enum { MZK_LAYOUT_CONTIGUOUS = 0, MZK_LAYOUT_CYCLIC = 1 };
int mzk_ntt_multi_dev(int field_id, const uint64_t* root, const void* const* d_in_parts, void* const* d_out_parts, size_t n, int inverse,
                      int layout_in, int layout_out);
int mzk_ntt_multi(int field_id, const uint64_t* root, const uint64_t* in, uint64_t* out, size_t n, int inverse);
typedef struct mzk_srs_multi mzk_srs_multi;
/* PublicKeyKZG.powers_1 sharded over the contexts: from host points, or built on the GPUs (setup_kzg, kzg.rs:27-40:
 * context r computes powers [lo_r, hi_r) itself; with_tables as in mzk_srs_from_device_ex). */
int mzk_srs_upload_multi(const uint64_t* powers_xy, size_t n, mzk_srs_multi** out);
int mzk_kzg_setup_srs_multi(const uint64_t alpha[4], const uint64_t g1_xy[8], size_t max_d, int with_tables, mzk_srs_multi** out);
void mzk_srs_multi_free(mzk_srs_multi* h);
int mzk_srs_multi_world(const mzk_srs_multi* h);
size_t mzk_srs_multi_shard_lo(const mzk_srs_multi* h, int rank);   /* rank = world gives n */
/* commit_kzg (kzg.rs:57-59) over the sharded SRS: coefficients in host memory, or d_coef_shards[r] = device pointer
 * on context r's GPU to coefficients [lo_r, min(hi_r, n)), complete before the call. */
int mzk_kzg_commit_srs_multi(const mzk_srs_multi* h, const uint64_t* coef, size_t n, uint64_t out_xy[8]);
int mzk_kzg_commit_srs_multi_dev(const mzk_srs_multi* h, const void* const* d_coef_shards, size_t n, uint64_t out_xy[8]);

/* commit against a device-resident SRS with device-resident coefficients; out_partial != 0 writes the
 * 16-limb XYZZ partial (multi-GPU shard) instead of the 8-limb affine point. */
int mzk_kzg_commit_srs_dev(const mzk_srs* srs, const void* d_coef, size_t n, void* d_out, int out_partial,
                           void* stream);

/* `count` commitments against one SRS -- commit_kzg (kzg.rs:57-59) once per polynomial, as the reference's callers do in
 * a loop -- with results bit-identical to `count` single calls.  coefs: count vectors of n coefficients back to back
 * (count * n * 4 limbs), out_xy: count affine points (count * 8 limbs).  One commit is kept in flight per context of the
 * current GPU (at most four; mzk_init_devices with the same ordinal repeated makes them: own stream and workspace each,
 * the SRS handle shared), so the latency-bound tail of one commit runs under the bucket accumulation of the others:
 * 1.40 instead of 1.64 ms per 2^20-coefficient commit with four contexts.  With a single context the commits simply
 * run one after the other.  The _dev form forks from and joins `stream`; max_in_flight caps the contexts it uses
 * (0 = up to four: more measured slower except for the smallest commitments; an explicit value may go up to eight).  The
 * lanes want hardware queues of their own: with more than four streams alive on the GPU set GPU_MAX_HW_QUEUES=8. */
int mzk_kzg_commit_srs_batch(const mzk_srs* srs, const uint64_t* coefs, size_t n, size_t count, uint64_t* out_xy);
int mzk_kzg_commit_srs_batch_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, void* d_out_xy, int max_in_flight,
                                 void* stream);
/* open_kzg (kzg.rs:61-72) of `count` polynomials of n coefficients each against one SRS, polynomial i at us[4 i .. 4 i + 4)
 * (repeat the point to open all at one place): d_ys = count * 4 limbs, d_ws_xy = count * 8 limbs, both on the device.  Same
 * lanes as the batch commit; every (y_i, w_i) bit-identical to mzk_kzg_open_srs_dev. */
int mzk_kzg_open_srs_batch_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us, void* d_ys, void* d_ws_xy,
                               int max_in_flight, void* stream);
/* the same with coefficients and results in host memory (blocking): ys = count * 4 limbs, ws_xy = count * 8 limbs */
int mzk_kzg_open_srs_batch(const mzk_srs* srs, const uint64_t* coefs, size_t n, size_t count, const uint64_t* us, uint64_t* ys, uint64_t* ws_xy);
/* The reference's actual call pattern -- hundreds of SHORT polynomials against one `pk`: one commit_kzg per row
 * (das/avail.rs:88-98), per chunk (das/eigenda.rs:92-101), per folded polynomial (algebra/gemini.rs:112-114), one open_kzg
 * per cell (das/avail.rs:132).  When the handle holds narrow window tables (8- or 10..13-bit: the default up to 2^14 points)
 * and count > 1, the whole batch runs as ONE bucket problem over (polynomial x bucket) -- digit sort, accumulation, bucket
 * reduction and one tail workgroup PER POLYNOMIAL, the same handful of launches whatever `count` is -- instead of one commit
 * per lane: 256 commitments of 2^10 coefficients take about what six single calls took (0.76 ms; 0.52 - 0.59 ms over the
 * direct tables below).  Arguments and results exactly as the _batch_dev forms, which route here themselves from four
 * polynomials on; handles without narrow tables take the lanes of the _batch forms.  Every point bit-identical to the single
 * call.  Work enqueued on `stream` only: no fork, no extra contexts needed. */
int mzk_kzg_commit_srs_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, void* d_out_xy, void* stream);
/* Optional second table set of a SHORT SRS (at most 2^14 points) for those batches: every multiple a signed window digit can
 * ask for, D[w][i][m] = (m + 1) 2^(c w) P_i -- (254 / c + 1) n 2^(c-1) affine points: 0.85 GiB for 1024 powers at c = 10.  With
 * it a batch needs no buckets at all: one gathered row and one mixed addition per (coefficient, window), a tree per 256
 * coefficients and one fold per polynomial -- two launches, no digit sort, no bucket reduction (the large HBM is what makes
 * this affordable; build once per SRS like the window tables).  window_bits: 8..12, or 0 = the widest that fits max_bytes
 * (0 = a quarter of the free device memory, at most 4 GiB).  Blocking (the tables are complete on return); calling it again with
 * another width replaces them; mzk_srs_drop_direct releases them (mzk_srs_free does too).  Results are bit-identical with and
 * without: the same group element, converted to the same canonical affine point. */
int mzk_srs_build_direct(mzk_srs* srs, int window_bits, size_t max_bytes, void* stream);
void mzk_srs_drop_direct(mzk_srs* srs);
/* What a handle holds: window width of its tables (0 = none: prepared points only), of its direct tables (0 = none), and the
 * device bytes of both together. */
int mzk_srs_window_bits(const mzk_srs* srs);
int mzk_srs_direct_bits(const mzk_srs* srs);
/* Window width (bits of a signed digit) mzk_msm_g1_bn254* uses for n arbitrary points: every scalar is split in two halves of
 * 127 bits (mzk_glv.h), each cut into 126 / bits + 1 windows -- 2 x that many mixed additions per pair (16 bits and 16 additions
 * below 3 x 2^21 pairs, 19 bits and 14 additions from there on).  Sizing information for the callers of Polynomial::
 * eval_with_powers_on_curve (polynomial.rs:156-165), which has no such notion; bench.py prices the accumulate kernel with it. */
int mzk_msm_generic_window_bits(size_t n);
size_t mzk_srs_table_bytes(const mzk_srs* srs);
int mzk_kzg_open_srs_many_dev(const mzk_srs* srs, const void* d_coefs, size_t n, size_t count, const uint64_t* us, void* d_ys, void* d_ws_xy,
                              void* stream);

/* open_kzg / setup_kzg with everything device-resident (end-to-end pipelines: iNTT -> commit -> open).
 * d_y: 4 limbs, d_w_xy: 8 limbs on the device; u / alpha / g1 are host parameters. */
int mzk_kzg_open_srs_dev(const mzk_srs* srs, const void* d_coef, size_t n, const uint64_t u_host[4], void* d_y,
                         void* d_w_xy, void* stream);
int mzk_kzg_setup_g1_dev(const uint64_t alpha_host[4], const uint64_t g1_xy_host[8], size_t max_d, void* d_powers_xy,
                         void* stream);
/* Sharded variants (one process per GPU): rank g builds powers [first, first+count) of the SRS and MSMs its own
 * slice of the coefficient / quotient vectors; mzk_kzg_open_quotient_dev exposes y = f(u) (4 limbs) and the
 * quotient (f - y)/(X - u) (n-1 elements) so that every rank can commit its slice of it. */
int mzk_kzg_setup_g1_range_dev(const uint64_t alpha_host[4], const uint64_t g1_xy_host[8], size_t first, size_t count,
                               void* d_powers_xy, void* stream);
int mzk_kzg_open_quotient_dev(const void* d_coef, size_t n, const uint64_t u_host[4], void* d_y, void* d_q, void* stream);
/* The quotient of open_kzg (kzg.rs:61-72: (f - y) / (X - u)) SHARDED over the ranks: q_{i-1} = b_i with b_i = c_i + u b_{i+1} is a suffix
 * recurrence over the whole coefficient vector, so the rank that holds the slice c[lo, hi) needs one value from the ranks above it,
 * b_hi.  Two local passes around one exchange of 32 bytes per rank:
 *   mzk_kzg_open_slice_value_dev     d_value (4 limbs) = sum_t c[lo + t] u^t, the slice's value at u (its b_lo with carry 0);
 *   (the ranks gather the values; top rank down: b_lo(g) = value(g) + u^(hi - lo) b_hi(g), b_hi(g - 1) = b_lo(g); y = b_lo(0))
 *   mzk_kzg_open_slice_quotient_dev  d_q_slice (len elements) = b[lo + 1 .. hi], given carry_in = b_hi (4 limbs, canonical; 0 for the
 *                                    top rank) -- exactly the quotient coefficients q[lo .. hi) the rank commits against ITS powers
 *                                    (the top rank's last one, q[n - 1] = b_n = 0, contributes nothing).
 * Same field elements as the one-piece recurrence, hence the same witness.  myzkp_amd/sharded.py: sharded_open_quotient. */
int mzk_kzg_open_slice_value_dev(const void* d_coef_slice, size_t len, const uint64_t u_host[4], void* d_value, void* stream);
int mzk_kzg_open_slice_quotient_dev(const void* d_coef_slice, size_t len, const uint64_t u_host[4], const uint64_t carry_in[4], void* d_q_slice,
                                    void* stream);
/* ---- Gemini multilinear commitments and the sum-check prover (algebra/gemini.rs, algebra/sumcheck.rs) ------------------
 * A multilinear g over el variables is given by its n = 2^el coefficients in the order of get_coefs_in_order
 * (sumcheck.rs:97-108): bit i of the index t is the exponent of variable i.  Every value is Fr, standard form, canonical.
 *
 * split_and_fold (gemini.rs:51-100): out = the el + 1 levels f_0 = coef, f_{i+1}[k] = f_i[2k] + rhos[i] f_i[2k+1], back to back
 * (2n - 1 elements; level i starts at 2n - 2n/2^i and holds n/2^i elements; level el is mu).  n not a power of two (0 included):
 * MZK_E_NOT_POW2 (CoefsNotPowerOfTwo); n_rhos != el: MZK_E_LENGTH (PointsLenMismatch); a rho not canonical: MZK_E_RANGE.
 * n <= 2^30.  The _dev form enqueues on `stream`; d_out may equal d_coef (level 0 is then already in place). */
int mzk_gemini_split_fold(const uint64_t* coef, size_t n, const uint64_t* rhos, size_t n_rhos, uint64_t* out);
int mzk_gemini_split_fold_dev(const void* d_coef, size_t n, const uint64_t* rhos, size_t n_rhos, void* d_out, void* stream);
/* commit_gemini (gemini.rs:112-114) of the packed levels of split_fold: out_xy = el + 1 affine points, commit_kzg of each level.
 * n > SRS length: MZK_E_LENGTH (the index panic of eval_with_powers_on_curve). */
int mzk_gemini_commit_srs(const mzk_srs* srs, const uint64_t* levels, size_t n, uint64_t* out_xy);
int mzk_gemini_commit_srs_dev(const mzk_srs* srs, const void* d_levels, size_t n, void* d_out_xy, void* stream);
/* open_gemini (gemini.rs:116-144) of the packed levels at beta:
 *   i < el:  batch_open_kzg(f_i, [beta, -beta, beta^2]) -- ys[12 i .. 12 i + 12) = f_i(beta), f_i(-beta), f_i(beta^2) (-beta =
 *            (0 - beta).sanitize()), ws_xy[8 i ..] = MSM of the quotient by (X - beta)(X + beta)(X - beta^2) (level el - 1 has two
 *            coefficients: empty quotient, w = infinity);
 *   i <= el: deg_xy[8 i ..] = prove_degree_bound(f_i, pk, 2^(el - i)) = MSM(f_i, powers[max_d - 2^(el-i), max_d)), max_d = SRS length - 1.
 * Every value and point is bit-identical to the reference's.  The SRS must hold n + 1 powers (max_d < n: the reference's usize
 * underflow, MZK_E_LENGTH).  beta not canonical: MZK_E_RANGE; beta in {0, 1, -1} (the three points are not distinct and the
 * reference's interpolation divides by zero): MZK_E_ARG.  ys / ws_xy may be NULL when n == 1. */
int mzk_gemini_open_srs(const mzk_srs* srs, const uint64_t* levels, size_t n, const uint64_t beta[4], uint64_t* ys, uint64_t* ws_xy, uint64_t* deg_xy);
int mzk_gemini_open_srs_dev(const mzk_srs* srs, const void* d_levels, size_t n, const uint64_t beta[4], void* d_ys, void* d_ws_xy, void* d_deg_xy,
                            void* stream);
/* sum_over_boolean_hypercube (sumcheck.rs:57-66) of a multilinear g: h = sum_t coef[t] 2^(el - popcount(t)). */
int mzk_sumcheck_sum(const uint64_t* coef, size_t n, uint64_t h[4]);
/* prove_sumcheck (sumcheck.rs:128-167) for a multilinear g.  Round j < el: the device computes g_j(X) = A_j + B_j X of
 * build_gj_from_prefix(g, r_0..r_{j-1}) from the current fold level f_j (m = el - 1 - j):
 *   A_j = sum over even t of f_j[t] 2^(m - popcount(t >> 1)),   B_j = the same over odd t,
 * writes them to gs[8 j .. 8 j + 8) (A_j then B_j), and calls challenge(user, j, g = gs + 8 j, r_out) for r_j (canonical;
 * MZK_E_RANGE otherwise), which it folds into f_{j+1} in the same pass that sums g_{j+1}.  Then challenge(user, el, NULL, r_out)
 * returns beta, and the kept fold levels (they are split_and_fold(coefs, rs)) are committed and opened exactly as
 * mzk_gemini_commit_srs (commits_xy: el + 1 points) and mzk_gemini_open_srs (ys, ws_xy, deg_xy) do.  rs: el values out.
 * Why a callback: the reference's transcript pushes bincode(MPolynomial g_j), a HashMap whose iteration order is random per
 * process, so those bytes cannot be reproduced on any device.  The caller owns the FiatShamirTransformer, builds g_j from
 * (A_j, B_j) (the constant term A_j, X_j's coefficient B_j), pushes it and samples r_j.  The reference samples beta from the
 * unchanged stream right after r_{el-1} (no push in between), so a faithful shim returns beta == r_{el-1}.
 * A non-zero return of the callback stops the prover with MZK_E_CALLBACK.  The callback must not call into this library (the
 * fold levels live in the context's workspace).  el = 0: MZK_E_LENGTH (the assert of build_gj_from_prefix); SRS shorter than
 * n + 1: MZK_E_LENGTH.  Every error returns with nothing left enqueued. */
typedef int (*mzk_sumcheck_challenge_fn)(void* user, int round, const uint64_t g[8], uint64_t r_out[4]);
int mzk_sumcheck_prove_srs(const mzk_srs* srs, const uint64_t* coef, size_t n, mzk_sumcheck_challenge_fn challenge, void* user, uint64_t* gs,
                           uint64_t* rs, uint64_t beta[4], uint64_t* commits_xy, uint64_t* ys, uint64_t* ws_xy, uint64_t* deg_xy);

/* ---- the product sum-check over evaluation tables (examples/sumcheck: SumCheckProverGPU::prove, prover.rs:98-247) -----
 * num_factors = k multilinear factors as tables of n = 2^num_vars canonical Fr values, back to back: factor f at
 * tables[4 (f n + x)].  Index bits are variables in BitCombinationsDictOrder: variable 0 is the most significant bit.  Claimed sum
 * C = sum_x prod_f T_f[x].  Round j (m = n >> j live entries per factor, h = m / 2): s_j(c) = sum_{i<h} prod_f (T_f[i] + c (T_f[i+h] -
 * T_f[i])) for c = 0..=d (d = max_degree, an input of its own: the demo uses d = k), each pushed as its own object
 * vec![bincode(s_j(c))]; r_j = F::sample(SHAKE256(stream)[0..32]) (the last 8 digest bytes big-endian, so r_j < 2^64); every factor
 * folds, T_f[i] <- T_f[i] + r_j (T_f[i+h] - T_f[i]).  Everything runs in one enqueue, the transcript included: no host round trip.
 * Values are canonical representatives in [0, p), which is what the reference's GPU prover pushes (it rebuilds them from bytes with
 * Sign::Plus); its CPU twin can push negative BigInts after sub_ref, which is not reproduced.  bincode(F) is the library's
 * restatement (sign byte 0 / 1, u64 digit count, u32 digits without a leading zero digit: see the Merkle section), not pinned
 * against a Rust vector.  The sums follow the mathematical definition and the *_cpu twins of utils.rs, not the reference's `sum`
 * kernel (several blocks reduce one buffer in place there).
 *
 * header: what the reference pushes before round 0 (prover.rs:108-122: max_degree, num_factors, num_variables, bincode of every
 * factor -- an MPolynomial is a HashMap, so only the caller has those bytes), as header_objects objects already in stream form and
 * concatenated: per object its u64 LE string count, then u64 LE length + bytes per string, i.e. the reference's serialization after
 * the leading object count (the library writes that count).  header_len = 0 with header_objects = 0 is legal.  header is HOST memory in
 * both forms.  Cost: the leading count changes with every push, so no hash state can be kept and the WHOLE stream is hashed again in
 * every round -- the reference's format.  A header costs num_vars times its length in SHAKE256 blocks on one lane pair: a caller at
 * scale should push a digest of its factors, not their bincode.
 *
 * Packed proof (mzk_sumcheck_product_layout; offsets 8-byte aligned; el = num_vars):
 *   MZK_SCP_STATUS          u64: 0
 *   MZK_SCP_SUM             4 u64: C
 *   MZK_SCP_EVALS           el (d+1) x 4 u64: s_j(c), canonical, round-major
 *   MZK_SCP_CHALLENGES      el x 4 u64: r_j
 *   MZK_SCP_FINALS          k x 4 u64: each factor's single remaining value after the last fold, T_f(r_0 .. r_(el-1)) -- what the
 *                           verifier's last check compares the product of against (verifier.rs:68-73)
 *   MZK_SCP_TRANSCRIPT_LEN  u64: bytes of the serialized proof stream
 *   MZK_SCP_TRANSCRIPT      transcript.serialize() after the last round; capacity 8 + header_len + el (d+1) (16 + 41)
 * The input tables are not modified; folded halves live in the context's workspace (k n/2 elements for round 1's tables, k n/4 for
 * round 2's, then ping-pong).  Errors, all before anything is enqueued: null pointer, num_factors or max_degree outside 1..8, a header
 * that does not parse to exactly header_objects objects over header_len bytes (MZK_E_ARG); num_vars == 0 (the reference has no round
 * to run), num_vars > 30, header_len above 2^40 (the layout's sizes must not wrap), proof_cap below the layout's total (MZK_E_LENGTH); a table value that is not canonical (MZK_E_RANGE; host
 * form only -- the _dev form ASSUMES canonical tables, 16-byte aligned, and an 8-byte aligned proof buffer, and only enqueues). */
enum { MZK_SCP_STATUS = 0, MZK_SCP_SUM = 1, MZK_SCP_EVALS = 2, MZK_SCP_CHALLENGES = 3, MZK_SCP_FINALS = 4, MZK_SCP_TRANSCRIPT_LEN = 5,
       MZK_SCP_TRANSCRIPT = 6, MZK_SCP_SECTIONS = 7 };
/* host only, no device work: offsets / sizes have MZK_SCP_SECTIONS entries (each may be NULL) */
int mzk_sumcheck_product_layout(size_t num_vars, size_t num_factors, size_t max_degree, size_t header_len, uint64_t* offsets, uint64_t* sizes,
                                uint64_t* total_bytes);
/* host memory in and out; returns when proof_out is complete */
int mzk_sumcheck_product_prove(const uint64_t* tables, size_t num_vars, size_t num_factors, size_t max_degree, const uint8_t* header,
                               size_t header_len, size_t header_objects, uint8_t* proof_out, size_t proof_cap);
/* device tables and proof; only enqueues on `stream` */
int mzk_sumcheck_product_prove_dev(const void* d_tables, size_t num_vars, size_t num_factors, size_t max_degree, const uint8_t* header,
                                   size_t header_len, size_t header_objects, void* d_proof, size_t proof_cap, void* stream);
/* evals_over_boolean_hypercube (examples/sumcheck/src/utils.rs) for a DENSE multilinear polynomial: coef[t] is the coefficient of
 * prod_{i: bit (el-1-i) of t set} x_i (the tables' MSB-first order), evals[b] = sum over t subset of b of coef[t]: el stages of one
 * modular addition each (the subset-sum butterfly).  n = 2^num_vars values in and out, canonical; num_vars <= 30 (MZK_E_LENGTH),
 * a coefficient that is not canonical MZK_E_RANGE (host form).  d_evals may equal d_coef. */
int mzk_mle_evals_from_coeffs(const uint64_t* coef, size_t num_vars, uint64_t* evals);
int mzk_mle_evals_from_coeffs_dev(const void* d_coef, size_t num_vars, void* d_evals, void* stream);
/* evals_over_boolean_hypercube for SPARSE factors -- the reference prover's first kernel (eval_all_binary_combinations over
 * convert_mpoly_to_kernel_format, prover.rs:124-187) -- and the prover from the reference's own inputs.  n_factors MPolynomials as the
 * flat term table of mzk_mpoly_compose over Fr: factor f = terms [term_offsets[f], term_offsets[f+1]), term t = term_coefs[t] (canonical)
 * and the exponents term_exps[t * num_vars .. (t+1) * num_vars); a HashMap key shorter than num_vars is padded with zeros by the
 * caller, num_vars is the maximum over the factors (prover.rs:99).  Table of factor f at tables[4 (f 2^num_vars + b)]:
 *   evals[b] = sum_t c_t prod_i b_i^(e_t[i]),  b_i = bit (num_vars-1-i) of b (BitCombinationsDictOrder),  0^0 = 1.
 * Only the support of a term matters on {0,1}: with mask_t = OR over {i: e_t[i] > 0} of 1 << (num_vars-1-i), evals[b] is the sum of
 * c_t over the terms with mask_t & ~b == 0 -- a factor that is not multilinear gives the table of its multilinearisation, as the
 * reference's kernel does.  Rows with equal masks add up (duplicate rows and rows such as x0^2, x0^5 included); zero coefficients are
 * allowed; a factor without terms is the zero table.  Coefficients of equal masks are added on the host.
 *   MZK_HYPER_TILE     one launch for all factors: a workgroup builds 2^min(num_vars,10) consecutive entries in LDS from the masks whose
 *                      high bits fit its own and writes them once; nothing of size 2^num_vars is read, uploaded or zero-filled.
 *   MZK_HYPER_SCATTER  hipMemsetAsync of the tables, one kernel writes every merged coefficient to table[mask], then the butterfly of
 *                      mzk_mle_evals_from_coeffs_dev in place per factor: the form for term counts near 2^num_vars.
 *   MZK_HYPER_AUTO     TILE while no factor has more than 256 groups (distinct values of mask >> 10) or more than 4096 distinct
 *                      masks, else SCATTER.
 * mzk_mpoly_hypercube_plan (host only, needs no device) reports what a call with these arguments does: the form that runs, tile_log =
 * min(num_vars, 10), the totals over the factors of terms, distinct masks and groups and the largest per-factor counts, per factor the
 * distinct masks and groups (the first MZK_HYPER_PLAN_FACTORS factors), kernel launches and memsets, the grid of the form's own kernel,
 * the butterfly passes per factor, the bytes uploaded, the workspace bytes of the _dev form and the bytes of the tables.
 * The term table is HOST memory in every form.  The _dev forms return once it has been uploaded (that waits for earlier work on
 * `stream`); the kernels are only enqueued.  d_tables: n_factors * 2^num_vars * 32 bytes, 16-byte aligned, laid out as
 * mzk_sumcheck_product_prove_dev reads them.  mzk_sumcheck_product_prove_terms* builds the tables in the context's workspace
 * (MZK_HYPER_AUTO) and runs mzk_sumcheck_product_prove_dev on them: same packed proof, same header convention.
 * Errors, all before anything is enqueued: null pointer, a form other than the three, misaligned d_tables / d_proof: MZK_E_ARG;
 * num_vars > 30, decreasing term_offsets, 2^28 terms or more, 65536 factors or more: MZK_E_LENGTH; a coefficient that is not
 * canonical: MZK_E_RANGE; prove_terms: every refusal of mzk_sumcheck_product_prove with its code.  num_vars == 0 (evals): one value
 * per factor, the sum of its coefficients.  n_factors == 0 (evals): MZK_OK, nothing written. */
enum { MZK_HYPER_AUTO = 0, MZK_HYPER_TILE = 1, MZK_HYPER_SCATTER = 2 };
enum { MZK_HYPER_PLAN_FACTORS = 8 };
typedef struct mzk_hypercube_plan {
  uint64_t form, tile_log, terms, masks, groups, max_masks, max_groups;
  uint64_t launches, memsets, grid_x, grid_y, mle_passes;
  uint64_t upload_bytes, workspace_bytes, table_bytes;
  uint64_t factor_masks[MZK_HYPER_PLAN_FACTORS], factor_groups[MZK_HYPER_PLAN_FACTORS];
} mzk_hypercube_plan;
int mzk_mpoly_hypercube_plan(const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars, int form,
                             mzk_hypercube_plan* out);
int mzk_mpoly_hypercube_evals(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors, size_t num_vars,
                              int form, uint64_t* tables);
int mzk_mpoly_hypercube_evals_dev(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors,
                                  size_t num_vars, int form, void* d_tables, void* stream);
int mzk_sumcheck_product_prove_terms(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors,
                                     size_t num_vars, size_t max_degree, const uint8_t* header, size_t header_len, size_t header_objects,
                                     uint8_t* proof_out, size_t proof_cap);
int mzk_sumcheck_product_prove_terms_dev(const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_factors,
                                         size_t num_vars, size_t max_degree, const uint8_t* header, size_t header_len, size_t header_objects,
                                         void* d_proof, size_t proof_cap, void* stream);

/* ---- symbolic evaluation of multivariate constraints and the combination of the quotients (FastStark::prove) ----------
 * MPolynomial::evaluate_symbolic (algebra/mpolynomials.rs:125-141; zkstark/fast_stark.rs:246-259 composes every transition
 * constraint with the trace polynomials, zkstark/stark.rs:214 does the same) for n_constraints sparse multivariate polynomials over
 * ONE point of n_vars univariate polynomials:  out_a = sum_t c_t * prod_i point[i]^k[t][i], trimmed of trailing zeros as every
 * `+` and `*` of polynomial.rs:214-228, 302-316 trims (the zero polynomial is empty; pow(0) is one even for the zero polynomial,
 * polynomial.rs:338-348).  Computed in evaluation form -- one batched forward transform of the point, one kernel over (domain point,
 * constraint), one batched inverse transform -- and bit-identical to the reference's term-by-term products (exact arithmetic).
 *   flat term table: constraint a = terms [term_offsets[a], term_offsets[a+1]) (n_constraints + 1 offsets); term t has the coefficient
 *     term_coefs[t] (one element) and the exponents term_exps[t * n_vars .. (t+1) * n_vars).  Duplicate exponent rows are allowed and
 *     add up (a HashMap cannot hold them, a flat table can); zero coefficients are allowed.  The reference indexes point[i] for every
 *     i < k.len(), so one n_vars serves the exponent rows and the point.
 *   point[i] = elements [point_offsets[i], point_offsets[i+1]) of `point`, ascending degree (n_vars + 1 offsets).  Lengths need not be
 *     trimmed: trailing zeros enlarge the bound below and give the same result.
 *   degree bound of constraint a: D_a = max over its terms of sum_i k[t][i] * (len_i - 1); a term with a positive exponent on an empty
 *     point[i] vanishes and does not count.  Transform size N = next_pow2(max_a D_a + 1).
 *   out: row a = out[a * out_stride ..], out_lens[a] coefficients and zeros behind them up to out_stride.
 * mzk_mpoly_compose_plan (host only, needs no device): *n_transform = N, *out_stride_min = max_a (D_a + 1), bounds[a] = D_a + 1
 * (bounds may be NULL; 0 for a constraint without a non-vanishing term; all three 0 when n_constraints == 0).
 * Errors, with nothing left enqueued: a field other than MZK_FIELD_FR / MZK_FIELD_M128, a null pointer, n_vars >
 * MZK_MPOLY_MAX_VARS: MZK_E_ARG; a coefficient of a term or (host form) of a point polynomial not canonical: MZK_E_RANGE;
 * out_stride < out_stride_min, N above the size limit of transforms, a degree bound that overflows 64 bits, an offset array that
 * decreases, 2^28 terms or more: MZK_E_LENGTH.  n_constraints == 0: MZK_OK, nothing written.  A constraint without terms: length 0.  Constants only: N = 1.
 * The _dev form: point and out in HBM (canonical, not checked), complete on `stream` before the call; the term table, the offsets and
 * out_lens are host memory; returns when d_out is complete (as mzk_fast_interpolate_batch_dev does). */
enum { MZK_MPOLY_MAX_VARS = 8 };
int mzk_mpoly_compose_plan(int field_id, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints, size_t n_vars,
                           const size_t* point_offsets, size_t* n_transform, size_t* out_stride_min, size_t* bounds);
int mzk_mpoly_compose(int field_id, const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                      size_t n_vars, const uint64_t* point, const size_t* point_offsets, uint64_t* out, size_t out_stride, size_t* out_lens);
int mzk_mpoly_compose_dev(int field_id, const uint64_t* term_coefs, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                          size_t n_vars, const void* d_point, const size_t* point_offsets, void* d_out, size_t out_stride, size_t* out_lens,
                          void* stream);
/* The weighted combination of the quotients (fast_stark.rs:301-326: sum_i w_i * X^(s_i) * p_i, each quotient once plain and once
 * shifted):  out[j] = sum_i weights[i] * p_i[j - shifts[i]],  p_i = elements [offsets[i], offsets[i+1]) of polys (count + 1 offsets).
 * One launch; out is written (zero-filled) up to out_cap, *out_len = the length after the reference's trim.  Bit-identical to the
 * reference's sequence of Polynomial products and sums.  weights (canonical, MZK_E_RANGE otherwise), shifts, offsets and out_len are
 * host memory in both forms.  out_cap < max_i (len_i + shifts[i]) or decreasing offsets: MZK_E_LENGTH; bad field, null pointer:
 * MZK_E_ARG; (host form) a coefficient not canonical: MZK_E_RANGE.  count == 0: the zero polynomial. */
int mzk_poly_lincomb(int field_id, const uint64_t* polys, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts,
                     uint64_t* out, size_t out_cap, size_t* out_len);
int mzk_poly_lincomb_dev(int field_id, const void* d_polys, const size_t* offsets, size_t count, const uint64_t* weights, const size_t* shifts,
                         void* d_out, size_t out_cap, size_t* out_len, void* stream);
/* Division by a product of linear factors, many rows at once (the boundary quotients of fast_stark.rs:217-224,
 * (tp - interpolant) / zerofier with zerofier = prod_j (X - r_j)).  Row i = polys[i * stride ..], lens[i] coefficients in ascending
 * degree, is divided by prod (X - roots[j]), j in [root_offsets[i], root_offsets[i+1]) (count + 1 offsets, in elements of `roots`):
 * the quotient of Polynomial long division (polynomial.rs:371-405), remainder dropped, trimmed.  Because the interpolant has a lower
 * degree than the zerofier, that quotient is floor(tp / zerofier) whatever the interpolant is, so it is neither an argument nor
 * computed; the division need not be exact.  One synthetic division per root (the engine of the KZG openings, over either field);
 * rows are independent jobs, round r handles every row with more than r roots.
 *   lens need NOT be trimmed: the division runs over the coefficients as given and the trimmed length is found on the device at the
 *     end, so an input with leading zeros gives the reference's result for its trimmed form.
 *   out row i = out[i * stride ..] (the same stride): out_lens[i] coefficients, zeros behind them up to stride.  No roots: the row,
 *     trimmed.  Trimmed length <= number of roots: the zero polynomial, out_lens[i] = 0 (polynomial.rs:372).  Repeated roots are legal.
 *     out must not overlap polys.  polys and out each hold count * stride elements: the last row, too, is a full stride (the host form
 *     copies the block whole; only the lens[i] coefficients of a row are read as values or range-checked).
 * lens, roots (canonical), root_offsets and out_lens are host memory in both forms; the _dev form takes rows in HBM (canonical, not
 * checked), complete on `stream` before the call, and returns when d_out and out_lens are complete.
 * Errors, with nothing left enqueued: bad field, null pointer: MZK_E_ARG; a root or (host form) a coefficient not canonical:
 * MZK_E_RANGE; decreasing root_offsets, lens[i] > stride, more than 2^40 elements in all: MZK_E_LENGTH.  count == 0: MZK_OK. */
int mzk_poly_div_roots(int field_id, const uint64_t* polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots,
                       const size_t* root_offsets, uint64_t* out, size_t* out_lens);
int mzk_poly_div_roots_dev(int field_id, const void* d_polys, size_t stride, const size_t* lens, size_t count, const uint64_t* roots,
                           const size_t* root_offsets, void* d_out, size_t* out_lens, void* stream);
/* ---- FastStark: the sizes of a proof before there is a trace (host only, needs no device) ---------------------------------------
 * Everything initialize_fast_stark_m128 (zkstark/fast_stark.rs:573-616), the degree helpers (:77-111, :150-160) and FRI::num_rounds
 * (fri.rs:86-97) derive from the parameters, the AIR and the boundary -- the lengths, strides and shifts a caller needs to run
 * FastStark::prove stage by stage over the *_dev entry points:
 *   num_randomizers = 4 * num_colinearity_checks; randomized_trace_length = num_cycles + num_randomizers;
 *   omicron_domain_length = 1 << bit_length(randomized_trace_length * transition_constraints_degree); fri_domain_length = that * expansion_factor;
 *   transition_degree_bounds[a] = max over the terms of constraint a of k[0] + (randomized_trace_length - 1) * (k[1] + .. + k[2 m])
 *     (0 without terms); transition_quotient_degree_bounds[a] = that - (num_cycles - 1);
 *   max_degree = (1 << bits(max_a quotient bound)) - 1, bits(0) = 1 as format!("{:b}", 0) has one digit; randomizer_length = max_degree + 1;
 *   boundary_counts[s] = boundary entries of register s (the degree of its zerofier; a cell listed twice counts twice; an entry whose
 *     register is >= num_registers is ignored, as the reference's `if *r == s` ignores it); boundary_quotient_degree_bounds[s] =
 *     randomized_trace_length - 1 - boundary_counts[s];
 *   transition_shifts[a] / boundary_shifts[s] = max_degree - the quotient's degree bound (the X^shift terms of fast_stark.rs:301-326);
 *   n_weights = 1 + 2 * n_constraints + 2 * num_registers; fri_num_rounds, fri_last_length = fri_domain_length >> (rounds - 1);
 *   num_indices = 4 * num_colinearity_checks, the duplicated indices at which every codeword is opened (fast_stark.rs:338-346).
 * The AIR is the flat term table of mzk_mpoly_compose with n_vars = 1 + 2 * num_registers (X, the registers, the registers one cycle on),
 * so num_registers <= MZK_STARK_MAX_REGISTERS = (MZK_MPOLY_MAX_VARS - 1) / 2 = 3 today; the coefficients are not needed.
 * Errors: bad field, null pointer, more registers or constraints than the limits, no constraint at all (the reference unwraps the maximum of an
 * empty list): MZK_E_ARG; expansion_factor not a power of two: MZK_E_NOT_POW2; every usize subtraction that would underflow in Rust
 * (num_cycles - 1, bound - (num_cycles - 1), randomized degree - boundary count, max_degree - boundary bound), an overflowing product,
 * a FRI domain beyond the transform size limit of the field, decreasing term_offsets, fewer than two FRI rounds: MZK_E_LENGTH; more
 * colinearity checks than the last FRI codeword has elements: MZK_E_ARG (as mzk_fri_prove). */
enum { MZK_STARK_MAX_REGISTERS = 3, MZK_STARK_MAX_CONSTRAINTS = 16 };
typedef struct mzk_stark_dims {
  uint64_t num_randomizers, randomized_trace_length, omicron_domain_length, fri_domain_length;
  uint64_t num_registers, n_vars, n_constraints;
  uint64_t max_degree, randomizer_length, n_weights, fri_num_rounds, fri_last_length, num_indices;
  uint64_t transition_degree_bounds[MZK_STARK_MAX_CONSTRAINTS], transition_quotient_degree_bounds[MZK_STARK_MAX_CONSTRAINTS],
      transition_shifts[MZK_STARK_MAX_CONSTRAINTS];
  uint64_t boundary_counts[MZK_STARK_MAX_REGISTERS], boundary_quotient_degree_bounds[MZK_STARK_MAX_REGISTERS], boundary_shifts[MZK_STARK_MAX_REGISTERS];
} mzk_stark_dims;
int mzk_stark_plan(int field_id, size_t expansion_factor, size_t num_colinearity_checks, size_t num_registers, size_t num_cycles,
                   size_t transition_constraints_degree, const uint32_t* term_exps, const size_t* term_offsets, size_t n_constraints,
                   const size_t* boundary_cycles, const size_t* boundary_registers, size_t n_boundary, mzk_stark_dims* out);
/* ---- FastStark::prove in one call (zkstark/fast_stark.rs:177-396) -------------------------------------------------------------------
 * mzk_stark_new is FastStark + preprocess (fast_stark.rs:52-75, :573-616): omega / omicron from mzk_root_of_unity, `generator` the
 * caller's coset offset (M128: 85408008396924667383611388730472331217), the AIR as the flat term table of mzk_mpoly_compose over
 * 1 + 2 * num_registers variables; it builds fast_zerofier over omicron^0 .. omicron^(T-2), its coset codeword and its Merkle tree (kept
 * for the openings), and allocates every buffer a prove needs (MZK_E_NOMEM).  Errors of mzk_stark_plan apply; num_cycles < 2: MZK_E_LENGTH.
 * mzk_stark_transition_zerofier_root: the 32-byte root the verifier is given.  mzk_stark_dims_of: the plan without a boundary (the
 * boundary_* fields are zero; mzk_stark_plan with the boundary gives the dims of a proof).
 *
 * mzk_stark_prove: trace = num_cycles + num_randomizers rows of num_registers elements, row-major as Trace<F> is -- THE CALLER appends
 * the random rows and supplies the max_degree + 1 random coefficients of the randomizer polynomial; the library draws no randomness, so
 * the call is a pure function of its arguments.  boundary entry j = (boundary_cycles[j], boundary_registers[j], boundary_values[j]); the
 * values do not enter the proof (the boundary quotient is floor(tp / zerofier) whatever the interpolant is) and are only range-checked.
 * Stages and pushes in the reference's order: bqc_root[0..m), rdc_root, weights = sample_weights(1 + 2 n_constraints + 2 m,
 * SHAKE256(stream)[0..32]) hashed on the host from the roots; FRI::prove on its own empty stream (mzk_fri_prove); the top-level indices
 * sorted, duplicated (+ expansion_factor, then + fri_domain_length / 2, mod the length, sorted), and all m + 2 trees opened there.
 * The packed proof (mzk_stark_proof_layout; sections 8-byte aligned, path entries MZK_FRI_PATH_STRIDE bytes, zero padded):
 *   MZK_STARK_STATUS      u64: the FRI sampler's status word (non-zero: MZK_E_RANGE, as mzk_fri_prove)
 *   MZK_STARK_FRI         the packed proof of mzk_fri_proof_layout verbatim, except that MZK_FRI_TOP_INDICES holds the SORTED indices
 *                         (fast_stark.rs:338); the revealed layers stay in sampling order
 *   MZK_STARK_INDICES     4 * checks x u64: the duplicated indices, sorted
 *   MZK_STARK_BQC_ROOTS   m x 32 bytes;  MZK_STARK_RDC_ROOT  32 bytes
 *   MZK_STARK_BQC_POINTS  m x 4 * checks elements (register-major);  MZK_STARK_RDC_POINTS, MZK_STARK_TZC_POINTS  4 * checks elements
 *   MZK_STARK_BQC_PATHS, _RDC_PATHS, _TZC_PATHS   per opened index log2(fri_domain_length) entries: the sibling leaf's bytes, then digests
 *   MZK_STARK_PATH_LENS   one u64 per path entry, in the order bqc, rdc, tzc
 * Errors before anything is enqueued: null pointer MZK_E_ARG; n_rows != num_cycles + num_randomizers, proof_cap below the layout's total,
 * the plan's errors for this boundary: MZK_E_LENGTH; (host form) a trace element, randomizer coefficient or boundary value not canonical:
 * MZK_E_RANGE.  Errors of a stage map as the stage maps them (a transition polynomial that is zero or of lower degree than the zerofier:
 * MZK_E_LENGTH, ntt.rs:285).  The _dev form takes trace, randomizer and proof in HBM, complete on `stream` before the call, and returns
 * when the proof is complete.  One prove at a time per handle.  Not kept between calls yet: the inverse of the zerofier's coset
 * transform (mzk_fast_coset_divide_batch_dev recomputes it). */
typedef struct mzk_stark mzk_stark;
enum { MZK_STARK_STATUS = 0, MZK_STARK_FRI = 1, MZK_STARK_INDICES = 2, MZK_STARK_BQC_ROOTS = 3, MZK_STARK_RDC_ROOT = 4, MZK_STARK_BQC_POINTS = 5,
       MZK_STARK_RDC_POINTS = 6, MZK_STARK_TZC_POINTS = 7, MZK_STARK_BQC_PATHS = 8, MZK_STARK_RDC_PATHS = 9, MZK_STARK_TZC_PATHS = 10,
       MZK_STARK_PATH_LENS = 11, MZK_STARK_SECTIONS = 12 };
/* host only: offsets / sizes have MZK_STARK_SECTIONS entries (each may be NULL); dims as mzk_stark_plan filled them (MZK_E_LENGTH otherwise) */
int mzk_stark_proof_layout(const mzk_stark_dims* dims, int field_id, uint64_t* offsets, uint64_t* sizes, uint64_t* total_bytes);
int mzk_stark_new(int field_id, size_t expansion_factor, size_t num_colinearity_checks, size_t num_registers, size_t num_cycles,
                  size_t transition_constraints_degree, const uint64_t* generator, const uint64_t* term_coefs, const uint32_t* term_exps,
                  const size_t* term_offsets, size_t n_constraints, mzk_stark** out);
void mzk_stark_free(mzk_stark* h);
int mzk_stark_transition_zerofier_root(const mzk_stark* h, uint8_t root[32]);
int mzk_stark_dims_of(const mzk_stark* h, mzk_stark_dims* out);
int mzk_stark_prove(mzk_stark* h, const uint64_t* trace, size_t n_rows, const size_t* boundary_cycles, const size_t* boundary_registers,
                    const uint64_t* boundary_values, size_t n_boundary, const uint64_t* randomizer, uint8_t* proof_out, size_t proof_cap);
int mzk_stark_prove_dev(mzk_stark* h, const void* d_trace, size_t n_rows, const size_t* boundary_cycles, const size_t* boundary_registers,
                        const uint64_t* boundary_values, size_t n_boundary, const void* d_randomizer, void* d_proof, size_t proof_cap, void* stream);

/* Build an SRS handle from points already in HBM (affine canonical, n * 8 limbs).  The _ex form chooses
 * whether the window tables are built (worth it from ~30 commits per SRS on at 2^20 points; a one-shot pipeline keeps
 * the plain prepared points and pays the window Horner instead).  Default widths by size: 8 bits up to 1024 points,
 * 10 up to 2^14, 16 below 2^19, 17 below 2^22, 20 from there on (254 / c + 1 tables of n points each: 15 at 17 bits, 13 at 20;
 * measured per size, profiles/r03b_window_sweep.txt, profiles/round4_window_sweep.txt). */
int mzk_srs_from_device(const void* d_powers_xy, size_t n, mzk_srs** out, void* stream);
int mzk_srs_from_device_ex(const void* d_powers_xy, size_t n, int with_tables, mzk_srs** out, void* stream);
/* with_tables: 0 = plain prepared points, 1 = tables with the default window width for n (above), 8..22 = that window width
 * (tuning / tests, and BASELINE configs[2]'s 16 bits at any size).
 * A handle never fails for lack of TABLE memory (commit_kzg(&poly, &pk) does not either): when the wanted tables exceed the
 * budget set by mzk_set_table_budget (bytes per handle; 0 = no limit, the default) or the device refuses the allocation, the
 * handle degrades -- every 2nd table with two bucket sets, every 4th with four (from 2^15 points on; 1/2 and 1/4 of the
 * memory, the same additions, 2 - 4 times the bucket reduction and a few dozen doublings at the end), finally the prepared
 * points alone (the generic layout: 128 bytes per point, ~25 % slower commits) -- and every commitment stays bit-identical.
 * mzk_srs_window_bits / mzk_srs_bucket_sets / mzk_srs_table_bytes tell what a handle got (bucket sets: 1 = full tables,
 * 2 / 4 = degraded, 0 = no tables).  Applies to mzk_srs_upload, mzk_srs_from_device[_ex], mzk_srs_load and the sharded forms. */
int mzk_set_table_budget(size_t bytes);
int mzk_srs_bucket_sets(const mzk_srs* srs);
/* Scratch memory that gives itself back (the reference's Vec buffers are freed when commit_kzg / ntt return, kzg.rs:57-59,
 * ntt.rs:7-48; the library instead keeps per-context workspace buffers so that steady-state calls never allocate).
 *   mzk_set_workspace_budget(bytes): the workspace a context may KEEP (0 = no limit, the default).  A call takes what it needs;
 *     whenever a buffer has to grow while the context holds more than the budget, every buffer the running call has not asked for
 *     is released first (the device is waited for).  Setting a budget below what is held releases the idle buffers at once.
 *   Whatever the budget: an allocation the device refuses -- workspace, SRS tables, prepared points, the buffers of a Merkle tree
 *     handle, the tables of a transform plan -- is tried again after the idle workspace has been released, and a new SRS handle does that BEFORE it degrades its table layout; what is still refused is
 *     MZK_E_NOMEM (never a bare MZK_E_HIP), with nothing enqueued.
 *   mzk_trim_workspace(&released): releases every workspace buffer of every context and the tables of the cached transform plans
 *     (rebuilt on demand); waits for the devices.  released may be NULL.
 *   mzk_workspace_bytes(&bytes): workspace bytes currently held over all contexts. */
int mzk_set_workspace_budget(size_t bytes);
int mzk_trim_workspace(size_t* bytes_released);
int mzk_workspace_bytes(size_t* bytes);
/* Device copy at 16 bytes per lane, grid-stride, on `stream` (d_dst and d_src 16-byte aligned, bytes a multiple of 16): the
 * memory-bound yardstick the benchmark quotes beside the nominal HBM peak (bench.py hbm_copy_GBps_measured). */
int mzk_selftest_copy_dev(const void* d_src, void* d_dst, size_t bytes, void* stream);

/* Host-side parameter arithmetic of the library (roots, inverses, offsets: O(log n) scalar work per call, never on the
 * data path), exposed for checking without a GPU: op 0 = a * b, 1 = a^-1 (0 -> 0), 2 = a^(b[0]), 3 = a * b by the
 * bit-serial reference implementation, 4 = a * R mod p with R = 2^(29 L) the device's Montgomery radix (L = 9 limbs for
 * Fr / Fq, 5 for M128), as the eight 32-bit words of a kernel argument: out receives four uint64 for every field, the upper
 * two zero for M128.  b is not read by ops 1 and 4 and may be null there.  field_id may also be MZK_FIELD_FQ. */
int mzk_host_field_op(int field_id, int op, const uint64_t* a, const uint64_t* b, uint64_t* out);

/* Device self-check: the throughput kernels compute their Montgomery products with hand-scheduled inline-asm blocks
 * (myzkp_amd/csrc/mzk_field_asm.h); this runs both forms (asm and portable C++) over n operand sets per field -- random,
 * all-ones, zero and the widest lazy limbs; for M128 also the signed sparse product of the transform's butterflies on i32 limbs of
 * either sign -- and returns the number of differing results (must be 0).  field_id may also be MZK_FIELD_FQ.
 * These three are self-comparisons (two device forms of one function, a count back); the arithmetic probe below is what compares
 * each form with integers. */
int mzk_selftest_field_asm(int field_id, uint64_t seed, size_t n, uint64_t* mismatches);
/* Device self-check of the ROW-cooperative group operations behind the MSM tails (myzkp_amd/csrc/mzk_row.h: one point
 * operation per wave, field elements spread over DPP rows): n pairs of XYZZ points -- independent points, P + P, P + (-P),
 * infinity on either side -- added and doubled `dbl_reps` times by the row code and by the plain exception-complete formulas
 * (the group law of curve.rs:44-161), compared as group elements; every record is also checked against the storage bound.
 * Returns the number of pairs that differ (must be 0). */
int mzk_selftest_row_ec(uint64_t seed, size_t n, int dbl_reps, uint64_t* mismatches);
/* Device self-check of the wave-cooperative Fq inversion that ends every MSM (myzkp_amd/csrc/mzk_inv_wave.h: the safegcd with
 * the limbs of f, g, d, e spread over the lanes): n values -- 0, 1, 2, 3, 2^29 - 1, 2^28, -1, 1 in Montgomery form, then random
 * ones -- against the single-lane safegcd (which the host build pins on the oracle) and against a * a^-1 == 1.  Returns the
 * number of values that differ (must be 0). */
int mzk_selftest_inv_wave(uint64_t seed, size_t n, uint64_t* mismatches);
/* The arithmetic probe (myzkp_amd/csrc/mzk_probe.h, mzk_probe.hip): where the three self-checks above compare one device form with
 * another and return a count, the probe runs ONE device function per call on operands the host supplies as raw 29-bit limbs and
 * hands the raw result limbs back -- no reduction, packing or comparison on the way -- so that the test-suite can judge every limb
 * against integer arithmetic (tests/arith_model.py, tests/test_gpu_arith_probe.py; the same table runs through the host build of
 * the headers in tests/test_hostcheck_probe.py).  n <= 2^20 cases per call; host pointers; unknown field / op / form, a form the
 * op does not have, null pointers or a larger n: MZK_E_ARG with nothing launched.
 *   mzk_selftest_field_probe: in = n x arity x L limbs (L = 9 for Fr / Fq, 5 for M128; arity 1 .. 4, operands in the order of the
 *     function's parameters), out = n x L limbs (the zero tests: limb 0 = 0 / 1).  MZK_PROBE_SHOUP_MUL takes (x, w, wq) and reads
 *     w, wq from the first case of each wave of 64 (scalar registers, as the transform holds them).  form: MZK_PROBE_FORM_CPP
 *     everywhere; _ASM for MUL, SQR, MUL_ADD2, SHOUP_MUL (Fr), SMUL (M128); _WAVE for INV over Fq (invw::inv, one case per wave).
 *   mzk_selftest_g1_probe: a, b = XYZZ operands as raw slots (4 x 9 limbs, coordinate-major, Montgomery form, all-zero = infinity)
 *     or affine operands (2 x 9 limbs, Montgomery form, canonical): MADD_SIGNED(a slot, b affine, neg[i]), MADD(a slot, b affine),
 *     ADD(a slot, b slot), DBL(a slot), DBL_AFFINE(a affine), TO_AFFINE(a slot); out = one slot per case holding the limbs the
 *     function returned (infinity all-zero; TO_AFFINE: 16 plain ABI words x || y, then zeros).  form: _CPP / _ASM (the product
 *     routines of the single-lane group law), _QUAD (xyzz_add_quad / xyzz_dbl_quad, one case per DPP quad), _ROW (rowop::add /
 *     rowop::dbl, one case per wave through the packed records of rowop::load / rowop::store), _WAVE (TO_AFFINE: wave_store_affine).
 *     b may be NULL where the op takes no second operand, neg where it takes no sign.
 *   mzk_selftest_g2_probe: ONE function of myzkp_amd/csrc/mzk_g2.h per call (tests/g2_model.py, tests/test_gpu_g2_probe.py; the host
 *     build runs the same tables in tests/test_hostcheck_g2_probe.py).  An Fq2 value is 2 x 9 limbs (c0 then c1, Montgomery form), an
 *     XYZZ slot over Fq2 4 x 2 x 9 limbs (X, Y, ZZ, ZZZ; all-zero = infinity), an affine operand 2 x 2 x 9 limbs (x, y; canonical).
 *     F2_ADD / F2_SUB / F2_MUL(a, b), F2_DBL / F2_SQR / F2_INV / F2_IS_ZERO(a): out = one Fq2 per case (IS_ZERO: limb 0 = 0 / 1).
 *     MADD(a slot, b affine), ADD(a slot, b slot), DBL(a slot), DBL_AFFINE(a affine), TO_AFFINE(a slot), SCALAR_MUL(a affine, k = 8
 *     canonical scalar words), STORE_LOAD(a slot: x2_store then x2_load): out = one slot per case holding the limbs the function
 *     returned (TO_AFFINE: the 32 plain wire words x.c0 | x.c1 | y.c0 | y.c1, then zeros).  G2 has the portable form only, so there
 *     is no form argument.  b and k may be NULL where the op does not take them; an unknown op, a null pointer the op needs or
 *     n > 2^20: MZK_E_ARG with nothing launched; n = 0 is MZK_OK. */
enum { MZK_PROBE_MUL = 0, MZK_PROBE_SQR = 1, MZK_PROBE_MUL_ADD2 = 2, MZK_PROBE_SHOUP_MUL = 3, MZK_PROBE_SMUL = 4, MZK_PROBE_SMUL_C1 = 5,
       MZK_PROBE_SADD = 6, MZK_PROBE_SSUB = 7, MZK_PROBE_SCARRY = 8, MZK_PROBE_SBIAS = 9, MZK_PROBE_SREDUCE = 10,
       MZK_PROBE_ADD = 11, MZK_PROBE_SUB4 = 12, MZK_PROBE_SUB8 = 13, MZK_PROBE_NEG_LAZY4 = 14, MZK_PROBE_NEG_LAZY8 = 15,
       MZK_PROBE_DBL = 16, MZK_PROBE_CARRY = 17, MZK_PROBE_WEAK_REDUCE = 18, MZK_PROBE_REDUCE = 19, MZK_PROBE_COND_SUB_P = 20,
       MZK_PROBE_NEG_CANON = 21, MZK_PROBE_IS_ZERO_MOD6 = 22, MZK_PROBE_IS_ZERO_MOD10 = 23, MZK_PROBE_IS_ZERO_MOD12 = 24,
       MZK_PROBE_INV = 25 };
enum { MZK_PROBE_FORM_CPP = 0, MZK_PROBE_FORM_ASM = 1, MZK_PROBE_FORM_QUAD = 2, MZK_PROBE_FORM_ROW = 3, MZK_PROBE_FORM_WAVE = 4 };
enum { MZK_PROBE_G1_MADD_SIGNED = 0, MZK_PROBE_G1_MADD = 1, MZK_PROBE_G1_ADD = 2, MZK_PROBE_G1_DBL = 3, MZK_PROBE_G1_DBL_AFFINE = 4,
       MZK_PROBE_G1_TO_AFFINE = 5 };
enum { MZK_PROBE_G2_F2_ADD = 0, MZK_PROBE_G2_F2_SUB = 1, MZK_PROBE_G2_F2_DBL = 2, MZK_PROBE_G2_F2_MUL = 3, MZK_PROBE_G2_F2_SQR = 4,
       MZK_PROBE_G2_F2_INV = 5, MZK_PROBE_G2_F2_IS_ZERO = 6, MZK_PROBE_G2_MADD = 7, MZK_PROBE_G2_ADD = 8, MZK_PROBE_G2_DBL = 9,
       MZK_PROBE_G2_DBL_AFFINE = 10, MZK_PROBE_G2_TO_AFFINE = 11, MZK_PROBE_G2_SCALAR_MUL = 12, MZK_PROBE_G2_STORE_LOAD = 13 };
int mzk_selftest_field_probe(int field_id, int op, int form, size_t n, const uint32_t* in, uint32_t* out);
int mzk_selftest_g1_probe(int op, int form, size_t n, const uint32_t* a, const uint32_t* b, const uint8_t* neg, uint32_t* out);
int mzk_selftest_g2_probe(int op, size_t n, const uint32_t* a, const uint32_t* b, const uint32_t* k, uint32_t* out);

/* ---- Reed-Solomon over GF(2^8) (algebra/reedsolomon.rs) ------------------------------------------------------------ */
/* The codec every data-availability system of das/ starts with (das/avail.rs, das/eigenda.rs, das/celestia.rs), batched: every chunk,
 * row and column is an independent codeword.  The field is ExtendedFieldElement<Mod2, Ip0x11D> (reedsolomon.rs:352-371): a byte is a
 * polynomial over GF(2), bit i the coefficient of x^i, modulo x^8 + x^4 + x^3 + x^2 + 1; the generator of every code is x = 0x02
 * (setup_rs1d / setup_rs2d, :396-416).  A symbol is one byte on both sides of the boundary; no call takes a field id.
 *   (n, k): 1 <= k <= n <= 255, d = n - k parity symbols, t = d / 2 correctable errors; d = 0 makes encode and decode copies.  Anything
 *   else is MZK_E_ARG: 2 has order 255, so from n = 256 on the reference's evaluation points repeat and its own decoder stops
 *   correcting.  batch: 1 .. 2^31 codewords (MZK_E_ARG outside).
 *   Messages are exactly k bytes.  The reference accepts a shorter message (reedsolomon.rs:54-78): that is the same call with the message
 *   zero-padded at the top.  Codewords are exactly n bytes: (m(x) x^d mod g) in positions 0 .. d-1, the message in d .. n-1.  The
 *   reference's vector is this one with its trailing zero symbols trimmed (its Polynomial subtraction trims, :76-77): shorter than n
 *   whenever the top message bytes are zero, empty for the zero message.
 *   status, one byte per codeword: 0 = all syndromes zero, the word is returned as it came; 1 .. = the number of symbols corrected
 *   (the degree of the error locator, all of whose roots were found); 255 = the reference's None (root count != degree, or a zero
 *   derivative in Forney's formula, :225-245) -- corrected / messages then hold the received word unchanged.  Beyond t errors the
 *   reference either gives up or miscorrects to another codeword; the status says which, the call itself returns MZK_OK.
 * Host forms take host pointers and return MZK_E_NOGPU without a device; the _dev forms take device pointers and only enqueue. */
/* generator_polynomial (:34-37) = prod_{i<d} (x - 2^i), n - k + 1 coefficients from the constant term up.  Host arithmetic: works without a GPU. */
int mzk_rs_generator_poly(size_t n, size_t k, uint8_t* g);
/* encode (:54-78) of `batch` messages, k bytes each, into `batch` codewords, n bytes each.
 * d_columns_fr (may be NULL): the codewords once more as BN254 Fr elements (4 x uint64_t, value = the byte), symbol-major: element
 * i * batch + b is symbol i of codeword b -- n polynomials of `batch` coefficients, the layout
 * mzk_kzg_commit_srs_many_dev(srs, d_columns_fr, batch, n, ...) takes, so that Avail's commit (das/avail.rs:87-98) follows its encode
 * with no host step in between.
 * _view_dev: both sides as views -- symbol s of item b at base + b * stride + s * symbol_stride (bytes) -- so that columns of a
 * row-major matrix are encoded where they lie.  In place is allowed in exactly one form: the message already sits in positions
 * d .. n-1 of its codeword (d_messages = d_codewords + d * cw_symbol_stride, equal strides); any other overlap is undefined. */
int mzk_rs_encode(size_t n, size_t k, const uint8_t* messages, size_t batch, uint8_t* codewords);
int mzk_rs_encode_dev(size_t n, size_t k, const void* d_messages, size_t batch, void* d_codewords, void* d_columns_fr, void* stream);
int mzk_rs_encode_view_dev(size_t n, size_t k, const void* d_messages, size_t msg_symbol_stride, size_t msg_stride, size_t batch, void* d_codewords,
                           size_t cw_symbol_stride, size_t cw_stride, void* d_columns_fr, void* stream);
/* compute_syndromes (:90-102): S_j = sum_i r_i 2^(i j), j < d; d bytes per word (nothing is written when d = 0). */
int mzk_rs_syndromes(size_t n, size_t k, const uint8_t* words, size_t batch, uint8_t* syndromes);
int mzk_rs_syndromes_dev(size_t n, size_t k, const void* d_words, size_t batch, void* d_syndromes, void* stream);
/* correct_errors (:206-253) and decode (:80-86): corrected = n bytes per word, messages = corrected[d ..] = k bytes per word; either
 * may be NULL.  status: see above. */
int mzk_rs_decode(size_t n, size_t k, const uint8_t* received, size_t batch, uint8_t* corrected, uint8_t* messages, uint8_t* status);
int mzk_rs_decode_dev(size_t n, size_t k, const void* d_received, size_t batch, void* d_corrected, void* d_messages, void* d_status, void* stream);
/* ReedSolomon2D (:256-350): size = ceil(sqrt(message_len)), rows coded (row_n, size), columns (col_n, size); message_len >= 1 and
 * size <= min(col_n, row_n) (MZK_E_ARG otherwise, in the words of the 1D code).  code = col_n rows of row_n bytes, row-major, the data at
 * [col_n - size + i][row_n - size + j].  The reference's transposes mis-handle rows that its encode trimmed (they truncate, or panic
 * when the first row is the shortest); these calls work on fixed-length rows: the reference's result wherever it does neither.
 * decode: every column, then every one of the `size` rows; *ok = 0 is the reference's None (a column or a row with status 255; data is
 * then not meaningful).  col_status (row_n bytes) / row_status (size bytes) may be NULL; the row statuses mean nothing when a
 * column failed (the reference returns before it decodes a row).  _dev: d_ok is a device int. */
int mzk_rs2d_encode(size_t col_n, size_t row_n, const uint8_t* data, size_t message_len, uint8_t* code);
int mzk_rs2d_encode_dev(size_t col_n, size_t row_n, const void* d_data, size_t message_len, void* d_code, void* stream);
int mzk_rs2d_decode(size_t col_n, size_t row_n, const uint8_t* code, size_t message_len, uint8_t* data, int* ok, uint8_t* col_status, uint8_t* row_status);
int mzk_rs2d_decode_dev(size_t col_n, size_t row_n, const void* d_code, size_t message_len, void* d_data, int* d_ok, void* d_col_status, void* d_row_status,
                        void* stream);

/* ---- Celestia's commitment (das/celestia.rs:73-169 over algebra/merkle.rs) ---------------------------------------------- */
/* Row roots, column roots and the data root of a batch of byte squares in one call, and a handle that keeps every node and serves
 * sample proofs as gathers.  A square is rows x cols symbols; symbol (r, c) of square q is at
 *     base + q * square_stride + r * row_stride + c
 * which is what mzk_rs2d_encode_dev writes, with rows = col_n, cols = row_n (dense: row_stride = cols, square_stride = rows * cols).
 *   Trees: a leaf is one symbol, one byte, not hashed itself; Merkle::commit splits a slice at mid = len / 2 and hashes
 *   SHA3-256(left || right); a one-leaf slice commits to the leaf.  row_roots[r] = commit of row r (cols leaves), col_roots[c] =
 *   commit of column c (rows leaves), data_root = commit of the rows + cols roots, rows first, as 32-byte leaves.
 *   Admitted: 2 <= rows, cols <= 255; row_stride >= cols; square_stride >= (rows - 1) * row_stride + cols when squares > 1;
 *   1 <= squares, squares * (rows + cols) <= 2^31.  Anything else: MZK_E_ARG, the text names the parameter, nothing is enqueued.
 *   Outputs per square: rows x 32, cols x 32 and 32 bytes, dense, square-major.
 * Host forms take host pointers and dense squares and return MZK_E_NOGPU without a device; the _dev forms take device pointers and
 * only enqueue. */
enum { MZK_DAS_PATH_MAX = 8 };      /* floor(log2 255) + 1: the most entries of a path */
/* What the calls below launch for (rows, cols, squares): host only, works without a GPU.  plan: MZK_DAS_PLAN_WORDS values, indexed by
 * the constants below (the form of mzk_stark_proof_layout's sections).  *_ITEMS / *_DEPTH: M = 2^D bottom subtrees of one or two leaves
 * and D = floor(log2 n) levels above them, of a row tree (cols leaves), a column tree (rows leaves) and the data-root tree (rows + cols
 * leaves).  The tree launch takes ROW_WGS + COL_WGS workgroups' worth of work (*_TREES_PER_WG trees each) with TREE_GRID workgroups in
 * TREE_ITERS rounds; the data-root launch one workgroup per square.  NODE_BYTES: what a handle keeps in device memory (every item
 * and node of every row and column tree, the roots, a copy of the symbols). */
enum { MZK_DAS_PLAN_ROWS = 0, MZK_DAS_PLAN_COLS = 1, MZK_DAS_PLAN_SQUARES = 2,
       MZK_DAS_PLAN_ROW_ITEMS = 3, MZK_DAS_PLAN_ROW_DEPTH = 4, MZK_DAS_PLAN_COL_ITEMS = 5, MZK_DAS_PLAN_COL_DEPTH = 6,
       MZK_DAS_PLAN_ROOT_ITEMS = 7, MZK_DAS_PLAN_ROOT_DEPTH = 8,
       MZK_DAS_PLAN_ROW_TREES_PER_WG = 9, MZK_DAS_PLAN_COL_TREES_PER_WG = 10, MZK_DAS_PLAN_ROW_WGS = 11, MZK_DAS_PLAN_COL_WGS = 12,
       MZK_DAS_PLAN_TREE_GRID = 13, MZK_DAS_PLAN_TREE_ITERS = 14, MZK_DAS_PLAN_TREE_BLOCK = 15, MZK_DAS_PLAN_TREE_LDS = 16,
       MZK_DAS_PLAN_ROOT_GRID = 17, MZK_DAS_PLAN_ROOT_ITERS = 18, MZK_DAS_PLAN_ROOT_BLOCK = 19, MZK_DAS_PLAN_ROOT_LDS = 20,
       MZK_DAS_PLAN_NODE_BYTES = 21, MZK_DAS_PLAN_PATH_MAX = 22, MZK_DAS_PLAN_WORDS = 23 };
int mzk_das_plan_get(size_t rows, size_t cols, size_t squares, uint64_t* plan);
/* Celestia::commit (:73-113) of `squares` squares: two launches, no host step.  d_row_roots / d_col_roots may be NULL when only the
 * data roots are wanted (they are then scratch of the workspace).  The three outputs must be 16-byte aligned (MZK_E_ARG otherwise); the
 * input needs no alignment. */
int mzk_das_commit_dev(const void* d_code, size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares, void* d_row_roots,
                       void* d_col_roots, void* d_data_roots, void* stream);
int mzk_das_commit(const uint8_t* code, size_t rows, size_t cols, size_t squares, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots);
/* The same hashing with every item and node level of every row and column tree kept in device memory, plus a copy of the symbols.
 * The handle belongs to the context that built it, as a mzk_merkle does: later calls enter that context and run behind the build. */
typedef struct mzk_das_grid mzk_das_grid;
int mzk_das_grid_build_dev(const void* d_code, size_t rows, size_t cols, size_t row_stride, size_t square_stride, size_t squares, mzk_das_grid** out,
                           void* stream);
int mzk_das_grid_build(const uint8_t* code, size_t rows, size_t cols, size_t squares, mzk_das_grid** out);
/* host outputs, any of them may be NULL */
int mzk_das_grid_roots(const mzk_das_grid* grid, uint8_t* row_roots, uint8_t* col_roots, uint8_t* data_roots);
/* Merkle::open as Celestia::verify calls it (:124-135), `count` samples in one gather launch.  positions: count x 4 uint64_t
 * (square, row, col, is_row), SamplePosition plus the square: is_row = 1 opens index col of row `row`'s tree, is_row = 0 index row of
 * column `col`'s tree.  For sample s: entry k at paths[(s * 8 + k) * 32 ..], zero-filled behind its length; its length (1 or 32) in
 * entry_lens[s * 8 + k] (0 from depths[s] on); depths[s] = the number of entries; leaves[s] = the opened symbol.  Entry 0 is the
 * sibling leaf, higher entries the sibling subtree's commitment: 1 byte where that is a one-leaf item, else 32.
 * depths[s] = 0 is the reference's non-termination (a leaf that is the one-leaf half of a three-leaf slice): nothing else of that
 * sample is meaningful and the call still returns MZK_OK, as the status byte of mzk_rs_decode.
 * A position out of range (or is_row > 1): MZK_E_ARG for the whole call in the host form; the _dev form (device pointers, only
 * enqueues on `stream` behind the build; d_paths 16-byte aligned, d_positions 8-byte aligned) writes depths[s] = 255 and nothing else of
 * that sample. */
int mzk_das_grid_open(const mzk_das_grid* grid, const uint64_t* positions, size_t count, uint8_t* paths, uint8_t* entry_lens, uint8_t* depths,
                      uint8_t* leaves);
int mzk_das_grid_open_dev(const mzk_das_grid* grid, const void* d_positions, size_t count, void* d_paths, void* d_entry_lens, void* d_depths,
                          void* d_leaves, void* stream);
void mzk_das_grid_free(mzk_das_grid* grid);

/* ---- Rescue-Prime (zkstark/rescueprime.rs) -------------------------------------------------------------------------------- */
/* Batched hashes, hash chains and their traces, one chain per lane: the witness of mzk_stark_prove_dev made where it is read.
 *   A hash (rescueprime.rs:401-452) absorbs one element, state = [x, 0, .., 0] of m elements, runs n_rounds rounds of two half-rounds
 *   -- every element raised to alpha (first half) or alphainv (second half), then state = mds * state + round constants, the constant
 *   of (round r, half h, element i) at index 2 r m + h m + i -- and returns state[0].  A chain of `links` hashes feeds the output of
 *   link l into link l + 1.  The trace of a hash is the state before round 0 and after every round: n_rounds + 1 rows of m elements.
 *   Admitted: rescue_field_id MZK_FIELD_M128 or MZK_FIELD_FR (any other id, MZK_FIELD_FQ and the Goldilocks ids included, is refused in this
 *   section's own words: "rescue: field id N is neither MZK_FIELD_M128 nor MZK_FIELD_FR"); 1 <= m <= MZK_RESCUE_MAX_M; 1 <= n_rounds <= MZK_RESCUE_MAX_ROUNDS; alpha any
 *   uint64_t; alphainv any exponent below 2^256, four little-endian uint64_t for both fields.  x^0 = 1 for every x, 0 included (utils.rs
 *   pow).  That the two exponents are inverse to each other is not checked, as the reference does not check it.
 *   Elements are canonical little-endian limbs, 2 uint64_t (M128) or 4 (Fr).  mds is m x m, row-major; round_constants 2 n_rounds m.
 *   Layout: outputs[b * links + l] = the output of link l of chain b.  The trace of (chain b, link l) starts at element
 *   (b * links + l) * trace_stride of `traces`, row r at r * m behind that; trace_stride >= (n_rounds + 1) m, in elements.  Elements of a
 *   slot past the last row are NOT written: a caller that keeps the random rows of mzk_stark_prove_dev there passes
 *   d_traces + slot * trace_stride (elements) on as d_trace as it stands.  The boundary values do not enter a proof, so a prove can be
 *   enqueued behind mzk_rescue_trace_dev before the host knows the output.
 *   Errors, all before anything is enqueued: MZK_E_ARG (null pointer, bad field, m or n_rounds outside the limits, a _dev pointer that
 *   is not 16-byte aligned), MZK_E_RANGE (a constant, or in the host forms an input, that is not canonical), MZK_E_LENGTH (trace_stride
 *   too small, batch beyond 2^40, an overflowing size product), MZK_E_NOMEM.  batch = 0 or links = 0: MZK_OK, nothing done.
 * Host forms take host pointers and return MZK_E_NOGPU without a device.  The _dev forms take device pointers holding canonical inputs
 * (not checked) and only enqueue on `stream`.  A handle belongs to the context that made it, as a mzk_stark and a mzk_das_grid do: later
 * calls enter that context; its constants are complete when mzk_rescue_new returns. */
enum { MZK_RESCUE_MAX_M = 4, MZK_RESCUE_MAX_ROUNDS = 64 };
typedef struct mzk_rescue mzk_rescue;
/* What the calls below run for these parameters and `batch` chains (mzk_rescue_plan.h): host only, works without a GPU.  plan:
 * MZK_RESCUE_PLAN_WORDS values indexed by the constants below.  For each exponent, from *_WINDOW on: the window width kept (3, 2 or 1;
 * 0 for exponent 0), the slots read (x, x^3, x^5, x^7: at most 4), the steps of the program, its squarings, its products by a slot, the
 * products that build the table, their sum, and what the binary method would take.  PRODUCTS_PER_HASH = n_rounds (m (both sums) + 2 m^2)
 * + 2.  ROWS = n_rounds + 1, MIN_STRIDE = ROWS m.  A launch takes WGS = ceil(batch / BLOCK) workgroups' worth of chains with GRID <=
 * GRID_CAP workgroups in ITERS rounds.  CONST_BYTES: what a handle keeps in device memory. */
enum { MZK_RESCUE_PLAN_FIELD = 0, MZK_RESCUE_PLAN_M = 1, MZK_RESCUE_PLAN_ROUNDS = 2, MZK_RESCUE_PLAN_BATCH = 3,
       MZK_RESCUE_PLAN_ALPHA_WINDOW = 4, MZK_RESCUE_PLAN_ALPHA_SLOTS = 5, MZK_RESCUE_PLAN_ALPHA_STEPS = 6, MZK_RESCUE_PLAN_ALPHA_SQUARINGS = 7,
       MZK_RESCUE_PLAN_ALPHA_MULTIPLIES = 8, MZK_RESCUE_PLAN_ALPHA_TABLE = 9, MZK_RESCUE_PLAN_ALPHA_PRODUCTS = 10, MZK_RESCUE_PLAN_ALPHA_BINARY = 11,
       MZK_RESCUE_PLAN_ALPHAINV_WINDOW = 12, MZK_RESCUE_PLAN_ALPHAINV_SLOTS = 13, MZK_RESCUE_PLAN_ALPHAINV_STEPS = 14, MZK_RESCUE_PLAN_ALPHAINV_SQUARINGS = 15,
       MZK_RESCUE_PLAN_ALPHAINV_MULTIPLIES = 16, MZK_RESCUE_PLAN_ALPHAINV_TABLE = 17, MZK_RESCUE_PLAN_ALPHAINV_PRODUCTS = 18, MZK_RESCUE_PLAN_ALPHAINV_BINARY = 19,
       MZK_RESCUE_PLAN_PRODUCTS_PER_HASH = 20, MZK_RESCUE_PLAN_ROWS = 21, MZK_RESCUE_PLAN_MIN_STRIDE = 22,
       MZK_RESCUE_PLAN_BLOCK = 23, MZK_RESCUE_PLAN_WGS = 24, MZK_RESCUE_PLAN_GRID = 25, MZK_RESCUE_PLAN_ITERS = 26, MZK_RESCUE_PLAN_GRID_CAP = 27,
       MZK_RESCUE_PLAN_CONST_BYTES = 28, MZK_RESCUE_PLAN_WORDS = 29 };
int mzk_rescue_plan_get(int rescue_field_id, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t alphainv[4], size_t batch, uint64_t* plan);
/* The parameters as a handle: both exponents as programs, the MDS matrix and the round constants in Montgomery form, in device memory. */
int mzk_rescue_new(int rescue_field_id, size_t m, size_t n_rounds, uint64_t alpha, const uint64_t alphainv[4], const uint64_t* mds,
                   const uint64_t* round_constants, mzk_rescue** out);
void mzk_rescue_free(mzk_rescue* h);
/* `batch` chains of `links` hashes: batch inputs, batch * links outputs. */
int mzk_rescue_hash(mzk_rescue* h, const uint64_t* inputs, size_t batch, size_t links, uint64_t* outputs);
int mzk_rescue_hash_dev(mzk_rescue* h, const void* d_inputs, size_t batch, size_t links, void* d_outputs, void* stream);
/* The same with the trace of every hash; outputs / d_outputs may be NULL. */
int mzk_rescue_trace(mzk_rescue* h, const uint64_t* inputs, size_t batch, size_t links, uint64_t* traces, size_t trace_stride, uint64_t* outputs);
int mzk_rescue_trace_dev(mzk_rescue* h, const void* d_inputs, size_t batch, size_t links, void* d_traces, size_t trace_stride, void* d_outputs,
                         void* stream);

/* Deterministic synthetic inputs (bench + tests): bit-identical to the oracle's orc_synth_*. */
int mzk_synth_field_dev(int field_id, uint64_t seed, size_t n, void* d_out, void* stream);
int mzk_synth_g1_points_dev(uint64_t seed, size_t n, void* d_out_xy, void* stream);

/* ---- per-phase device timing (HIP events recorded on the launch stream around each kernel group) ---- */
enum { MZK_PH_MSM_PREPARE = 0, MZK_PH_MSM_SORT = 1, MZK_PH_MSM_ACCUMULATE = 2, MZK_PH_MSM_REDUCE = 3,
       MZK_PH_MSM_COMBINE = 4, MZK_PH_NTT_PASS0 = 5, MZK_PH_NTT_PASS1 = 6, MZK_PH_NTT_PASS2 = 7,
       MZK_PH_NTT_PASS3 = 8, MZK_PH_NTT_PRESCALE = 9, MZK_PH_MERKLE = 10,
       MZK_PH_MSM_SEG_COMBINE = 11,   /* k_seg_combine (+ heavy): sums a bucket's segment partials; MSM_ACCUMULATE is k_seg_accumulate alone */
       MZK_PH_NTT_TOTAL = 12,         /* one pair around all passes of a transform */
       MZK_PH_SCP_ROUND0 = 13,        /* mzk_sumcheck_product_prove: round 0's kernel (no fold: one read of the tables) */
       MZK_PH_SCP_ROUND = 14,         /* ... the fold-and-sum kernels of the later grid rounds */
       MZK_PH_SCP_ROUND_END = 15,     /* ... the one-workgroup transcript steps between them */
       MZK_PH_SCP_TAIL = 16,          /* ... every round from 2^7 entries per factor down, one launch */
       MZK_PH_HYPERCUBE = 17,         /* mzk_mpoly_hypercube_evals: the device work behind the upload (tile kernel, or memset, scatter and butterfly) */
       MZK_PH_COUNT = 18 };
int mzk_prof_enable(int on);
/* bit p set = phase p gets its event pair while profiling is on (default: all).  An event pair costs a few
 * microseconds of stream time, so a timed region instruments only the kernel it prices. */
int mzk_prof_select(uint32_t phase_mask);
int mzk_prof_reset(void);
/* Synchronises the device, folds all pending event pairs, returns accumulated ms and launch count. */
int mzk_prof_read(int phase, double* total_ms, uint64_t* launches);
const char* mzk_prof_name(int phase);

#ifdef __cplusplus
}
#endif
#endif /* MZK_H */
