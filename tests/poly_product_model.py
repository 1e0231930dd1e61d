"""Polynomial::fft_multiply (polynomial.rs:242-276) and ntt::fast_multiply (ntt.rs:66-116) on Python integers: the exact product by
the schoolbook rule or by Kronecker substitution (one big-integer product), and around it the reference's length bookkeeping --
next_power_of_two, resize, truncate, trim; the zero-operand and degree < 8 exits, the halving of the order, the untrimmed cyclic
result.  No transform, no root: what the kernels must reproduce, computed another way.  Owned by tests/test_oracle_products.py,
which checks the two product rules against each other and the CPU oracle against the model; tests/test_gpu_poly_products.py then
holds the library to it.  Polynomials are lists of ints in [0, p), lowest coefficient first; arrays are (n, limbs) uint64."""
import numpy as np
import orc

E_NOT_POW2, E_LENGTH = -2, -5          # MZK_E_NOT_POW2, MZK_E_LENGTH (include/mzk.h); the oracle returns the same numbers
SCHOOLBOOK_MAX = 4096                  # la * lb up to here by the schoolbook rule


def to_ints(arr):
    arr = np.ascontiguousarray(arr, dtype="<u8")
    w = 8 * arr.shape[1]
    raw = arr.tobytes()
    return [int.from_bytes(raw[i:i + w], "little") for i in range(0, len(raw), w)]


def to_arr(fid, vals):
    nl = orc.LIMBS[fid]
    raw = b"".join(int(v).to_bytes(8 * nl, "little") for v in vals)
    return np.frombuffer(raw, dtype="<u8").reshape(len(vals), nl).astype(np.uint64)


def operand(fid, seed, n, zeros=0):
    """n canonical pseudo-random coefficients, the top `zeros` of them zero"""
    a = orc.synth_vector(fid, seed, max(n, 1))[:n].copy()
    if zeros:
        a[n - zeros:] = 0
    return a


def trim(c):
    n = len(c)
    while n and c[n - 1] == 0:
        n -= 1
    return c[:n]


def schoolbook(p, a, b):
    if not a or not b:
        return []
    c = [0] * (len(a) + len(b) - 1)
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                c[i + j] += x * y
    return [v % p for v in c]


def kronecker(p, a, b):
    """a(X) b(X) from ONE integer product a(2^s) b(2^s): every coefficient of the product over the integers is below
    min(la, lb) (p - 1)^2 < 2^(2 bits(p) + bits(min(la, lb))), so at a stride of one bit more, rounded up to bytes, none reaches
    into the next"""
    if not a or not b:
        return []
    stride = (2 * p.bit_length() + min(len(a), len(b)).bit_length() + 1 + 7) // 8
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(stride, "little") for x in v), "little")
    m = len(a) + len(b) - 1
    raw = (pack(a) * pack(b)).to_bytes(stride * (m + 1), "little")
    assert not any(raw[stride * m:])
    return [int.from_bytes(raw[i:i + stride], "little") % p for i in range(0, stride * m, stride)]


_long_products = {}                    # the last few long products: both entry points are asked for the same operands


def product(p, a, b):
    """the la + lb - 1 coefficients of a(X) b(X) mod p, untrimmed; [] when an operand is empty"""
    if len(a) * len(b) <= SCHOOLBOOK_MAX:
        return schoolbook(p, a, b)
    if len(a) + len(b) < 1 << 15:
        return kronecker(p, a, b)
    key = (p, tuple(a), tuple(b))
    if key not in _long_products:
        if len(_long_products) >= 4:
            _long_products.clear()
        _long_products[key] = kronecker(p, a, b)
    return _long_products[key]


def fold(p, c, order):
    """c(X) mod X^order - 1, `order` coefficients"""
    out = list(c[:order]) + [0] * max(0, order - len(c))
    for i in range(order, len(c)):
        out[i % order] = (out[i % order] + c[i]) % p
    return out


def next_power_of_two(m):
    n = 1
    while n < m:
        n <<= 1
    return n


def fft_multiply(fid, a, b):
    """(rc, coefficient array) of Polynomial::fft_multiply for any omega of order n: (E_LENGTH, None) for the usize underflow of
    two empty operands (:244)"""
    p = orc.MOD[fid]
    a, b = to_ints(a), to_ints(b)
    if len(a) + len(b) == 0:
        return E_LENGTH, None
    m = len(a) + len(b) - 1
    n = next_power_of_two(m)                       # :245
    a, b = a[:n], b[:n]                            # :248-251 resize(n): cuts, or fills with zeros that add nothing to the product
    c = fold(p, product(p, a, b), n)               # :254-269 transform, Hadamard, inverse transform = the product mod X^n - 1
    return 0, to_arr(fid, trim(c[:m]))             # :272-275


def fast_order(degree, root_order):
    order = root_order
    while degree < order // 2:                     # :90-93
        order //= 2
    return order


def fast_multiply(fid, a, b, root_order):
    """(rc, coefficient array) of ntt::fast_multiply for a primitive root of order root_order (the assertions :75-76 hold)"""
    p = orc.MOD[fid]
    a, b = to_ints(a), to_ints(b)
    ta, tb = trim(a), trim(b)
    if not ta or not tb:                           # :78-80
        return 0, to_arr(fid, [])
    degree = len(ta) + len(tb) - 2
    if degree < 8:                                 # :86-88 lhs * rhs, trimmed (mul_ref, polynomial.rs:302-316)
        return 0, to_arr(fid, trim(product(p, ta, tb)))
    order = fast_order(degree, root_order)
    # :95-105 the stored coefficients are filled up to `order`, never cut: a longer operand reaches ntt as it is and ntt panics on
    # its length (:8-11) or on the root (:16-23); so does an order that is no power of two
    if len(a) > order or len(b) > order:
        return E_LENGTH, None
    if order & (order - 1):
        return E_NOT_POW2, None
    return 0, to_arr(fid, fold(p, product(p, ta, tb), order))      # :104-115 untrimmed, cyclic


# ---- the shapes at an order boundary, shared by the oracle's and the library's tests -----------------------------------------------
def split_shapes(total):
    """(la, lb) with la + lb = total: near-equal lengths, one coefficient against the rest, and a short second operand"""
    return [((total + 1) // 2, total // 2), (1, total - 1), (total - 3, 3)]


def fft_boundary_shapes(k):
    """m = la + lb - 1 = 2^k fits the order 2^k exactly; m = 2^k + 1 takes the next one"""
    return [(m, s) for m in ((1 << k), (1 << k) + 1) for s in split_shapes(m + 1)]


def fast_boundary_shapes(k):
    """degree = la + lb - 2 = 2^k - 1 fits the order 2^k exactly; degree 2^k takes 2^(k + 1)"""
    return [(1 << k if d < (1 << k) else 2 << k, s) for d in ((1 << k) - 1, 1 << k) for s in split_shapes(d + 2)]
