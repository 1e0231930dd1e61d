"""The window-table layouts a caller can commit through (mzk_srs_from_device_ex: 8..22 bits; mzk_set_table_budget: two or four bucket
sets at 14..17 bits), the path msm_plan (myzkp_amd/csrc/mzk_msm_plan.h) gives each of them by the number of coefficients, and the
scalars that reach every edge of the signed-digit recoding at every width.  Shared by tests/test_msm_plan.py, tests/test_digit_bias.py,
tests/test_hostcheck_digit_walk.py (CPU) and tests/test_gpu_msm_layouts.py.  Plain Python integers; no GPU, no library."""
import random

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
N_SRS = 1 << 15
PREFIXES = (1, 300, 4095, 4096, 4097, 16384, 16385, 32768)
WIDTHS = tuple(range(8, 23))
LAYOUTS = tuple((c, 1) for c in WIDTHS) + tuple((c, s) for c in range(14, 18) for s in (2, 4))

SCAN, SSORT, TWO, LDS = "SmallScan", "SmallSort", "TwoLevel", "LdsOnePass"
PATH_ID = {SCAN: 0, SSORT: 1, TWO: 2, LDS: 3}                     # MsmPath (mzk_msm_plan.h)


def rows(c, s):
    """tables of a handle with s bucket sets: every s-th window (msm_table_rows)"""
    return 254 // (c * s) + 1


# the path of every prefix of PREFIXES, default knobs, table stride N_SRS; it does not depend on the CU count
_SCAN_LDS = (SCAN,) * 6 + (LDS,) * 2
_LDS_TWO = (LDS,) * 3 + (TWO,) * 5
_TWO = (TWO,) * 8
EXPECTED_PATH = {
    (8, 1): _SCAN_LDS, (10, 1): _SCAN_LDS, (11, 1): _SCAN_LDS, (12, 1): _SCAN_LDS,
    (13, 1): (SCAN,) * 6 + (TWO,) * 2,
    (9, 1): (SSORT,) * 4 + (LDS,) * 4,
    (14, 1): (SSORT,) * 4 + (TWO,) * 4,
    (15, 1): _LDS_TWO, (16, 1): _LDS_TWO, (14, 2): _LDS_TWO, (14, 4): _LDS_TWO, (15, 2): _LDS_TWO,
    (17, 1): _TWO, (18, 1): _TWO, (19, 1): _TWO, (20, 1): _TWO, (21, 1): _TWO, (22, 1): _TWO,
    (15, 4): _TWO, (16, 2): _TWO, (16, 4): _TWO, (17, 2): _TWO, (17, 4): _TWO,
}
# further facts of the TwoLevel entries: buckets per coarse bin with one bucket set, the compile-time coarse kernels, the 1024-bin sort,
# and the one width whose sort records need 8 bytes at this stride (references below 12 x 2^15 do not fit 31 - 13 bits)
EXPECTED_F = {13: 16, 14: 32, 15: 64, 16: 128, 17: 256, 18: 512, 19: 1024, 20: 512, 21: 4096, 22: 8192}
EXPECTED_COARSE_C = {(16, 1): 16, (17, 1): 17, (20, 1): 20}
EXPECTED_CL = {(20, 1): 10}
EXPECTED_WIDE_RECORDS = {(22, 1)}


# ---- scalars ---------------------------------------------------------------------------------------------------------------------------
def width_family(c):
    """scalars that put 1, half - 1, half, half + 1 and 2^c - 1 into every window of width c, alone and in all windows at once, and
    2^(c w) - 1: digit -1, zeros, then +1 at window w -- a carry that runs the whole length"""
    half, full, nwin = 1 << (c - 1), (1 << c) - 1, 254 // c + 1
    out = []
    for d in (1, half - 1, half, half + 1, full):
        out += [d << (c * w) for w in range(nwin) if d << (c * w) < R]
        v = sum(d << (c * w) for w in range(nwin))
        while v >= R:
            v >>= c
        out.append(v)
    out += [(1 << (c * w)) - 1 for w in range(1, nwin + 1) if (1 << (c * w)) - 1 < R]
    return out


FIXED = (0, 1, R - 1, R - 2, (R - 1) // 2, (R + 1) // 2)


def family():
    """the union over the widths 8..22, sorted: 1177 scalars"""
    u = set(FIXED)
    for c in WIDTHS:
        u.update(width_family(c))
    return sorted(u)


def signed_digits(k, c):
    """the carry-walking recoding of walk_digits (mzk_msm_plan.h): digits in (-2^(c-1), 2^(c-1)]"""
    nwin, half = 254 // c + 1, 1 << (c - 1)
    out, carry = [], 0
    for w in range(nwin):
        raw = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 1 if raw > half else 0
        out.append(raw - (carry << c))
    assert carry == 0
    return out


# where the structured rows and blocks of scalar_vector sit: the points of tests/test_gpu_msm_layouts.py repeat / negate at the same rows
REPEAT_POINT = (1200, 1240)        # one point, one scalar: the bucket sees P + P
NEG_PAIR = (1300, 1301)            # P and -P under equal scalars
REPEAT_SCALAR = (1400, 1450)       # one scalar on different points
EQUAL_BLOCK = (2048, 2560)
ZERO_BLOCK = (2560, 3072)


def scalar_vector(uniform):
    """N_SRS scalars as integers: the family shuffled with a fixed seed (the prefix of 300 holds a mix), then `uniform` (N_SRS
    integers below r) with the structured rows, a block of equal scalars and a block of zeros written over it"""
    fam = family()
    random.Random(2215).shuffle(fam)
    s = fam + [int(x) for x in uniform[len(fam):N_SRS]]
    assert len(s) == N_SRS and len(fam) < REPEAT_POINT[0]
    for lo, hi in (REPEAT_POINT, REPEAT_SCALAR, EQUAL_BLOCK):
        s[lo:hi] = [s[lo]] * (hi - lo)
    s[NEG_PAIR[0]] = s[NEG_PAIR[1]]
    s[ZERO_BLOCK[0]:ZERO_BLOCK[1]] = [0] * (ZERO_BLOCK[1] - ZERO_BLOCK[0])
    return s
