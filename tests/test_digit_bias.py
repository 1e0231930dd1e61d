"""Signed window digits without the serial carry walk (digit_bias_word / walk_digits_merged, mzk_msm_plan.h; k_small_accumulate_scan,
mzk_msm.hip): with t = k + sum_w (2^(c-1) - 1) 2^(c w), digit_w = window_w(t) - (2^(c-1) - 1) must equal the carry-walking recoding of
walk_digits (digits in (-2^(c-1), 2^(c-1)], raw > half borrows from the next window) for every scalar below r.  A Python restatement;
the C++ itself runs on the host in tests/test_hostcheck_digit_walk.py."""
import random
import msm_layouts
from msm_layouts import R


def walk_digits(k, c):
    nwin = 254 // c + 1
    half = 1 << (c - 1)
    out, carry = [], 0
    for w in range(nwin):
        raw = ((k >> (c * w)) & ((1 << c) - 1)) + carry
        carry = 0
        d = raw
        if raw > half:
            d = raw - (1 << c)
            carry = 1
        out.append(d)
    assert carry == 0
    return out


def biased_digits(k, c):
    nwin = 254 // c + 1
    half = 1 << (c - 1)
    bias = sum((half - 1) << (c * w) for w in range(nwin))
    t = k + bias
    assert t < 1 << 288                                   # nine 32-bit words in the kernel
    return [((t >> (c * w)) & ((1 << c) - 1)) - (half - 1) for w in range(nwin)]


def test_biased_windows_equal_the_carry_walk():
    rng = random.Random(5)
    for c in msm_layouts.WIDTHS:                    # every width a handle can have; 8, 10..13, 16, 17 and 20 have a compile-time walker
        half = 1 << (c - 1)
        special = [0, 1, R - 1, R - 2, half, half + 1, half - 1, (1 << 254) - 1 if (1 << 254) - 1 < R else R - 1]
        special += [sum(half << (c * w) for w in range(254 // c)) % R, sum((half + 1) << (c * w) for w in range(254 // c)) % R]
        for k in special + [rng.randrange(R) for _ in range(3000)]:
            a, b = walk_digits(k, c), biased_digits(k, c)
            assert a == b, (c, hex(k))
            assert sum(d << (c * w) for w, d in enumerate(a)) == k


def test_the_scalar_family_reaches_every_digit_edge_at_every_width():
    """msm_layouts.family(), the scalars the layout tests commit and the host walkers are run over: at every width 8..22 every window
    below the top one sees the signed digits +1, -1, +half, -(half - 1) and half - 1, the top window 0, 1, 2 and the top bits of r - 1,
    and the biased extraction agrees with the carry walk on all of them"""
    fam = msm_layouts.family()
    assert len(fam) == 1177 and fam[0] == 0 and fam[-1] == R - 1 and all(a < b for a, b in zip(fam, fam[1:]))
    for c in msm_layouts.WIDTHS:
        nwin, half = 254 // c + 1, 1 << (c - 1)
        seen = [set() for _ in range(nwin)]
        for k in fam:
            a = walk_digits(k, c)
            assert a == biased_digits(k, c) == msm_layouts.signed_digits(k, c), (c, hex(k))
            assert sum(d << (c * w) for w, d in enumerate(a)) == k
            for w, d in enumerate(a):
                seen[w].add(d)
        for w in range(nwin - 1):
            assert {1, -1, half, -(half - 1), half - 1} <= seen[w], (c, w)
            assert min(seen[w]) == -(half - 1) and max(seen[w]) == half
        assert {0, 1, 2} <= seen[-1] and max(seen[-1]) >= (R - 1) >> (c * (nwin - 1)), (c, sorted(seen[-1]))


def test_the_scalar_vector_keeps_the_family_and_its_blocks():
    rng = random.Random(9)
    s = msm_layouts.scalar_vector([rng.randrange(R) for _ in range(msm_layouts.N_SRS)])
    assert sorted(s[:1177]) == msm_layouts.family() and all(0 <= k < R for k in s)
    head = set(s[:300])
    assert len(head) == 300 and sum(k.bit_length() > 200 for k in head) > 50 and sum(k.bit_length() < 128 for k in head) > 50      # a mix
    lo, hi = msm_layouts.EQUAL_BLOCK
    assert len(set(s[lo:hi])) == 1 and s[lo] != 0 and not any(s[slice(*msm_layouts.ZERO_BLOCK)])
    assert s[msm_layouts.NEG_PAIR[0]] == s[msm_layouts.NEG_PAIR[1]] and len(set(s[slice(*msm_layouts.REPEAT_POINT)])) == 1
