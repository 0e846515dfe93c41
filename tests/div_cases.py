"""Cases of the signed floor division mod 2^k shared by the CPU tier (plain_div.hpp on the host simulator) and the GPU tier
(k_plain_divfloor, the closing step, the protocol): numerators and divisors as exponent records, the expected quotient from
Python integers.  TEST INFRASTRUCTURE.

A numerator is a pair (magnitude, sign word): the record of -0 and of a negative magnitude of 2^k and above have no Python
integer of their own.  A divisor is a Python integer (negative: a record with a set sign word)."""
import random

import numpy as np

import prim_cases as PC

KBITS_CPU = (8, 33, 64, 128, 256, 300, 639)   # sub-word mask; sign bit = bit 0 of the top limb; bit 31 of a limb; L = 4, 8; runtime L; the bound
KBITS_GPU = (8, 33, 128, 639)
ST_DIV_CAP = 4                               # lane.hpp: CF_ST_DIV_CAP


def centred(v, k):
    """s(v): the residue of v mod 2^k in [-2^(k-1), 2^(k-1))"""
    v %= 1 << k
    return v - (1 << k) if v >> (k - 1) else v


def value(num):
    mag, neg = num
    return -mag if neg else mag


def valid_divisor(D, k):
    """as the kernel judges a record: no sign word, residue of the magnitude in [1, 2^(k-1))"""
    return D > 0 and 1 <= D % (1 << k) < (1 << (k - 1))


def divfloor(num, D, k):
    """floor(s(v) / D) mod 2^k (0 for an invalid divisor); Python's // is the floor"""
    if not valid_divisor(D, k):
        return 0
    return (centred(value(num), k) // (D % (1 << k))) % (1 << k)


def records(nums):
    out = np.zeros((len(nums), 32), dtype=np.uint32)
    for i, (mag, neg) in enumerate(nums):
        out[i, :31] = np.frombuffer(mag.to_bytes(124, "little"), dtype="<u4")
        out[i, 31] = 1 if neg else 0
    return out.reshape(-1)


def int_records(vals):
    return records([(abs(v), v < 0) for v in vals])


def divisors(k, rng):
    """1, 2, 3, powers of two, 2^(k-1) - 1, one-limb, two-limb and full-width values, as far as they are below 2^(k-1)"""
    top = (1 << (k - 1)) - 1
    ds = [1, 2, 3, top, 1 << (k - 2), 1 << ((k - 1) // 2)]
    for bits in (5, 31, 32, 33, 63, 64, 65, k - 2, k - 1):
        if 2 <= bits <= k - 1:
            ds.append(rng.getrandbits(bits) | (1 << (bits - 1)))
    return sorted({d for d in ds if 1 <= d <= top})


def numerators(k, D, rng):
    """the fixed residues, multiples of D and their neighbours of either sign, |v| < D, records with a set sign word, magnitudes
    of 2^k and above (up to 900 bits) and -0"""
    M, half = 1 << k, 1 << (k - 1)
    out = [(0, 0), (1, 0), (M - 1, 0), (half, 0), (half - 1, 0), (0, 1), (1, 1), (half, 1), (half + 1, 1), (M - 1, 1)]
    q = rng.randrange(half // D + 1)
    for m in (q * D, q * D - 1, q * D + D - 1):
        if 0 <= m < half:
            out += [(m, 0), (M - m, 0)]             # +m, and -m as a residue
        if 0 <= m <= half:
            out.append((m, 1))                      # -m as a record with a set sign word
    small = rng.randrange(D)
    out += [(small, 0), (small, 1), (M - small, 0)]
    out += [(M, 0), (M, 1), (M + 5, 0), (3 * M + 7, 1), ((1 << 900) + rng.getrandbits(k), 0), ((1 << 899) + rng.getrandbits(k), 1)]
    out += [(rng.getrandbits(k), rng.randrange(2)) for _ in range(2)]
    return out


def addback_pairs(k):
    """(numerator, divisor) with the numerators +-qD, +-(qD - 1), +-(qD + D - 1) for the q and D of prim_cases'
    divrem_addback_cases (divisors beyond one limb: the digit estimates of mp_divrem_norm land one above and its add-back runs);
    everything stays inside the centred range"""
    M, half = 1 << k, 1 << (k - 1)
    den_bits = [b for b in (33, 64, 65, 127, 255, 299, 600, 637) if b <= k - 2]
    out = []
    for i, (num, den, fam) in enumerate(PC.divrem_addback_cases(k - 1, den_bits, [1, 32, 33, 65, 200, 544], seed=800 + k)):
        Q = (num + 1) // den - fam
        # what the kernel divides is m for +m and m - 1 for -m: every family member on either side of the sign
        for m in (Q * den, Q * den - 1, Q * den + den - 1):
            if m < half:
                out.append(((m, 0), den))
            if 0 < m <= half:
                out.append(((M - m, 0), den) if i % 3 else ((m, 1), den))
    return out


def cases(k):
    """[(numerator, divisor)] of one k: every divisor with its numerators, then the add-back family"""
    rng = random.Random(500 + k)
    out = []
    for D in divisors(k, rng):
        out += [(v, D) for v in numerators(k, D, rng)]
    return out + addback_pairs(k)


def invalid_divisors(k):
    """0, 2^(k-1), 2^k - 1, 2^k (residue 0), and a valid magnitude under a set sign word"""
    return [0, 1 << (k - 1), (1 << k) - 1, 1 << k, -5 if k > 4 else -1]


def check_output(recs, want, k):
    """every record: sign word 0, value below 2^k (so zero words above ceil(k/32) limbs), value as expected"""
    r = np.asarray(recs, dtype="<u4").reshape(-1, 32)
    assert len(r) == len(want)
    for idx, (row, w) in enumerate(zip(r, want)):
        v = int.from_bytes(row[:31].tobytes(), "little")
        assert row[31] == 0, "output %d carries a sign word" % idx
        assert v < (1 << k), "output %d is not reduced mod 2^%d" % (idx, k)
        assert v == w, "output %d differs: got %x, want %x" % (idx, v, w)


def no_wrap_masks(xs, k, rng):
    """for every x a mask r with s(x) = s(r) + s(e) over the integers, e = x - r mod 2^k: r uniform among those with
    -2^(k-1) <= s(x) - s(r) < 2^(k-1)"""
    half = 1 << (k - 1)
    out = []
    for x in xs:
        sx = centred(x, k)
        lo, hi = max(-half, sx - half + 1), min(half - 1, sx + half)
        out.append(rng.randint(lo, hi) % (1 << k))
    return out
