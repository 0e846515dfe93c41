"""Cases of the sign from digit comparisons shared by the CPU tier (compare.hpp compiled for the host) and the GPU tier
(k_cmp_rows, k_cmp_close, the tuples, the protocol): masks and opened values as exponent records, and the reference in Python
integers.  TEST INFRASTRUCTURE.

A value is a pair (magnitude, sign word), as in lut_cases: the record of -0 and of a negative magnitude of 2^k and above have no
Python integer of their own."""
import numpy as np

from lut_cases import records  # noqa: F401  (re-exported: the tests build their records with it)

# (k, bits, digit_bits): the digit width divides the window or not, one digit per word boundary crossed, the widest window, the
# most digits (n = 10 at (639, 64, 7))
PARAMS = ((8, 8, 2), (8, 8, 3), (128, 16, 4), (128, 17, 5), (128, 32, 6), (128, 64, 8), (639, 64, 7))
MAX_BITS, MAX_DIGIT_BITS, MAX_DIGITS, LUT_MAX_BITS = 64, 8, 11, 12


def digits_of(bits, d):
    return -(-bits // d)


def shape_ok(bits, d, k, lut_max=LUT_MAX_BITS):
    if not 1 <= k <= 639 or not 2 <= bits <= min(k, MAX_BITS) or not 1 <= d <= MAX_DIGIT_BITS:
        return False
    return digits_of(bits, d) + 1 <= min(lut_max, k)


def pick_digit_bits(bits, k, lut_max=LUT_MAX_BITS):
    """the d that minimises n 2^d + 2^(n + 2) ciphertexts per element (the comparison tuple and the two lookups of n + 1 bits),
    the smallest such d; None when no d is allowed"""
    best = None
    for d in range(1, MAX_DIGIT_BITS + 1):
        if shape_ok(bits, d, k, lut_max):
            n = digits_of(bits, d)
            cost = n * (1 << d) + (1 << (n + 2))
            if best is None or cost < best[0]:
                best = (cost, d)
    return None if best is None else best[1]


def low(val, bits):
    """the value of a record mod 2^bits: Python's % is the residue in [0, 2^bits) of a negative number too"""
    mag, neg = val
    return (-mag if neg else mag) % (1 << bits)


def thresholds(u, bits):
    M = 1 << bits
    a, b = ((M >> 1) - u) % M, (-u) % M
    return a, b, int(a > b)


def digit(v, j, d):
    return (v >> (j * d)) & ((1 << d) - 1)


def sgn(v):
    return (v > 0) - (v < 0)


def rows(rs, bits, d):
    """the plaintexts of the tuples as (magnitude, sign word): out[(i n + j) 2^d + c] = 2^j sgn(r_ij - c)"""
    n = digits_of(bits, d)
    out = []
    for r in rs:
        rl = low(r, bits)
        for j in range(n):
            for c in range(1 << d):
                s = sgn(digit(rl, j, d) - c)
                out.append(((1 << j) if s else 0, 1 if s < 0 else 0))
    return out


def s_value(r_low, t, bits, d):
    """S_t = sum_j 2^j sgn(r_j - t_j): the plaintext of the product of the selected entries"""
    return sum((1 << j) * sgn(digit(r_low, j, d) - digit(t, j, d)) for j in range(digits_of(bits, d)))


def entries(i, t, bits, d):
    """the ciphertext indices of the tuple buffer [E][n][2^d] that the threshold t selects for element i"""
    n = digits_of(bits, d)
    return [((i * n + j) << d) + digit(t, j, d) for j in range(n)]


def sign_table(n):
    """g over n + 1 bits: g[v] = 1 for v < 2^n (S >= 0 in two's complement), 0 otherwise"""
    return [1 if v < (1 << n) else 0 for v in range(1 << (n + 1))]


def nonneg_by_protocol(x, r, k, bits, d):
    """[x >= 0] as the protocol computes it, on Python integers; x in the signed window of `bits` bits, r in Z/2^k"""
    n = digits_of(bits, d)
    e = (x - r) % (1 << k)
    u = e % (1 << bits)
    a, b, wrap = thresholds(u, bits)
    g = sign_table(n)
    rl = r % (1 << bits)
    ga = g[s_value(rl, a, bits, d) % (1 << (n + 1))]
    gb = g[s_value(rl, b, bits, d) % (1 << (n + 1))]
    assert ga == int(rl >= a) and gb == int(rl >= b)
    return (1 - wrap) - ga + gb


def edges(bits):
    return [-(1 << (bits - 1)), -1, 0, 1, (1 << (bits - 1)) - 1]


def values(bits, k, n, rng):
    """n masks or opened values: 0, 1, 2^(bits-1), 2^bits - 1, 2^bits, 2^32 and its neighbours, 2^k - 1, the same under a set
    sign word (-0 among them), magnitudes of 2^k and above of either sign, then random ones of up to 992 bits; cut to n"""
    M = 1 << k
    mags = [0, 1, 1 << (bits - 1), (1 << (bits - 1)) - 1, (1 << bits) - 1, 1 << bits, (1 << 32) - 1, 1 << 32, M - 1]
    out = [(m, s) for m in mags for s in (0, 1)]
    out += [(M, 0), (M + 5, 1), ((1 << 900) + rng.getrandbits(k), 0), ((1 << 991) + rng.getrandbits(k), 1)]
    rng.shuffle(out)
    while len(out) < n:
        out.append((rng.getrandbits(rng.choice((bits, k, 992))), rng.randrange(2)))
    return out[:n]


def value_record(v, k):
    """the record (magnitude, sign word) of a Python integer, reduced mod 2^k"""
    return (v % (1 << k), 0)


def u64(a):
    return np.asarray(a, dtype=np.uint64)
