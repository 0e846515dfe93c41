"""Cases of the polynomial evaluation shared by the CPU tier (pow_dot.hpp and poly_shift.hpp on the host) and the GPU tier
(k_pow_dot, k_poly_shift): exponent families, the signed digits the kernel reads, and the Taylor shift from Python integers.
TEST INFRASTRUCTURE."""
import math

MAX_DEGREE = 8                              # pow_dot.hpp: POLY_MAX_DEGREE
EXP_BITS = 992                              # magnitude bits of an exponent record


def naf(v):
    """the non-adjacent form of |v|, position 0 first, every digit times the sign of v (what k_pow_dot reads: qf.hpp's
    digit_i = bit_(i+1)(3 |v|) - bit_(i+1)(|v|), negated for a set sign word)"""
    s, m, out = (-1 if v < 0 else 1), abs(v), []
    while m:
        dg = 0
        if m & 1:
            dg = 2 - (m & 3)
            m -= dg
        out.append(s * dg)
        m >>= 1
    return out


def walk_counts(exps):
    """(squarings, multiplications) of the shared-squarings walk over these exponents: T and non-zero digits - 1"""
    digs = [naf(v) for v in exps]
    nz = sum(1 for dg in digs for x in dg if x)
    if nz == 0:
        return 0, 0
    return max(len(dg) for dg in digs) - 1, nz - 1


def exponent_families(d, k, rng):
    """[(name, d exponents)]: all zero; one zero among non-zero; ones; 2^k - 1; negative; lengths 3, 128 and 992 bits mixed over
    the bases; the top digit shared by several bases; random k-bit values"""
    top = (1 << k) - 1
    rnd = lambda bits: rng.getrandbits(bits) | (1 << (bits - 1))     # noqa: E731
    zero_among = [rnd(k) for _ in range(d)]
    zero_among[rng.randrange(d)] = 0
    lengths = [(3, 128)[(i - 1) % 2] if i else EXP_BITS for i in range(d)]                 # one 992-bit exponent, then 3, 128, 3, ..
    mixed = [rnd(b) * (-1 if i % 4 == 3 else 1) for i, b in enumerate(lengths)]
    if d == 1:
        zero_among = [0]
    return [("all zero", [0] * d), ("one zero among non-zero", zero_among), ("ones", [1] * d), ("2^k - 1", [top] * d),
            ("negative", [-rnd(k) if i % 2 == 0 else rnd(k) for i in range(d)]), ("minus ones", [-1] * d),
            ("lengths 3, 128 and 992 mixed", mixed), ("shared top digit", [(1 << (k - 1)) | rng.getrandbits(k - 1) for _ in range(d)]),
            ("equal exponents", [rnd(k)] * d), ("random", [rng.getrandbits(k) for _ in range(d)])]


def taylor_shift(coef, x, k):
    """[q_0 .. q_d] with q_i = sum_{j >= i} C(j, i) c_j x^(j - i) mod 2^k"""
    d, M = len(coef) - 1, 1 << k
    return [sum(math.comb(j, i) * coef[j] * x ** (j - i) for j in range(i, d + 1)) % M for i in range(d + 1)]


def poly(coef, x, k):
    return sum(c * x ** j for j, c in enumerate(coef)) % (1 << k)


def shift_points(k, n, rng):
    """n values of x: 0, 1, 2^k - 1, 2^(k-1), then random k-bit ones"""
    vals = [0, 1, (1 << k) - 1, 1 << (k - 1)]
    return (vals + [rng.getrandbits(k) for _ in range(max(0, n - len(vals)))])[:n]
