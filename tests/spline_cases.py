"""Cases of the piecewise-polynomial activations from one opened value shared by the CPU tier (spline.hpp compiled for the host)
and the GPU tier (k_spline_rows, k_spline_powers, k_spline_close, the tuples, the protocol): masks and opened values as exponent
records, tables of pieces, and the reference in Python integers.  TEST INFRASTRUCTURE.

A value is a pair (magnitude, sign word), as in lut_cases: the record of -0 and of a negative magnitude of 2^k and above have no
Python integer of their own.  A table is a list of 2^b pieces, a piece a list of d + 1 such pairs."""
import numpy as np

from lut_cases import records  # noqa: F401
from poly_cases import taylor_shift

MAX_TUPLE = 4096                             # spline.hpp: SPLINE_MAX_TUPLE
IDENTITY_CASES = ((2, 3, 2), (3, 0, 1), (1, 7, 3))       # (b, t, d) of the exhaustive check at k = 8


def residue(val, k):
    mag, neg = val
    return (-mag if neg else mag) % (1 << k)


def segment(v, t, b):
    """bits t .. t + b - 1 of a residue"""
    return (v >> t) & ((1 << b) - 1)


def index(val, t, b, k):
    return segment(residue(val, k), t, b)


def origin(p, t, b):
    """o(p) = sigma(p) 2^t, sigma the b-bit two's complement reading"""
    return (p - (1 << b) if p >> (b - 1) else p) << t


def piece_value(coef, p, x, t, b, k):
    """S_p(x) = sum_i c_i (x - o(p))^i mod 2^k, coef: d + 1 integers"""
    u = x - origin(p, t, b)
    return sum(c * u ** i for i, c in enumerate(coef)) % (1 << k)


def rows(pieces, n_tab, rs, b, t, d, k):
    """the plaintext rows of the tuples, as integers in [0, 2^k): out[(i 2^b + j) (d + 1) + c]; pieces: n_tab tables"""
    assert len(pieces) == n_tab << b and all(len(p) == d + 1 for p in pieces)
    M, out = 1 << k, []
    for i, r in enumerate(rs):
        rv = residue(r, k)
        rho = segment(rv, t, b)
        for j in range(1 << b):
            p = (j + rho) % (1 << b)
            coef = [residue(c, k) for c in pieces[((i % n_tab) << b) + p]]
            out += taylor_shift(coef, (rv - origin(p, t, b)) % M, k)
    return out


def powers(es, d, k):
    """power-major: out[(c - 1) n + i] = e_i^c mod 2^k"""
    return [pow(residue(e, k), c, 1 << k) for c in range(1, d + 1) for e in es]


def closed(row, e, k):
    """q_0 + sum_{i >= 1} q_i (e^i mod 2^k) mod 2^k: what the closing step's ciphertext decrypts to"""
    M = 1 << k
    return (row[0] + sum(q * pow(e, i, M) for i, q in enumerate(row) if i)) % M


def expected(table, x, r, b, t, k):
    """S_{(pi(x) - c) mod 2^b}(x), c the carry of the low t bits of e = x - r and r; table: 2^b pieces of integers"""
    M = 1 << k
    e = (x - r) % M
    c = 1 if (e % (1 << t)) + (r % (1 << t)) >= (1 << t) else 0
    p = (segment(x % M, t, b) - c) % (1 << b)
    return piece_value(table[p], p, x % M, t, b, k), p


def int_records(vals):
    """non-negative integers as exponent records"""
    return records([(v, 0) for v in vals])


def values(t, b, k, n, rng):
    """n masks or opened values: 0, 1, the field's own bits alone and all ones below / above it, 2^k - 1, the same under a set
    sign word (-0 among them), magnitudes of 2^k and above of either sign, then random ones of up to 992 bits and either sign;
    cut or cycled to n"""
    M, lo, f = 1 << k, (1 << t) - 1, ((1 << b) - 1) << t
    out = [(0, 0), (1, 0), (f, 0), (lo, 0), (M - 1 - f, 0), (M - 1, 0), (1 << (k - 1), 0), (0, 1), (1, 1), (f, 1), (lo + 1, 1), (M - 1, 1),
           (M, 0), (M, 1), (M + (5 << t), 1), ((1 << 900) + rng.getrandbits(k), 0), ((1 << 991) + rng.getrandbits(k), 1)]
    rng.shuffle(out)
    while len(out) < n:
        out.append((rng.getrandbits(rng.choice((t + b, k, 992))), rng.randrange(2)))
    return out[:n]


def table(b, d, k, n_tab, rng):
    """n_tab tables of 2^b pieces of d + 1 coefficients: random k-bit values, every fifth one of 992 bits and every third one under a
    set sign word, so that the reduction of the coefficients is seen too"""
    out = []
    for p in range(n_tab << b):
        piece = []
        for c in range(d + 1):
            m = rng.getrandbits(992) if (p + c) % 5 == 0 else rng.getrandbits(k)
            piece.append((m, 1 if (p * (d + 1) + c) % 3 == 0 else 0))
        out.append(piece)
    return out


def piece_records(pieces):
    return records([c for p in pieces for c in p])


def sigmoid_table_check(tab, b, t, d, in_frac, out_frac, g):
    """the largest |S_p(x) / 2^out_frac - g(x / 2^in_frac)| over every x of the window outside the lowest segment, on its own piece
    and on the one below; tab: 2^b pieces of signed integers"""
    worst = 0.0
    half = 1 << (b - 1)
    xs = np.arange(-(half - 1) << t, half << t, dtype=np.int64)             # sigma(pi(x)) > -2^(b-1)
    want = g(xs.astype(np.float64) / (1 << in_frac))
    for c in (0, 1):
        sig = (xs >> t) - c                                                  # sigma of the piece used
        p = sig % (1 << b)
        u = (xs - (sig << t)).astype(np.float64)
        coef = np.array(tab, dtype=np.float64)[p]                            # [len(xs), d + 1]
        val = sum(coef[:, i] * u ** i for i in range(d + 1)) / (1 << out_frac)
        worst = max(worst, float(np.abs(val - want).max()))
    return worst
