"""Cases of the table lookups from one opened value shared by the CPU tier (lut.hpp compiled for the host) and the GPU tier
(k_lut_rotate, k_lut_select, the tuples, the protocol): masks and opened values as exponent records, tables of distinct
records, and the reference in Python integers.  TEST INFRASTRUCTURE.

A value is a pair (magnitude, sign word): the record of -0 and of a negative magnitude of 2^k and above have no Python integer
of their own.  A table entry is such a pair too, so that a table can hold records with set sign words."""
import random

import numpy as np

BITS_CPU = (1, 2, 3, 8, 12)
BITS_GPU = (1, 3, 8)
SIZES_GPU = (1, 7, 8, 9, 63, 64, 65)         # one wavefront's 8 records of the rotate, one workgroup of either kernel, each +-1
MAX_BITS = 12                                # lut.hpp: LUT_MAX_BITS


def index(val, b):
    """the value of a record mod 2^b: Python's % is the residue in [0, 2^b) of a negative number too"""
    mag, neg = val
    return (-mag if neg else mag) % (1 << b)


def records(vals):
    out = np.zeros((len(vals), 32), dtype=np.uint32)
    for i, (mag, neg) in enumerate(vals):
        out[i, :31] = np.frombuffer(mag.to_bytes(124, "little"), dtype="<u4")
        out[i, 31] = 1 if neg else 0
    return out.reshape(-1)


def values(b, k, n, rng):
    """n masks or opened values: 0, 1, 2^b - 1, 2^b, 2^k - 1, the same under a set sign word (-0 among them), magnitudes of 2^k
    and above of either sign, then random ones of up to 992 bits and either sign; cut or cycled to n"""
    M = 1 << k
    out = [(0, 0), (1, 0), ((1 << b) - 1, 0), (1 << b, 0), (M - 1, 0), (0, 1), (1, 1), ((1 << b) - 1, 1), (1 << b, 1), (M - 1, 1),
           (M, 0), (M + 5, 1), ((1 << 900) + rng.getrandbits(k), 0), ((1 << 991) + rng.getrandbits(k), 1)]
    rng.shuffle(out)
    while len(out) < n:
        out.append((rng.getrandbits(rng.choice((b, k, 992))), rng.randrange(2)))
    return out[:n]


def table(b, n_tab, rng):
    """n_tab tables of 2^b entries, every record of all of them distinct (the low 24 bits of the magnitude number it), so a wrong
    index cannot pass; every third entry has 992 bits and every other one a set sign word, so all 32 words are seen copied"""
    assert n_tab << b <= 1 << 24
    out = []
    for t in range(n_tab << b):
        hi = rng.getrandbits(960) | (1 << 959) if t % 3 == 0 else rng.getrandbits(rng.choice((8, 100, 700)))
        out.append(((hi << 32) | (rng.getrandbits(8) << 24) | t, t & 1))
    assert len(set(out)) == len(out)
    return out


def rotate(tab, n_tab, rs, b):
    """the rows of the tuples: out[i 2^b + j] = tab[(i mod n_tab) 2^b + ((j + r_i) mod 2^b)]"""
    size = 1 << b
    assert len(tab) == n_tab * size
    return [tab[(i % n_tab) * size + (j + index(r, b)) % size] for i, r in enumerate(rs) for j in range(size)]


def selected(es, b):
    """the entry of the tuple buffer that element i's opened value names"""
    return [(i << b) + index(e, b) for i, e in enumerate(es)]


def relu_table(b):
    """g[v] = v for 0 < v < 2^(b-1), 0 otherwise: the ReLU of a b-bit signed value read as its two's-complement index"""
    return [v if 0 < v < (1 << (b - 1)) else 0 for v in range(1 << b)]


def signed(v, b):
    v %= 1 << b
    return v - (1 << b) if v >> (b - 1) else v
