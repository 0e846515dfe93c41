"""Cases and Python-integer oracles of the exact floor division by small public divisors, shared by the CPU tier
(plain_divmod.hpp on the host simulator) and the GPU tier (k_plain_divmod, k_divx_rows, k_divx_select, the closing step, the
protocol).  TEST INFRASTRUCTURE.

Numerators and divisors are those of div_cases: a numerator is a pair (magnitude, sign word), a divisor a Python integer."""
import numpy as np

import div_cases as DC

MAX_ROWS = 4096
ROWS_KBITS = (8, 33, 128, 639)
PROTOCOL_DIVISORS = (1, 2, 3, 5, 7, 8, 16, 100, 127)          # the nine of the exhaustive check at k = 8


def valid_divisor(D, k, rows):
    """as the kernels judge a record: valid for div_cases, and its residue at most rows"""
    return DC.valid_divisor(D, k) and D % (1 << k) <= rows


def divmod_centred(num, D, k, rows=MAX_ROWS):
    """(q(v) mod 2^k, m(v)) of the centred residue of num by D; (0, 0) for an invalid divisor.  Python's divmod is the floor"""
    if not valid_divisor(D, k, rows):
        return 0, 0
    q, m = divmod(DC.centred(DC.value(num), k), D % (1 << k))
    return q % (1 << k), m


def cases(k):
    """div_cases.cases(k) restricted to D <= 4096"""
    return [(v, D) for v, D in DC.cases(k) if D <= MAX_ROWS]


def row_values(r, D, k, rows):
    """T_0 .. T_{rows-1} of the mask r (an integer mod 2^k): q(r) + [m(r) + j >= D] mod 2^k for j < D, zero beyond; all zero for
    an invalid divisor"""
    if not valid_divisor(D, k, rows):
        return [0] * rows
    q, m = divmod(DC.centred(r, k), D)
    return [(q + (1 if m + j >= D else 0)) % (1 << k) if j < D else 0 for j in range(rows)]


def pow2_table(r, t, k):
    """g of the power-of-two identity T_j = g[(j + r) mod 2^t]: g[v] = q(r) + [v < m(r)] mod 2^k, D = 2^t"""
    q, m = divmod(DC.centred(r, k), 1 << t)
    return [(q + (1 if v < m else 0)) % (1 << k) for v in range(1 << t)]


def masks(k, D, rng, extra=3):
    """masks with m(r) in {0, 1, D - 1} on either side of zero, and random ones"""
    half = 1 << (k - 1)
    out = []
    for m in sorted({0, 1 % D, D - 1}):
        qmax = (half - 1 - m) // D
        out += [(rng.randrange(qmax + 1) * D + m) % (1 << k), (-(rng.randrange(1, half // D + 1)) * D + m) % (1 << k)]
    return out + [rng.getrandbits(k) for _ in range(extra)]


def protocol_result(x, r, D, k):
    """what the protocol decrypts to for the value x and the mask r (integers mod 2^k): T_{m(e)} + q(e) mod 2^k"""
    e = (x - r) % (1 << k)
    qe, me = divmod(DC.centred(e, k), D)
    return (row_values(r, D, k, D)[me] + qe) % (1 << k)


def u32_values(recs):
    r = np.asarray(recs, dtype="<u4").reshape(-1, 32)
    return [int.from_bytes(row[:31].tobytes(), "little") for row in r]
