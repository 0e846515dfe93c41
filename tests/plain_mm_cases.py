"""Cases of the plaintext matrix product mod 2^k shared by the CPU tier (plain_mm.hpp on the host) and the GPU tier
(k_plain_matmul): operands as exponent records, the expected product from Python integers.  TEST INFRASTRUCTURE."""
import random

import numpy as np

TILE = 16                                   # k_plain_matmul's output tile and inner step (plain_mm.hpp: PMM_TILE)
# one limb with a sub-word mask, a mask inside the top limb, L = 4, L = 8, the runtime-L path
KBITS = (8, 100, 128, 256, 300)
# one element; no dimension a multiple of anything; one below / at / one above the tile in both output dimensions with an
# inner dimension of two steps and one element
SHAPES = ((1, 1, 1), (3, 5, 4), (15, 33, 17), (16, 33, 16), (17, 33, 15))


def exp_records(vals):
    out = np.zeros((len(vals), 32), dtype=np.uint32)
    for i, v in enumerate(vals):
        out[i, :31] = np.frombuffer(abs(v).to_bytes(124, "little"), dtype="<u4")
        out[i, 31] = 1 if v < 0 else 0
    return out.reshape(-1)


def record_values(recs):
    """[(value of the 31 magnitude words, sign word)] of exponent records"""
    r = np.asarray(recs, dtype="<u4").reshape(-1, 32)
    return [(int.from_bytes(row[:31].tobytes(), "little"), int(row[31])) for row in r]


def operand(count, k, rng, fill=None):
    """`count` values: the edge values first (0, 1, -1, 2^k - 1, its negative, magnitudes of 2^k and above, a 900-bit one),
    then random ones of mixed sign; fill: that value everywhere"""
    if fill is not None:
        return [fill] * count
    top = (1 << k) - 1
    edge = [0, 1, -1, top, -top, 1 << k, (1 << k) + 5, -(3 << k) - 7, (1 << 900) + 12345, -((1 << 991) - 1), -0]
    vals = []
    while len(vals) < count:
        r = rng.random()
        if r < 0.25:
            vals.append(rng.choice(edge))
        elif r < 0.5:
            vals.append(rng.choice((1, -1)) * rng.getrandbits(k + 40))
        else:
            vals.append(rng.choice((1, -1)) * rng.getrandbits(k))
    vals[:min(count, len(edge))] = edge[:count]
    rng.shuffle(vals)
    return vals


def product(a, b, n, m, p, k):
    mod = 1 << k
    return [sum(a[i * m + j] * b[j * p + c] for j in range(m)) % mod for i in range(n) for c in range(p)]


def cases(k):
    """[(name, n, m, p, a, b)]: every shape with mixed operands, and 2^k - 1 everywhere (the longest carries) at two shapes"""
    rng = random.Random(1000 + k)
    out = []
    for n, m, p in SHAPES:
        out.append(("mixed", n, m, p, operand(n * m, k, rng), operand(m * p, k, rng)))
    top = (1 << k) - 1
    for n, m, p in ((3, 5, 4), (17, 33, 15)):
        out.append(("all_top", n, m, p, operand(n * m, k, rng, fill=top), operand(m * p, k, rng, fill=top)))
        out.append(("all_minus_one", n, m, p, operand(n * m, k, rng, fill=-1), operand(m * p, k, rng, fill=top)))
    return out


def check_output(recs, want, k):
    """every record: sign word 0, zero words above ceil(k/32) limbs (implied by value < 2^k), value as expected"""
    got = record_values(recs)
    assert len(got) == len(want)
    for idx, ((v, sign), w) in enumerate(zip(got, want)):
        assert sign == 0, "output %d carries a sign word" % idx
        assert v < (1 << k), "output %d is not reduced mod 2^%d" % (idx, k)
        assert v == w, "output %d differs" % idx
