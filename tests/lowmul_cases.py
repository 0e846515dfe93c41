"""Case lists of the low-half products (cofhe_amd/csrc/mp.hpp: mp_mul_low2) and of nucomp_m12 on both of its routes
(cofhe_amd/csrc/qf.hpp) as plain Python integers, shared by the CPU tier (tests/test_lowmul_cpu.py on the host simulator)
and the GPU tier (tests/test_gpu_lowmul.py on tests/gpu_kernels/lowmul_gpu.hip).  Nothing here touches a library.

A case of nucomp_m12 is (R, C, v1, v2, m, s, c2d) with C, m, s signed, v1 | v2 R - m C and v1 | s R + c2d C; expected are
M1 = (v2 R - m C) / v1 and M2 = (s R + c2d C) / v1 by Python's exact division, and whether the bound of qf.hpp lets the
group take the low-half route: nb + 1 + tz(v1) <= 640 for both quotients, tz(v1) < 32, where
nb = max(bits x0 + bits y0, bits x1 + bits y1) - bits(v1) + 2 (below zero: the quotient is zero) -- written out again here, from the derivation in
qf.hpp and not from its code.  TEST INFRASTRUCTURE."""
import json
import math
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyref as P  # noqa: E402

import simlib as S  # noqa: E402

LOW = 1 << 640
PLANE = 1 << 1280
MUL_IN, MUL_OUT, M12_IN, M12_OUT = 160, 40, 322, 123
# the largest |M| the bound admits: |M| v1 = |A +- B| with A = x0 y0 <= (2^a - 1)(2^b - 1), a + b = bits x0 + bits y0, which
# is largest for a == b; nb + 1 + tz <= 640 allows a + b - bits(v1) + 2 <= 639, and v1 = 1 (one bit, tz = 0) makes the most
# of it: a + b = 638, A = B = (2^319 - 1)^2, M = 2 (2^319 - 1)^2 = 2^639 - 2^321 + 2
T319 = (1 << 319) - 1
M_LARGEST = 2 * T319 * T319


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def tz(v):
    return (v & -v).bit_length() - 1


def bound(bx0, by0, bx1, by1, bv1):
    return max(bx0 + by0, bx1 + by1) - bv1 + 2


def serves(nb, v1):
    t = tz(v1)
    return t < 32 and nb + 1 + t <= 640


def bounds(case):
    R, C, v1, v2, m, s, c2d = case
    bl = lambda x: abs(x).bit_length()
    return bound(bl(v2), bl(R), bl(m), bl(C), bl(v1)), bound(bl(s), bl(R), bl(c2d), bl(C), bl(v1))


def low_route(case):
    """the group's own verdict: both quotients within the bound"""
    nb1, nb2 = bounds(case)
    return serves(nb1, case[2]) and serves(nb2, case[2])


def expected(case):
    R, C, v1, v2, m, s, c2d = case
    n1, n2 = v2 * R - m * C, s * R + c2d * C
    assert v1 > 0 and n1 % v1 == 0 and n2 % v1 == 0, "not a case of an exact division"
    return n1 // v1, n2 // v1


def check_fits(case):
    R, C, v1, v2, m, s, c2d = case
    assert all(0 <= abs(x) < PLANE for x in (R, C, v1, v2, m, s)) and 0 <= c2d < PLANE * PLANE and R >= 0 and v2 >= 0
    M1, M2 = expected(case)
    assert abs(M1) < PLANE and abs(M2) < PLANE * PLANE
    return case


def build(v1, R, C, M1, M2, v2_bits, c2d_bits):
    """a case with the given quotients: v2 and s are fixed modulo |C| by exactness (R and C coprime), the rest is size"""
    aC = abs(C)
    assert aC >= 1 and math.gcd(R, aC) == 1
    inv = pow(R, -1, aC) if aC > 1 else 0
    v2 = (M1 * v1 * inv) % aC
    v2 += ((1 << v2_bits) // aC) * aC if v2_bits else 0
    if v2 == 0:
        v2 = aC
    m = (v2 * R - M1 * v1) // C
    assert m * C == v2 * R - M1 * v1
    # s R + c2d C = M2 v1 with c2d >= 0 near 2^c2d_bits: s near (M2 v1 - 2^c2d_bits C) / R, in its residue class
    want = ((M2 * v1 - (1 << c2d_bits) * C) // R) if c2d_bits else (M2 * v1) // R
    s0 = (M2 * v1 * inv) % aC if aC > 1 else 0
    s = want - ((want - s0) % aC)
    c2d = (M2 * v1 - s * R) // C
    while c2d < 0:
        s -= aC if C > 0 else -aC
        c2d = (M2 * v1 - s * R) // C
    assert c2d * C == M2 * v1 - s * R
    return check_fits((R, C, v1, v2, m, s, c2d))


def _odd(rng, bits):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def _coprime_pair(rng, rb, cb):
    while True:
        R, C = _odd(rng, rb), (rng.getrandbits(cb) | (1 << (cb - 1))) if cb > 1 else 1
        if math.gcd(R, C) == 1:
            return R, C


def synthetic_cases():
    """(name, case): sizes of a 2088-bit discriminant unless the name says otherwise"""
    rng = random.Random(640)
    out = []

    def std(M1, M2, csign=1, v1=None, name="", c2d_bits=1040, v2_bits=1038, rb=522, cb=520, near=False):
        R, C = _coprime_pair(rng, rb, cb)
        v1 = v1 or _odd(rng, 1044)
        if near:                              # M2 near c2d C / v1, so that s stays within a plane
            M2 += ((csign * C) << c2d_bits) // v1
        out.append((name, build(v1, R, csign * C, M1, M2, v2_bits, c2d_bits)))

    # every sign of C with every sign and zero of M1, M2 (the signs of m and s follow and are recorded below)
    for csign in (1, -1):
        for M1 in (0, rng.getrandbits(521), -rng.getrandbits(521)):
            for M2 in (0, rng.getrandbits(522), -rng.getrandbits(522)):
                std(M1, M2, csign, name="signs")
    # trailing zero bits of v1: 0, 1, 31 on the low route; 32 and more is mp_divexact's long-division branch, the full route
    for t in (0, 1, 31, 32, 45):
        std(rng.getrandbits(500), -rng.getrandbits(500), 1, v1=_odd(rng, 1000) << t, name="tz%d" % t)
        std(-rng.getrandbits(500), rng.getrandbits(500), -1, v1=_odd(rng, 1000) << t, name="tz%d" % t)
    # C = 1: a partial sequence of no rounds (C0 = 0, C1 = 1, R = the first remainder)
    for d1, M2 in ((0, rng.getrandbits(1040)), (1, -rng.getrandbits(500))):
        v1, R = _odd(rng, 1044), _odd(rng, 1040)
        out.append(("C=1", build(v1, R, 1, (R << 1040) // v1 + d1, M2, 1040, 1040)))      # v2 = 2^1040, |m| < v1
    out.append(("C=1 small", build(_odd(rng, 600), _odd(rng, 590), 1, 5, -7, 500, 600)))
    # the bound at its edge: nb2 + 1 + tz == 640 and 641 through the length of c2d (bits(c2d) + bits(C) - bits(v1) + 2 == nb2)
    for t in (0, 3):
        for total in (640, 641):
            while True:
                v1 = _odd(rng, 700 - t) << t
                R, C = _coprime_pair(rng, 300, 400)
                case = build(v1, R, C, rng.getrandbits(200), (1 << (total - 5 - t)) + rng.getrandbits(600), 600, total - t + 700 - 400 - 4)
                if bounds(case)[1] + 1 + t == total and bounds(case)[0] + 1 + t < 640:
                    break
            out.append(("edge%d tz%d" % (total, t), case))
    # the same edge for M1 through the length of m (v1 = 1, C = 1: M1 = v2 R - m C, nb1 = bits(m) + 1 - 1 + 2)
    for mb in (637, 638):
        x = (1 << 300) - 1
        case = check_fits((x, 1, 1, x, -((1 << mb) - 1), 3, 11))
        assert bounds(case)[0] + 1 == mb + 3
        out.append(("edge m%d" % mb, case))
    # the largest magnitude the bound admits (M_LARGEST, above) with both signs; the nearest smaller one that operands of
    # the same lengths reach (M_LARGEST - T319: M_LARGEST - 1 would need (T319 - 1)(T319 + 1) = 2^320 (2^318 - 1) as a
    # product of lengths 319 + 319, and 2^318 - 1 = (2^159 - 1)(2^159 + 1) only splits into lengths that add up to one more);
    # and M_LARGEST + 1, which no operands within the bound give: it must come from the full route
    T = T319
    out.append(("largest", check_fits((T, T, 1, T, -T, T, T))))                        # M1 = M2 = T T + T T
    out.append(("largest neg", check_fits((T, -T, 1, 1, -T, -T, T))))                  # M1 = T - T T, M2 = -T T - T T
    out.append(("below", check_fits((T, T, 1, T, -(T - 1), T - 1, T))))                # M1 = M2 = T T + (T - 1) T
    out.append(("above", check_fits((T, 1, 1, T, -(T * T + 1), T, T * T + 1))))        # M1 = M2 = 2 T T + 1
    assert [expected(c) for _, c in out[-4:]] == [(M_LARGEST, M_LARGEST), (T - T * T, -M_LARGEST), (M_LARGEST - T, M_LARGEST - T),
                                                  (M_LARGEST + 1, M_LARGEST + 1)]
    assert [low_route(c) for _, c in out[-4:]] == [True, True, True, False]
    # M2 of two planes: a small v1 under a full-size c2d (forms with small first coefficients), and a v1 of one word
    std(rng.getrandbits(900), rng.getrandbits(1000), 1, v1=_odd(rng, 40), name="two planes", c2d_bits=2000, v2_bits=30, rb=20, cb=18, near=True)
    std(-rng.getrandbits(300), -rng.getrandbits(900), -1, v1=_odd(rng, 9), name="two planes", c2d_bits=2040, v2_bits=8, rb=5, cb=4, near=True)
    return out


def _load(name):
    return json.load(open(os.path.join(HERE, "golden", name)))


def partial_sequence(f1, f2, half_dbits, rounds=None):
    """the operands qf_compose hands to nucomp_m12 for coprime first coefficients: both pairs (R1, C1), (R0, C0)"""
    if f1.a < f2.a:
        f1, f2 = f2, f1
    if math.gcd(f1.a, f2.a) != 1:
        return []
    s, m = (f1.b + f2.b) // 2, (f1.b - f2.b) // 2
    v1, v2, c2d = f1.a, f2.a, f2.c
    r = (pow(v2, -1, v1) * m) % v1 if v1 > 1 else 0
    stop = (v1.bit_length() - v2.bit_length() + half_dbits) // 2
    R0, R1, C0, C1 = v1, r, 0, 1
    n = 0
    while R1 != 0 and (R1.bit_length() > stop if rounds is None else n < rounds):
        q = R0 // R1
        R0, R1, C0, C1 = R1, R0 - q * R1, C1, C0 - q * C1
        n += 1
    return [(R1, C1, v1, v2, m, s, c2d), (R0, C0, v1, v2, m, s, c2d)]


def parameter_set_cases():
    """operands of real compositions from the three committed parameter sets: random forms, squarings, a form with its
    inverse, powers of f (small first coefficients: M2 of two planes) -- at the composition's own stopping point and after
    no rounds at all"""
    out = []
    for name in ("tiny_k8", "s128_k128", "s128_k256"):
        prm = _load("params_%s.json" % name)
        d, k = hx(prm["delta"]), prm["k"]
        half = ((-d).bit_length() + 1) // 2
        rng = P.SplitMix64(77)
        g = [P.random_form(d, rng, 12, 10) if name == "tiny_k8" else P.random_form(d, rng) for _ in range(4)]
        f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
        f2 = P.compose(f, f)
        fk = P.power(f, 1 << (k - 2), d)
        pairs = [(g[0], g[1]), (g[2], P.inverse(g[3])), (g[0], g[0]), (g[1], P.inverse(g[1])), (g[0], f), (f2, g[1]), (fk, g[2]), (fk, P.inverse(f2)),
                 (P.inverse(g[3]), P.inverse(g[2]))]
        for a, b in pairs:
            for rounds in (None, 0):
                for case in partial_sequence(a, b, half, rounds):
                    if case[2] > 0 and case[0] >= 0:
                        expected(case)
                        out.append((name, check_fits(case)))
    return out


_cases = None


def m12_cases():
    """the shared list [(name, case)], made once"""
    global _cases
    if _cases is None:
        _cases = synthetic_cases() + parameter_set_cases()
    return _cases


def pack_m12(case, try_low=1):
    R, C, v1, v2, m, s, c2d = case
    signs = (1 if C < 0 else 0) | (2 if m < 0 else 0) | (4 if s < 0 else 0)
    return np.concatenate([S.to_limbs(R, 40), S.to_limbs(abs(C), 40), S.to_limbs(v1, 40), S.to_limbs(v2, 40), S.to_limbs(abs(m), 40),
                           S.to_limbs(abs(s), 40), S.to_limbs(c2d, 80), np.array([signs, try_low], dtype=np.uint32)])


def unpack_m12(rec):
    """(M1, M2, low) of an output record; a zero magnitude may carry either sign flag"""
    assert int(rec[120]) in (0, 1) and int(rec[121]) in (0, 1) and int(rec[122]) in (0, 1)
    M1, M2 = S.from_limbs(rec[:40]), S.from_limbs(rec[40:120])
    return (-M1 if rec[120] else M1), (-M2 if rec[121] else M2), int(rec[122])


def mul_cases():
    """(x0, y0, x1, y1), one-plane operands; only their limbs 0..19 may matter"""
    rng = random.Random(641)
    r = lambda b: rng.getrandbits(b) if b else 0
    cases = []
    for b in (0, 1, 32, 33, 159, 160, 161, 320, 522, 639, 640, 641, 1044, 1280):
        cases.append((r(b), r(640), r(640), r(b)))
        cases.append((r(b), r(b), r(1280), r(1280)))
    ones = LOW - 1
    cases += [(ones, ones, ones, ones), (PLANE - 1, PLANE - 1, 1, PLANE - 1), (0, ones, ones, 0), (1, 1, ones, 1), (1 << 639, 1 << 639, 1 << 639, 3),
              ((1 << 160) - 1, (1 << 160) + 1, (1 << 480) - 1, (1 << 160) - 1), (ones << 640, ones, ones, ones << 640)]
    # products that end in long runs of zeros or ones: the hand-over words wrap the chunk sums, the bits that remain travel
    # through all-ones chunks (the second and third pass of the carry loop)
    for T in (1 << 480, 1 << 320, 1 << 160, 1 << 639, ones, ones - (1 << 160) + 1, (1 << 480) - 1, ((1 << 160) - 1) << 160, 1):
        for _ in range(4):
            y, y2 = r(640) | 1, r(640) | 1
            cases.append(((T * pow(y, -1, LOW)) % LOW, y, (((LOW - T) % LOW) * pow(y2, -1, LOW)) % LOW, y2))
    return cases


def pack_mul(case):
    return np.concatenate([S.to_limbs(v, 40) for v in case])


def expected_mul(case):
    x0, y0, x1, y1 = case
    return S.to_limbs(((x0 % LOW) * (y0 % LOW)) % LOW | ((((x1 % LOW) * (y1 % LOW)) % LOW) << 640), 40)
