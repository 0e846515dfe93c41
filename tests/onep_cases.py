"""Case lists of the one-plane tail of the composition as plain Python integers: mp_mul_half2 and mp_sqr_low
(cofhe_amd/csrc/mp.hpp), nucomp_ab and nucomp_c on both of their routes (cofhe_amd/csrc/qf.hpp).  Shared by the CPU tier
(tests/test_onep_cpu.py on the host simulator) and the GPU tier (tests/test_gpu_onep.py on tests/gpu_kernels/onep_gpu.hip).
Nothing here touches a library.

A case of nucomp_ab is (R1, C1, R0, C0, M1, M2, b1, m2_one_plane) with C1, C0, M1, M2, b1 signed; expected are
a' = R1 M1 + C1 M2 and b' = -sgn 2 (R0 M1 + C0 M2) - b1 with sgn = -1 for C1 < 0 and +1 otherwise, and whether the bounds
of qf.hpp let the group take the one-plane route: m2_one_plane, every operand of both dots at most 640 bits,
bits R + bits M1 <= 1277 and bits C + bits M2 <= 1277 for both pairs, bits b1 <= 1279.  A case of nucomp_c is (a, b, D) with
4 a | b^2 + D; expected is c = (b^2 + D) / (4 a), and the low half serves when nbc + 2 + tz(a) <= 1280 and tz(a) < 32 for
nbc = max(2 bits b, bits D) - bits a.  Both predicates are written out again here, from the derivations in qf.hpp and not
from its code.  TEST INFRASTRUCTURE."""
import math
import random

import numpy as np

import lowmul_cases as LC
import simlib as S
from lowmul_cases import P, hx, tz

HALF = 1 << 640
PLANE = 1 << 1280
MUL_IN, MUL_OUT, SQR_IN, SQR_OUT, AB_IN, AB_OUT, C_IN, C_OUT = 160, 80, 40, 40, 322, 163, 161, 81
MUL_LENGTHS = (0, 1, 32, 33, 159, 160, 161, 320, 522, 639, 640)


def bl(x):
    return abs(x).bit_length()


# ---------------------------------------------------------------------------- mp_mul_half2
def mul_cases():
    """(x0, y0, x1, y1) as one-plane values; only limbs 0..19 may matter (several cases carry garbage above them)"""
    rng = random.Random(1277)
    r = lambda b: (rng.getrandbits(b) | (1 << (b - 1))) if b else 0
    ones = HALF - 1
    cases = []
    for b in MUL_LENGTHS:
        cases.append((r(b), r(640), r(640), r(b)))
        cases.append((r(b), r(b), r(640 - b), r(b)))
        cases.append((r(b) | (rng.getrandbits(640) << 640), r(640), r(522), r(b) | (rng.getrandbits(640) << 640)))      # garbage in limbs 20..39
    cases += [(ones, ones, ones, ones), (0, ones, ones, ones), (ones, ones, ones, 0), (0, 0, 0, 0), (1, 1, ones, 1), (ones, 1, 1, 1),
              (ones | (ones << 640), ones | (ones << 640), ones | (1 << 640), ones | (ones << 640))]
    # products that end in, or consist of, long runs of ones and zeros: the chunk sums hand over words into all-ones chunks
    for a in (160, 320, 480, 640):
        for b in (160, 320, 480, 640):
            cases.append(((1 << a) - 1, (1 << b) - 1, ((1 << a) - 1) << (640 - a), (1 << b) - 1))
    for a in (80, 160, 320):
        cases.append(((1 << a) - 1, (1 << a) + 1, (1 << 2 * a) - 1, (1 << 2 * a) + 1 if a < 320 else 1))   # 2^2a - 1, 2^4a - 1: all ones
        cases.append((1 << a, 1 << (639 - a), (1 << 639), (1 << 639)))
    for _ in range(6):
        y = r(320)
        cases.append((ones, y, (ones // 3), 3 * (y | 1) & ones))
        cases.append((((1 << 480) - 1) << 160, r(640), ((1 << 160) - 1) * ((1 << 320) + 1), ones))
    return cases


def pack_mul(case):
    return np.concatenate([S.to_limbs(v, 40) for v in case])


def expected_mul(case):
    x0, y0, x1, y1 = case
    return np.concatenate([S.to_limbs((x0 % HALF) * (y0 % HALF), 40), S.to_limbs((x1 % HALF) * (y1 % HALF), 40)])


# ---------------------------------------------------------------------------- mp_sqr_low
def sqrt_2adic(t, n=1280):
    """x with x^2 == t (mod 2^n), t == 1 (mod 8)"""
    assert t % 8 == 1
    x = 1
    for i in range(3, n):
        if (x * x - t) % (1 << (i + 1)):
            x += 1 << (i - 1)
    assert (x * x - t) % (1 << n) == 0
    return x % (1 << n)


def sqr_cases():
    rng = random.Random(1280)
    r = lambda b: (rng.getrandbits(b) | (1 << (b - 1))) if b else 0
    cases = [r(b) for b in (0, 1, 32, 33, 159, 160, 161, 320, 522, 639, 640, 641, 800, 960, 1044, 1120, 1121, 1279, 1280) for _ in range(2)]
    cases += [PLANE - 1, 1 << 640, (1 << 640) - 1, (1 << 640) + 1, 1 << 1279, (1 << 1279) - 1, 1 << 639, HALF - 1 << 640, (1 << 1120) - 1]
    # squares that are long runs of ones modulo 2^1280: 2^1280 - 2^k + 1, and runs of zeros: 2^k + 1
    for k in (3, 32, 160, 161, 320, 640, 1119, 1120, 1279):
        cases.append(sqrt_2adic(PLANE - (1 << k) + 1))
        cases.append(sqrt_2adic((1 << k) + 1))
    return cases


def expected_sqr(x):
    return S.to_limbs((x * x) % PLANE, 40)


# ---------------------------------------------------------------------------- nucomp_ab
def ab_expected(case):
    R1, C1, R0, C0, M1, M2, b1, _ = case
    sgn = -1 if C1 < 0 else 1
    return R1 * M1 + C1 * M2, -sgn * 2 * (R0 * M1 + C0 * M2) - b1


def dot_serves(R, C, M1, M2):
    return max(bl(R), bl(C), bl(M1), bl(M2)) <= 640 and bl(R) + bl(M1) <= 1277 and bl(C) + bl(M2) <= 1277


def ab_one_plane(case):
    """the group's own verdict"""
    R1, C1, R0, C0, M1, M2, b1, m2_one_plane = case
    return bool(m2_one_plane) and dot_serves(R1, C1, M1, M2) and dot_serves(R0, C0, M1, M2) and bl(b1) <= 1279


def check_ab(case):
    R1, C1, R0, C0, M1, M2, b1, flag = case
    assert R1 >= 0 and R0 >= 0 and all(bl(x) <= 1280 for x in (R1, C1, R0, C0, M1, b1)) and bl(M2) <= (1280 if flag else 2560)
    an, bn = ab_expected(case)
    assert bl(an) <= 2559 and bl(bn) <= 2559
    return case


def ab_synthetic_cases():
    rng = random.Random(1278)
    r = lambda b: (rng.getrandbits(b) | (1 << (b - 1))) if b else 0
    out = []
    add = lambda name, *case: out.append((name, check_ab(tuple(case))))
    # every sign and zero of C, M1, M2 (C1 and C0 of opposite signs, as cofactors are), both signs of b1
    for sc in (1, -1, 0):
        for s1 in (1, -1, 0):
            for s2 in (1, -1, 0):
                add("signs", r(522), sc * r(520), r(530), -sc * r(512), s1 * r(521), s2 * r(522), (1 if (sc + s1 + s2) & 1 else -1) * r(1044), 1)
    # near-total cancellation of the two products: R M1 == C M2 up to a few low bits, and exactly
    for d in (0, 1, -1, 1 << 40):
        x, y = r(520), r(523)
        add("cancel", x, -y, x + d, -(y + 1), y, x + d, r(1040), 1)
        add("cancel", x, y, x, -y, -y, x + d, -r(1040), 1)
    # an operand of 640 bits against one of 641, in each position
    for pos in range(6):
        for nb in (640, 641):
            v = [r(600), r(600), r(610), -r(590), r(620), -r(620)]
            v[pos] = (1 if v[pos] > 0 else -1) * r(nb)
            add("op%d" % nb, v[0], v[1], v[2], v[3], v[4], v[5], r(1000), 1)
    # a product at 2^1277 and just above: bits R + bits M1 == 1277 / 1278 (the largest values of those lengths), then C with M2
    for tot in (1277, 1278):
        add("prod%d" % tot, (1 << 640) - 1, r(100), r(500), -r(90), (1 << (tot - 640)) - 1, r(100), r(1000), 1)
        add("prod%d" % tot, r(100), -((1 << 638) - 1), r(90), r(600), -r(100), (1 << (tot - 638)) - 1, -r(1000), 1)
        add("prod%d" % tot, r(100), -r(100), (1 << 639) - 1, r(600), -((1 << (tot - 639)) - 1), r(100), -r(1000), 1)
    # b1 at 1279 bits against 1280, both signs, with the doubled dot at its largest and of the sign that adds up
    for nb in (1279, 1280):
        for sb in (1, -1):
            add("b1_%d" % nb, r(500), r(500), (1 << 640) - 1, -r(10), sb * ((1 << 637) - 1), r(10), sb * ((1 << nb) - 1), 1)
    # the no-rounds case of a discriminant of full size: R0 = v1 of a plane, C0 = 0, C1 = 1
    add("no rounds", r(1040), 1, r(1044), 0, r(1038), -r(1040), r(1043), 1)
    add("no rounds", r(1040), 1, r(1044), 0, -r(500), r(520), -r(1043), 1)
    # M2 of two planes (nucomp_m12 took the full products): the flag alone sends the group to the double-width dots
    add("m2 two planes", r(20), r(18), r(30), -r(10), r(900), -r(2000), r(40), 0)
    add("flag off", r(522), -r(520), r(530), r(512), r(521), r(522), r(1044), 0)
    # a' and b' of two planes
    add("two-plane ab", r(1044), -r(1000), r(1100), r(900), r(1040), r(1200), -r(1044), 1)
    add("two-plane ab", r(641), r(700), r(1279), -r(640), -r(1270), r(1279), r(1280), 1)
    return out


PRIMES23 = (2, 3, 5, 7, 11, 13, 17, 19, 23)


def representative(fa, fb):
    """the form of fb's class that qf_compose composes fa with: the first of (a, b, c), (c, -b, a) and the forms with first
    coefficient f(1, 1), f(1, -1), f(1, 2), f(1, -2) that shares no prime <= 23 with fa.a; never fb itself when the first
    coefficients are equal (a squaring, a form with its inverse).  Written from the description in qf.hpp."""
    a, b, c = fb.a, fb.b, fb.c
    if bl(c) > 1280 - 110:
        return fb
    cand = [(a, b, c), (c, -b, a), (a + b + c, b + 2 * c, c), (a - b + c, b - 2 * c, c), (a + 2 * b + 4 * c, b + 4 * c, c),
            (a - 2 * b + 4 * c, b - 4 * c, c)]
    for k in range(1 if fa.a == fb.a else 0, 6):
        if not any(cand[k][0] % p == 0 and fa.a % p == 0 for p in PRIMES23):
            return P.Form(*cand[k])
    return fb


def composition_operands(fa, fb, delta, rounds=None):
    """What qf_compose hands to nucomp_m12, nucomp_ab and nucomp_c for ANY pair, by the formulas at the head of qf.hpp: the
    coprime representative, a1 >= a2, d = gcd(a1, a2), d1 = gcd(s, d) = x2 s - y2 d, v1 = a1 / d1, v2 = a2 / d1,
    r = (-y1 y2 m - x2 c2) mod v1, the partial sequence down to the composition's stopping point (or `rounds` rounds of it),
    M1 and M2 of the pair (R1, C1).  Returns (m12 case, (R1, C1, R0, C0, M1, M2, b1)), or None when a sequence has no step
    left (r == 0).  The device may pick another y1 or x2 (any choice gives a form of the same class), so these are operands of
    the right kind and size, not necessarily the device's own bit for bit; a', b', c' made from them are checked below to be
    a form of the product's class."""
    half = ((-delta).bit_length() + 1) // 2
    f2 = representative(fa, fb)
    f1 = fa
    if f1.a < f2.a:
        f1, f2 = f2, f1
    s, m = (f1.b + f2.b) // 2, (f1.b - f2.b) // 2
    d, y1, _ = P.xgcd(f2.a, f1.a)                       # y1 a2 == d (mod a1)
    assert d == math.gcd(f1.a, f2.a) and (y1 * f2.a - d) % f1.a == 0
    d1, x2, t = P.xgcd(s, d) if s else (d, 0, 1)
    if d1 < 0:
        d1, x2, t = -d1, -x2, -t
    y2 = -t
    assert x2 * s - y2 * d == d1
    v1, v2, c2d = f1.a // d1, f2.a // d1, f2.c * d1
    r = (-y1 * y2 * m - x2 * f2.c) % v1
    stop = (v1.bit_length() - v2.bit_length() + half) // 2
    R0, R1, C0, C1 = v1, r, 0, 1
    n = 0
    while R1 != 0 and (R1.bit_length() > stop if rounds is None else n < rounds):
        q = R0 // R1
        R0, R1, C0, C1 = R1, R0 - q * R1, C1, C0 - q * C1
        n += 1
    m12 = (R1, C1, v1, v2, m, s, c2d)
    M1, M2 = LC.expected(m12)                           # asserts both divisions exact
    return m12, (R1, C1, R0, C0, M1, M2, f1.b)


def ab_parameter_set_cases():
    """[(name, case, |Delta|)]: operands of real compositions of the three committed parameter sets, named "<set> <kind>" with
    the kinds random (pairs of random forms), squaring (of random forms), inverse (a form with its inverse), f power (powers
    of f with random forms, with each other and squared), each at the composition's own stopping point and after no rounds.
    m2_one_plane is what nucomp_m12 would report for the group alone: both quotients within the low-half bound."""
    out = []
    for name in ("tiny_k8", "s128_k128", "s128_k256"):
        prm = LC._load("params_%s.json" % name)
        d, k = hx(prm["delta"]), prm["k"]
        rng = P.SplitMix64(78)
        g = [P.random_form(d, rng, 12, 10) if name == "tiny_k8" else P.random_form(d, rng) for _ in range(8)]
        f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
        f2 = P.compose(f, f)
        fk = P.power(f, 1 << (k - 2), d)
        pairs = [("random", g[0], g[1]), ("random", g[2], P.inverse(g[3])), ("random", P.inverse(g[3]), P.inverse(g[2])), ("random", g[4], g[5]),
                 ("random", g[6], P.inverse(g[7])), ("random", g[5], g[6]), ("random", g[7], g[4]), ("random", g[1], g[2]),
                 ("squaring", g[0], g[0]), ("squaring", g[3], g[3]), ("squaring", P.inverse(g[5]), P.inverse(g[5])),
                 ("inverse", g[1], P.inverse(g[1])), ("inverse", P.inverse(g[6]), g[6]),
                 ("f power", g[0], f), ("f power", f2, g[1]), ("f power", fk, g[2]), ("f power", f2, f2), ("f power", fk, fk), ("f power", f, fk)]
        for kind, a, b in pairs:
            want = P.compose(a, b)
            for rounds in (None, 0):
                ops = composition_operands(a, b, d, rounds)
                if ops is None or ops[0][0] < 0:
                    continue
                m12, (R1, C1, R0, C0, M1, M2, b1) = ops
                case = check_ab((R1, C1, R0, C0, M1, M2, b1, 1 if LC.low_route(m12) else 0))
                an, bn = ab_expected(case)
                if an > 0:                                  # the model itself: (a', b', c') is a form of the product's class
                    cn = c_expected((an, abs(bn), -d))
                    got = P.reduce_form(an, bn, cn)
                    assert (got.a, got.b, got.c) == (want.a, want.b, want.c), (name, kind)
                out.append(("%s %s" % (name, kind), case, -d))
    return out


_ab = None


def ab_cases():
    """the shared list [(name, case)], made once"""
    global _ab
    if _ab is None:
        _ab = ab_synthetic_cases() + [(n, c) for n, c, _ in ab_parameter_set_cases()]
    return _ab


def pack_ab(case):
    R1, C1, R0, C0, M1, M2, b1, flag = case
    signs = sum(1 << i for i, v in enumerate((C1, C0, M1, M2, b1)) if v < 0)
    return np.concatenate([S.to_limbs(R1, 40), S.to_limbs(abs(C1), 40), S.to_limbs(R0, 40), S.to_limbs(abs(C0), 40), S.to_limbs(abs(M1), 40),
                           S.to_limbs(abs(M2), 80), S.to_limbs(abs(b1), 40), np.array([signs, flag], dtype=np.uint32)])


def unpack_ab(rec):
    """(a', b', one-plane route taken) of an output record; a zero magnitude may carry either sign flag"""
    assert int(rec[160]) in (0, 1) and int(rec[161]) in (0, 1) and int(rec[162]) in (0, 1)
    an, bn = S.from_limbs(rec[:80]), S.from_limbs(rec[80:160])
    return (-an if rec[160] else an), (-bn if rec[161] else bn), int(rec[162])


# ---------------------------------------------------------------------------- nucomp_c
def c_bound(case):
    a, b, D = case
    return max(2 * bl(b), bl(D)) - bl(a)


def c_low(case):
    t = tz(case[0])
    return t < 32 and c_bound(case) >= 1 and c_bound(case) + 2 + t <= 1280


def c_expected(case):
    a, b, D = case
    assert a > 0 and D > 0 and (b * b + D) % (4 * a) == 0, "not a case of an exact division"
    return (b * b + D) // (4 * a)


def c_make(a, b, c):
    """the case with the given quotient: |Delta| = 4 a c - b^2"""
    case = (a, abs(b), 4 * a * c - b * b)
    assert case[2] > 0 and bl(case[2]) <= 2560 and bl(a) <= 1280 and bl(b) <= 1280 and c_expected(case) == c and bl(c) <= 2560
    return case


def c_synthetic_cases():
    rng = random.Random(1281)
    r = lambda b: (rng.getrandbits(b) | (1 << (b - 1))) if b else 0
    odd = lambda b: r(b) | 1
    out = []
    # trailing zero bits of a': 0, 1, 31 on the low route; 32 is mp_divexact's long-division branch, the full route
    for t in (0, 1, 31, 32):
        for _ in range(3):
            a, b = odd(1040 - t) << t, r(1043)
            out.append(("tz%d" % t, c_make(a, b, b * b // (4 * a) + r(1040))))
    # nbc + 2 + tz at 1280 and at 1281, through the length of b' (2 bits b' decides) and through the length of |Delta|
    for t in (0, 5):
        for total in (1280, 1281):
            ab_ = 500
            nbc = total - 2 - t
            while True:
                a = odd(ab_ - t) << t
                if (nbc + ab_) % 2 == 0:
                    b = r((nbc + ab_) // 2)                       # 2 bits b' == nbc + bits a'; |Delta| shorter
                    case = c_make(a, b, b * b // (4 * a) + 1 + rng.getrandbits(600))
                else:
                    b = r((nbc + ab_ - 1) // 2 - 3)               # bits |Delta| == nbc + bits a' decides; b' shorter
                    case = c_make(a, b, (1 << (nbc + ab_ - 1)) // (4 * a) + (1 << (nbc - 8)))
                if c_bound(case) == nbc:
                    break
            out.append(("edge%d tz%d" % (total, t), case))
    # small and lopsided forms: b' == 0, a' == 1, c' of one word, a' of one word under a c' of two planes
    out.append(("b zero", c_make(odd(900), 0, r(1000))))
    out.append(("a one", c_make(1, r(600), r(1210))))
    out.append(("c small", c_make(odd(1044), 3, 5)))
    out.append(("c two planes", c_make(odd(30), r(20), r(2000))))
    out.append(("c two planes", c_make(odd(600) << 3, r(1100), r(1900))))
    # quotients that are long runs of ones and zeros
    for q in ((1 << 1046) - 1, 1 << 1045, (1 << 1200) - (1 << 170), (1 << 1278) - 1):
        a = odd(bl(q) > 1200 and 1 or 1040)
        out.append(("runs", c_make(a, r(min(1043, (bl(q) + bl(a)) // 2)), q)))
    return out


_c = None


def c_cases():
    """[(name, case)]: the synthetic ones and the (a', b') of the real compositions of ab_parameter_set_cases that fit a plane"""
    global _c
    if _c is None:
        out = c_synthetic_cases()
        for name, case, D in ab_parameter_set_cases():
            an, bn = ab_expected(case)
            if 0 < an < PLANE and abs(bn) < PLANE:
                c_expected((an, abs(bn), D))
                out.append((name, (an, abs(bn), D)))
        _c = out
    return _c


def pack_c(case):
    a, b, D = case
    return np.concatenate([S.to_limbs(a, 40), S.to_limbs(b, 40), S.to_limbs(D, 80), np.array([(bl(D) + 1) // 2], dtype=np.uint32)])


def unpack_c(rec):
    assert int(rec[80]) in (0, 1)
    return S.from_limbs(rec[:80]), int(rec[80])
