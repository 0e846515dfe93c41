"""Case lists of the remainder-only long division (cofhe_amd/csrc/mp.hpp: mp_rem_norm, mp_lincomb_sub_carry_sparse) and of the
step r = y1 m mod a1 of the composition (qf.hpp: smod with its remainder-only flag) as plain Python integers, shared by the
CPU tier (tests/test_remnorm_cpu.py on the host simulator) and the GPU tier (tests/test_gpu_remnorm.py on
tests/gpu_kernels/remnorm_gpu.hip).  Nothing here touches a library.

Expected values are Python's: num % den, and for a whole step (y1 * m) % a1 -- Python's % of a negative product is the
residue in [0, a1), which is the sign rule of smod.

model(num, den) walks the division as mp.hpp describes it -- the divisor shifted to the top bit of the plane, one f64 digit
estimate per 32-bit digit (Python floats are IEEE doubles; every operation of the estimate rounds once, also when it is
contracted into a fused multiply-add, because its products are by powers of two), the add-back when the estimate is one
too large, and each lane's carry chain of S + q ~D + q up to the word it hands over -- and counts the digits, the add-backs
and the steps in which some lane's limb 1 is all ones before the hand-over (the general carry resolve).  It is used to FIND
inputs that take the rare paths, with fixed seeds, and to say so when a list is made; that the code took them is asserted
from the simulator's own counters in the CPU tier.  TEST INFRASTRUCTURE."""
import random

import numpy as np

import lowmul_cases as LC
import simlib as S

M32 = 0xFFFFFFFF
PLANE_BITS = 1280
PLANE = 1 << PLANE_BITS
REM_IN, REM_OUT, REM1_IN, REM1_OUT, STEP_IN, STEP_OUT = 120, 80, 80, 40, 121, 40


def _estimate(top, l39, l38, rd):
    x = ((float(top) * 4294967296.0 + float(l39)) * 4294967296.0 + float(l38)) * rd
    x += x * 1.7763568394002505e-15
    return min(int(x), M32)


def _limb1_all_ones(Sv, q, D):
    """does some lane's limb 1 of S + q ~D + q equal 2^32 - 1 before the lanes hand their words over?"""
    for g in range(8):
        prev, carry = (q if g == 0 else 0), 0
        for j in range(2):
            i = 5 * g + j
            t = ((Sv >> (32 * i)) & M32) + q * (~(D >> (32 * i)) & M32)
            s = (t & M32) + prev + carry
            carry, prev = s >> 32, t >> 32
            if j == 1 and (s & M32) == M32:
                return True
    return False


def model(num, den):
    """(remainder, digits, add-backs, steps through the general resolve) of num mod den, den beyond one word"""
    db, nb = den.bit_length(), num.bit_length()
    assert db > 32
    if nb < db:
        return num, 0, 0, 0
    s = PLANE_BITS - db
    D, N = den << s, num << s
    K = (nb + s - 1) >> 5
    rd = 1.0 / (float(D >> (39 * 32)) * 4294967296.0 + float((D >> (38 * 32)) & M32))
    Sv, top = N >> (32 * (K - 39)), 0
    assert Sv < PLANE
    digits = addbacks = general = 0
    for k in range(K - 39, -1, -1):
        digits += 1
        q = _estimate(top, Sv >> (39 * 32), (Sv >> (38 * 32)) & M32, rd)
        if q:
            general += 1 if _limb1_all_ones(Sv, q, D) else 0
            v = (top << PLANE_BITS) + Sv - q * D
            while v < 0:
                addbacks += 1
                v += D
            assert v < D
            Sv = v
        if k == 0:
            break
        top = Sv >> (39 * 32)
        Sv = ((Sv << 32) % PLANE) | ((N >> (32 * (k - 1))) & M32)
    assert Sv >> s == num % den and Sv % (1 << s) == 0
    return Sv >> s, digits, addbacks, general


def _rnd(rng, bits):
    return rng.getrandbits(bits) | (1 << (bits - 1)) if bits > 0 else 0


# ---------------------------------------------------------------------------- mp_rem_norm<2>
_rem = None


def rem_cases():
    """[(name, (num, den))]: num below 2^2560, den of 33 to 1280 bits"""
    global _rem
    if _rem is not None:
        return _rem
    rng = random.Random(1800)
    out = []
    add = lambda name, num, den: out.append((name, (num, den)))
    den = _rnd(rng, 1044)
    # the early return
    add("num below den", den - 1, den)
    add("num below den", _rnd(rng, 700), den)
    add("num below den", 0, den)
    # a remainder of zero: one digit, many digits, the numerator the divisor itself
    add("remainder zero", den, den)
    add("remainder zero", den * _rnd(rng, 1000), den)
    add("remainder zero", den * M32, den)
    # the shift s = 1280 - bits(den): bits(den) a multiple of 32 (no bit shift: the staged numerator is a copy), one below it
    # (a shift by one bit) and one above it (by 31 bits)
    for db in (1024, 1056, 64, 1280):
        add("den bits 0 mod 32", _rnd(rng, 2 * db - 7 if db < 1280 else 2559), _rnd(rng, db))
        add("den bits 31 mod 32", _rnd(rng, 2 * db - 40 if db < 1280 else 2500), _rnd(rng, db - 1))
        if db < 1280:
            add("den bits 1 mod 32", _rnd(rng, 2 * db), _rnd(rng, db + 1))
    # the shortest divisor beyond the word path (38 zero words under the staged numerator) and the longest below a full plane
    for nb in (33, 34, 64, 65, 1300, 2559, 2560):
        add("den 33 bits", _rnd(rng, nb), _rnd(rng, 33))
    add("den 33 bits", (1 << 2560) - 1, (1 << 32) + 1)
    add("den 33 bits", (1 << 2560) - 1, (1 << 33) - 1)
    for nb in (1279, 1280, 1311, 1312, 2000, 2558, 2560):
        add("den 1279 bits", _rnd(rng, nb), _rnd(rng, 1279))
    add("den 1280 bits", (1 << 2560) - 1, (1 << 1280) - 1)
    add("den 1280 bits", (1 << 2560) - 1, 1 << 1279)
    add("den 1280 bits", _rnd(rng, 2560), _rnd(rng, 1280))
    # two planes with nothing in the upper one
    for nb in (1045, 1100, 1279, 1280):
        add("empty top plane", _rnd(rng, nb), den)
    add("empty top plane", PLANE - 1, _rnd(rng, 640))
    # the largest products smp_mul makes of two 1044-bit operands, under divisors of that length
    big = (1 << 1044) - 1
    add("largest product", big * big, big)
    add("largest product", big * big, (1 << 1043) + 1)
    add("largest product", big * big, den)
    add("largest product", big * (big - 2), big - 1)
    # remainder den - 1: every estimate that is rounded up lands one above the digit (the add-back)
    n0 = len(out)
    for db, qb in ((1044, 1040), (1044, 33), (640, 1300), (33, 2000), (1279, 1280), (1280, 1279), (65, 64), (1024, 1024), (1055, 100)):
        d = _rnd(rng, db)
        for dd in (d, (1 << db) - 1, (1 << (db - 1)) + 1):
            Q = _rnd(rng, qb)
            add("add-back family", dd * Q - 1, dd)
            add("add-back family", dd * Q + dd - 1, dd)
    assert sum(model(*c)[2] for _, c in out[n0:]) >= 10, "the family no longer reaches the add-back"
    # a step whose remainder has an all-ones limb 1 in one lane and nothing carried into it: the general resolve without an
    # add-back.  A whole-limb shift s and a quotient of two digits: after the last digit S is the remainder moved up by s / 32
    # limbs; the seeds are searched with the model
    n0 = len(out)
    for lane in (0, 3, 7):
        for db in (1280, 1248):
            for seed in range(64):
                r2 = random.Random(1810 + 100 * lane + seed)
                d = _rnd(r2, db)
                T = _rnd(r2, db - 2)
                T |= M32 << (32 * (5 * lane + 1 - (PLANE_BITS - db) // 32))      # limb 1 of the lane once T is shifted by s
                if T >= d:
                    continue
                case = (d * _rnd(r2, 30) + T, d)
                mo = model(*case)
                if mo[2] == 0 and mo[3] >= 1:
                    add("limb 1 all ones, lane %d" % lane, *case)
                    break
    assert len(out) - n0 >= 4, "no seed reaches the general resolve without an add-back"
    # a long division (33 digits) that meets such a limb on its way: remainder limbs forced to all ones at the last digit
    d = _rnd(rng, 1044)
    for seed in range(64):
        r2 = random.Random(1850 + seed)
        T = (_rnd(r2, 1040) | (M32 << (32 * 11))) % d
        case = (d * _rnd(r2, 1040) + T, d)
        if model(*case)[3] >= 1:
            add("limb 1 all ones, 33 digits", *case)
            break
    # remainders with zero limbs in the middle of a lane, and with zero lanes
    for db in (1044, 1280, 700):
        d = _rnd(rng, db)
        for mask in (~(M32 << 64) & ~(M32 << (32 * 17)), ~(((1 << 96) - 1) << (32 * 6)), ~(((1 << 160) - 1) << 160), ~(M32 << 32) & ~M32):
            T = (_rnd(rng, db - 1) & mask) % d
            add("zero limbs in the remainder", d * _rnd(rng, db - 5) + T, d)
    # random operands of every length relation
    for nb, db in ((2088, 1044), (2087, 1044), (2000, 1000), (1500, 1200), (2560, 40), (2560, 100), (1281, 1280), (2100, 33), (77, 76)):
        add("random", _rnd(rng, nb), _rnd(rng, db))
    for name, (n, dd) in out:
        assert 0 <= n < 1 << 2560 and 32 < dd.bit_length() <= 1280, name
    _rem = out
    return out


def pack_rem(case):
    return np.concatenate([S.to_limbs(case[0], 80), S.to_limbs(case[1], 40)])


def rem1_cases():
    """the one-plane instantiation: the cases above whose numerator fits a plane"""
    return [(n, c) for n, c in rem_cases() if c[0] < PLANE]


def pack_rem1(case):
    return np.concatenate([S.to_limbs(case[0], 40), S.to_limbs(case[1], 40)])


# ---------------------------------------------------------------------------- whole steps r = y1 m mod a1
_steps = None


def _bezout(a1, a2):
    """y1 with y1 a2 == gcd (mod a1) as the remainder sequence leaves it (|y1| < a1, either sign), and the gcd"""
    r0, r1, u0, u1 = a1, a2, 0, 1
    while r1:
        q = r0 // r1
        r0, r1, u0, u1 = r1, r0 - q * r1, u1, u0 - q * u1
    return u0, r0


def step_cases():
    """[(name, (y1, m, a1))] from compositions of the three committed parameter sets: random pairs, a squaring and a form
    with its inverse (equal first coefficients: the second operand by its representative (c, -b, a), as qf_compose takes
    another one), powers of f; every y1 with both of its signs"""
    global _steps
    if _steps is not None:
        return _steps
    P = LC.P
    out = []
    for name in ("tiny_k8", "s128_k128", "s128_k256"):
        prm = LC._load("params_%s.json" % name)
        d, k = LC.hx(prm["delta"]), prm["k"]
        rng = P.SplitMix64(78)
        g = [P.random_form(d, rng, 12, 10) if name == "tiny_k8" else P.random_form(d, rng) for _ in range(6)]
        f = P.Form(LC.hx(prm["f"]["a"]), LC.hx(prm["f"]["b"]), LC.hx(prm["f"]["c"]))
        f2 = P.compose(f, f)
        fk = P.power(f, 1 << (k - 2), d)
        pairs = [("random", g[0], g[1]), ("random", g[2], P.inverse(g[3])), ("random", g[4], g[5]), ("squaring", g[0], g[0]),
                 ("inverse", g[1], P.inverse(g[1])), ("f power", g[0], f), ("f power", f2, g[1]), ("f power", fk, g[2]),
                 ("f power", fk, P.inverse(f2))]
        for kind, x, y in pairs:
            if x.a == y.a:
                y = P.Form(y.c, -y.b, y.a)
            if x.a < y.a:
                x, y = y, x
            if x.a.bit_length() <= 32 or y.c.bit_length() > 1280 or x.a.bit_length() > 1280:
                continue
            y1, gcd = _bezout(x.a, y.a)
            m = (x.b - y.b) // 2
            if gcd != 1 or abs(m).bit_length() > 1280:
                continue
            for yy in (y1, y1 - x.a if y1 > 0 else y1 + x.a):
                assert abs(yy) < x.a and (yy * y.a) % x.a == 1
                out.append(("%s %s" % (name, kind), (yy, m, x.a)))
    # synthetic: the largest magnitudes of 1044-bit operands, a zero product, a product below the divisor, a multiple
    big = (1 << 1044) - 1
    out += [("largest", (big - 1, -(big - 2), big)), ("largest", (-(big - 1), -big, big)), ("zero", (0, 12345, big)),
            ("small", (3, -5, big)), ("multiple", (-(big - 4), 0, big - 4)), ("multiple", ((1 << 600) + 1, -((1 << 444) - 1) , ((1 << 600) + 1)))]
    _steps = out
    return out


def step_expected(case):
    y1, m, a1 = case
    return (y1 * m) % a1


def pack_step(case):
    y1, m, a1 = case
    sg = np.array([(1 if y1 < 0 else 0) | (2 if m < 0 else 0)], dtype=np.uint32)
    return np.concatenate([S.to_limbs(abs(y1), 40), S.to_limbs(abs(m), 40), S.to_limbs(a1, 40), sg])


REQUIRED = ("num below den", "remainder zero", "den bits 0 mod 32", "den bits 31 mod 32", "den 33 bits", "den 1279 bits", "empty top plane",
            "largest product", "add-back family", "limb 1 all ones, lane 3", "zero limbs in the remainder")
STEP_KINDS = ("random", "squaring", "inverse", "f power")
