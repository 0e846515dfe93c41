"""Case lists of the paired 2-adic division (cofhe_amd/csrc/mp.hpp: mp_resolve_pair, mp_divexact_pair; qf.hpp:
m12_low_quot_pair), of mp_divexact with a one-plane numerator (no high-limb bookkeeping) and of mp_sqr_low (every chunk pair
once) as plain Python integers, shared by the CPU tier (tests/test_pairdiv_cpu.py on the host simulator) and the GPU tier
(tests/test_gpu_pairdiv.py on tests/gpu_kernels/pairdiv_gpu.hip).  The whole compositions through nucomp_m12, nucomp_ab and
nucomp_c come from the generators of lowmul_cases.py and onep_cases.py.  Nothing here touches a library.

A "pair" is one plane of 40 limbs that holds a value modulo 2^640 in limbs 0..19 (lanes 0..3 of the group) and another in
limbs 20..39 (lanes 4..7).

The models, from the definitions and not from the code:
  mp_divexact_pair(num, den, nq): half h of the result is ((n_h >> tz) * (den >> tz)^-1) mod 2^(32 nq), tz = the trailing zero
    bits of den (< 32), n_h >> tz with zeros shifted in at bit 640.
  m12_low_quot_pair(pa, pb, sub0, sub1, v1, nb0, nb1): half h is the two's-complement value of nb_h + 1 bits of
    (((pa_h +- pb_h) mod 2^640) >> tz) * (v1 >> tz)^-1, as sign and magnitude; zero for nb_h < 0.  Where the case was made
    from an exact quotient M with |M| < 2^nb and nb + 1 + tz <= 640 that value is M, which is asserted when the case is made.
  mp_divexact<1, 1>(num, den, q, nq): q = ((num >> tz) * (den >> tz)^-1) mod 2^(32 nq), limbs from nq on zero.
TEST INFRASTRUCTURE."""
import random

import numpy as np

import lowmul_cases as LC
import onep_cases as OC
import simlib as S
from lowmul_cases import tz

HALF = 1 << 640
PLANE = 1 << 1280
ONES = HALF - 1
DIVP_IN, DIVP_OUT, QUOTP_IN, QUOTP_OUT, DIVX_IN, DIVX_OUT, SQR_IN, SQR_OUT = 81, 40, 124, 42, 81, 40, 40, 40


def _odd(rng, bits):
    return rng.getrandbits(bits) | (1 << (bits - 1)) | 1


def signed(v, bits):
    """the two's-complement value of the low `bits` bits of v"""
    v %= 1 << bits
    return v - (1 << bits) if v >> (bits - 1) else v


def nq_of(nb):
    return 0 if nb < 0 else (nb + 32) >> 5


# ---------------------------------------------------------------------------- mp_divexact_pair
def divp_expected(case):
    n0, n1, den, nq = case
    t = tz(den)
    inv = pow(den >> t, -1, 1 << (32 * nq)) if nq else 0
    q = [((n >> t) * inv) % (1 << (32 * nq)) if nq else 0 for n in (n0, n1)]
    return S.to_limbs(q[0] | (q[1] << 640), 40)


def divp_cases():
    """(n0, n1, den, nq): den a plane with a non-zero limb 0"""
    rng = random.Random(1700)
    out = []
    for nq in (1, 2, 3, 7, 10, 19, 20):
        for t in (0, 1, 31):
            out.append((rng.getrandbits(640), rng.getrandbits(640), _odd(rng, 1044 - t) << t, nq))
    den = _odd(rng, 1044)
    # chunk 3 of half 0 all ones under digits whose products carry out of it; half 1 a small exact multiple, then zero: nothing
    # that leaves half 0 may show in half 1
    for top in (ONES, (ONES >> 480) << 480, ((ONES >> 480) << 480) | rng.getrandbits(480)):
        out.append((top, (5 * den) % HALF, den, 20))
        out.append((top, 0, den, 20))
        out.append((top, top, den | (ONES << 640), 20))
    # all-ones halves against a divisor of all ones (every digit's product is a long run), and unit divisors
    out += [(ONES, ONES, PLANE - 1, 20), (ONES, 0, 1, 20), (0, ONES, 1, 19), (ONES, ONES, 3, 20), (1, ONES, ONES, 20), (0, 0, den, 20)]
    # quotients that are runs of ones and zeros: every pass subtracts into all-ones limbs (the propagate chain of the resolve)
    for q in (ONES, 1 << 639, (1 << 320) - 1, ONES - ((1 << 160) - 1), ((1 << 160) - 1) << 160):
        d = _odd(rng, 700)
        out.append(((q * d) % HALF, ((HALF - q) * d) % HALF, d, 20))
    return out


def pack_divp(case):
    n0, n1, den, nq = case
    return np.concatenate([S.to_limbs(n0 | (n1 << 640), 40), S.to_limbs(den, 40), np.array([nq], dtype=np.uint32)])


# ---------------------------------------------------------------------------- m12_low_quot_pair
def quotp_model(case):
    pa, pb, sub, v1, nb = case
    t = tz(v1)
    out = []
    for h in (0, 1):
        if nb[h] < 0:
            out.append(0)
            continue
        a, b = (pa >> (640 * h)) % HALF, (pb >> (640 * h)) % HALF
        n = ((a - b) if sub[h] else (a + b)) % HALF
        out.append(signed((n >> t) * pow(v1 >> t, -1, 1 << (nb[h] + 1)), nb[h] + 1))
    return tuple(out)


def quotp_make(rng, v1, M, nb, sub):
    """the case whose halves have the exact quotients M[h], |M[h]| < 2^nb[h]: first terms random, second terms what is left"""
    t = tz(v1)
    pa = pb = 0
    for h in (0, 1):
        assert (M[h] == 0 if nb[h] < 0 else abs(M[h]) < (1 << nb[h]) and nb[h] + 1 + t <= 640), (M[h], nb[h])
        a = rng.getrandbits(640)
        b = ((a - M[h] * v1) if sub[h] else (M[h] * v1 - a)) % HALF
        pa |= a << (640 * h)
        pb |= b << (640 * h)
    case = (pa, pb, tuple(sub), v1, tuple(nb))
    assert quotp_model(case) == tuple(M)
    return case


def quotp_cases():
    """[(name, case)], case = (pa, pb, (sub0, sub1), v1, (nb0, nb1))"""
    rng = random.Random(1701)
    out = []
    r = lambda nb: rng.getrandbits(nb) | (1 << (nb - 1)) if nb > 0 else 0

    def add(name, nb0, nb1, s0=1, s1=1, t=0, sub=(0, 1), M=None):
        v1 = _odd(rng, 1044 - t) << t
        M = M or (s0 * r(nb0), s1 * r(nb1))
        out.append((name, quotp_make(rng, v1, M, (nb0, nb1), sub)))

    # digit counts of the two halves: 1 and 20, 20 and 1, both odd, both even
    add("digits 1 20", 10, 639, 1, -1)
    add("digits 20 1", 639, 31, -1, 1)
    add("digits odd", 80, 200, 1, 1)                   # 3 and 7
    add("digits even", 100, 300, -1, -1)               # 4 and 10
    add("digits 1 1", 0, 5, 1, 1, M=(0, -17))
    # a zero quotient announced by its bound in one half only
    add("nb<0 half 0", -1, 500, 1, -1, M=(0, -r(500)))
    add("nb<0 half 1", 522, -3, -1, 1, M=(-r(522), 0))
    add("nb<0 both", -1, -1, M=(0, 0))
    # trailing zero bits of v1
    for t in (0, 31):
        add("tz%d" % t, 521, 522, 1, -1, t=t, sub=(1, 0))
        add("tz%d" % t, 608, 600, -1, 1, t=t, sub=(1, 1))
    # a negative quotient in one half only, with every choice of the subtraction flags
    for sub in ((0, 0), (0, 1), (1, 0), (1, 1)):
        add("neg half 0", 521, 522, -1, 1, sub=sub)
        add("neg half 1", 521, 522, 1, -1, sub=sub)
    # the sign bit at bit 0 and at bit 31 of its limb
    for nb in (512, 511, 32, 31):
        add("nb&31", nb, nb, -1, 1)
        add("nb&31", nb, 640 - 1 - nb if nb > 100 else 300, 1, -1)
    # nb + 1 + tz == 640, the largest and smallest values of that length, both signs
    for t in (0, 31):
        nb = 639 - t
        for M in (((1 << nb) - 1, -((1 << nb) - 1)), (-((1 << nb) - 1), 1 << (nb - 1)), (-(1 << (nb - 1)), (1 << nb) - 1), (1, -1)):
            add("edge640 tz%d" % t, nb, nb, t=t, M=M)
    return out


def quotp_raw_cases():
    """numerators given as they are (no exact quotient behind them): compared with the model alone"""
    rng = random.Random(1702)
    v1 = _odd(rng, 1044)
    top = (ONES >> 480) << 480
    out = []
    for sub in ((0, 0), (1, 1)):
        # chunk 3 of half 0 all ones, half 1 an exact small quotient
        b1 = ((7 * v1) % HALF - 12345) % HALF if not sub[1] else (12345 - 7 * v1) % HALF
        out.append(("chunk 3 ones", (top | rng.getrandbits(480) | (12345 << 640), 0 | (b1 << 640), sub, v1, (639, 3))))
        # a half whose limbs are all ones
        out.append(("all ones", (ONES | (rng.getrandbits(640) << 640), 0, sub, v1, (639, 639))))
        out.append(("all ones", (rng.getrandbits(640) | (ONES << 640), 0, sub, v1 | 1, (100, 639))))
        out.append(("all ones", (ONES | (ONES << 640), 0, sub, 1, (639, 639))))
    assert quotp_model(out[0][1])[1] == 7 and quotp_model(out[4][1])[1] == 7
    return out


def pack_quotp(case):
    pa, pb, sub, v1, nb = case
    tail = np.array([sub[0], sub[1], nb[0] & 0xFFFFFFFF, nb[1] & 0xFFFFFFFF], dtype=np.uint32)
    return np.concatenate([S.to_limbs(pa, 40), S.to_limbs(pb, 40), S.to_limbs(v1, 40), tail])


def unpack_quotp(rec):
    assert int(rec[40]) in (0, 1) and int(rec[41]) in (0, 1)
    m0, m1 = S.from_limbs(rec[:20]), S.from_limbs(rec[20:40])
    return (-m0 if rec[40] else m0), (-m1 if rec[41] else m1)


# ---------------------------------------------------------------------------- mp_divexact<1, 1>
def divx_expected(case):
    num, den, nq = case[:3]
    t = tz(den)
    return ((num >> t) * pow(den >> t, -1, 1 << (32 * nq))) % (1 << (32 * nq))


def divx_cases():
    """[(name, (num, den, nq, bits))]: the quotient is compared modulo 2^bits"""
    rng = random.Random(1703)
    out = []
    # exact numerators with quotients of 1, 2, 39 and 40 limbs, divisors with 0, 1 and 31 trailing zero bits
    for nq, qb, db in ((1, 32, 1248), (1, 1, 1279), (2, 64, 1216), (2, 33, 1000), (39, 1248, 32), (39, 1217, 40), (40, 1250, 30), (40, 1279, 1),
                       (17, 530, 700), (33, 1046, 230)):
        for t in (0, 1, 31):
            if db - t < 1:
                continue
            q, den = rng.getrandbits(qb) | (1 << (qb - 1)), _odd(rng, db - t) << t
            assert q * den < PLANE and (q.bit_length() + 31) // 32 == nq
            case = (q * den, den, nq, 32 * nq)
            assert divx_expected(case) == q
            out.append(("exact nq%d" % nq, case))
    # a numerator cut modulo 2^1280 whose quotient has nbc bits with nbc + 2 + tz == 1280 (the numerator of c' after its shift
    # by two: nbc + tz bits of it decide the quotient): compared modulo 2^nbc
    for t in (0, 5, 31):
        nbc = 1278 - t
        q, den = rng.getrandbits(nbc) | (1 << (nbc - 1)), _odd(rng, 1040 - t) << t
        out.append(("cut tz%d" % t, ((q * den) % PLANE, den, (nbc + 31) >> 5, nbc)))
        assert divx_expected(out[-1][1]) % (1 << nbc) == q
    # quotients of all ones: every pass leaves all-ones limbs behind
    for nq in (39, 40):
        q = (1 << (32 * nq - 8)) - 1
        out.append(("ones nq%d" % nq, (q * 255, 255, nq, 32 * nq)))
    return out


def pack_divx(case):
    return np.concatenate([S.to_limbs(case[0], 40), S.to_limbs(case[1], 40), np.array([case[2]], dtype=np.uint32)])


# ---------------------------------------------------------------------------- mp_sqr_low
def sqr_cases():
    rng = random.Random(1704)
    r = lambda b: rng.getrandbits(b) | (1 << (b - 1))
    cases = [r(160 * k) for k in range(1, 9)] + [r(160 * k - 159) for k in range(1, 9)]          # x of 1 to 8 chunks, full and barely
    cases += [PLANE - 1, 1 << 1279, r(1280), (1 << 1279) | 1]                                    # all ones; the top bit set
    cases += [1 << k for k in (0, 31, 32, 159, 160, 319, 320, 479, 480, 639, 640, 799, 800, 959, 960, 1119, 1120, 1279)]      # single bits
    c3, c7 = r(160) << 480, r(160) << 1120
    cases += [c3 | c7, c3, c7, (((1 << 160) - 1) << 480) | (((1 << 160) - 1) << 1120)]           # only chunks 3 and 7
    cases += [sum(((1 << 160) - 1) << (160 * k) for k in ks) for ks in ((0, 2, 4, 6), (1, 3, 5, 7), (0, 7), (3, 4))]
    return cases + OC.sqr_cases()


# ---------------------------------------------------------------------------- whole compositions
_comp = None


def composition_cases():
    """(m12, ab, c): [(name, case)] each, the operands of real compositions of the three committed parameter sets as
    lowmul_cases.py and onep_cases.py draw them: random pairs, squarings, inverse pairs and powers of f"""
    global _comp
    if _comp is None:
        ab = OC.ab_parameter_set_cases()
        c = []
        for name, case, D in ab:
            an, bn = OC.ab_expected(case)
            if 0 < an < PLANE and abs(bn) < PLANE:
                c.append((name, (an, abs(bn), D)))
        _comp = (LC.parameter_set_cases(), [(n, k) for n, k, _ in ab], c)
    return _comp
