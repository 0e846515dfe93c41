"""Case lists of the device arithmetic primitives (cofhe_amd/csrc/{lane,mp,wide}.hpp) as plain Python integers, shared by
the CPU tier (the host simulators, tests/test_hostsim_device_code.py and tests/test_hostsim_wide.py) and the GPU tier (the
primitive harness, tests/test_gpu_prims.py).  The lists that lived inside the CPU tests keep their seeds and their order;
the families added below them are the routes random operands do not reach: the add-back of the long divisions, the carry
chain at its bounds, the hand-overs of the carry resolve, bit positions at lane and plane edges, and the row edges of the
wavefront-wide layout.  Nothing here touches a library: every function returns integers.  TEST INFRASTRUCTURE."""
import os
import random
import sys

M1 = 1 << 1280            # one plane
M2 = 1 << 2560            # two planes
MW = 1 << 4096            # the wide layout's capacity
ONES = 0xFFFFFFFF
ST_DIV_CAP = 4            # lane.hpp: CF_ST_DIV_CAP


def rnd(rng, bits):
    return rng.getrandbits(bits) if bits else 0


def _pyref():
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
    import pyref
    return pyref


# ------------------------------------------------------------------------------------------------ moved from the CPU tests
def mul_cases():
    """test_mul: (xs, ys) for <1,1> and (xs2, ys2) for <2,1>"""
    rng = random.Random(1)
    sizes = [1, 31, 32, 33, 160, 161, 640, 1044, 1279, 1280]
    xs = [rnd(rng, rng.choice(sizes)) for _ in range(24)] + [0, 1, (1 << 1280) - 1]
    ys = [rnd(rng, rng.choice(sizes)) for _ in range(24)] + [(1 << 1280) - 1, 0, (1 << 1280) - 1]
    xs2 = [rnd(rng, rng.choice([2086, 2560, 1300, 5])) for _ in range(10)] + [(1 << 2560) - 1]
    ys2 = [rnd(rng, rng.choice([1044, 1280, 17, 522])) for _ in range(10)] + [(1 << 1280) - 1]
    # lane and plane edges of both operands, all-ones chunks (every hand-over word of the product at its largest)
    e = [160, 161, 1120, 1121, 1279, 1280]
    xs += [(1 << b) - 1 for b in e] + [1 << (b - 1) for b in e]
    ys += [(1 << b) - 1 for b in reversed(e)] + [(1 << b) - 1 for b in e]
    xs2 += [(1 << b) - 1 for b in (1280, 1281, 2400, 2559)] + [1 << 2559, 1 << 1280]
    ys2 += [(1 << b) - 1 for b in (1280, 1279, 160, 1)] + [(1 << 1280) - 1, 1 << 1279]
    return xs, ys, xs2, ys2


def lincomb_shift_cases():
    """test_lincomb_shift_bitlen: linear combinations as (A, B, x, y) and shifts as (sh, value)"""
    rng = random.Random(2)
    n = 12
    xs = [rnd(rng, 2500) for _ in range(n)]
    ys = [rnd(rng, 2400) for _ in range(n)]
    lin = [(A, B, x, y) for A, B in [(0x7FFFFFFF, 12345), (1, 0x7FFFFFFF), (65535, 1)] for x, y in zip(xs, ys)]
    shifts = []
    for sh in [0, 1, 31, 32, 33, 160, 161, 1279, 1280, 1281, 2000]:
        vals = [rnd(rng, b) for b in (2560, 100, 1280)] + [0, 1, M2 - 1]
        shifts += [(sh, v) for v in vals]
    return lin, shifts


def carry_ripple_operands():
    """test_carry_ripples_across_lanes: long carry / borrow runs, and the pat(...) operands of the sparse resolve"""
    xs = [(1 << 1600) - 1, (1 << 2560) - 1, (1 << 160) - 1, (1 << 1600), (1 << 2400), ((1 << 800) - 1) << 160, (1 << 2559) + (1 << 32) - 1,
          (1 << 1280) - 1, 1 << 1280]
    ys = [1, 1, (1 << 32) - 1, 1, (1 << 161) + 1, 1 << 160, 1, 1, 1]
    # the sparse resolve of sums (mp_resolve_sparse): a word handed over into an all-ones limb 0 next to a limb 1 that is
    # NOT all ones (fast path: the carry stops in limb 1) although limbs 2-4 are; then the same with limb 1 all ones in one
    # lane only (fallback to the general resolve for the whole wavefront)
    pat = lambda l1: sum(((0xFFFFFFFF if i % 5 != 1 else l1(i)) << (32 * i)) for i in range(80))
    top = sum(1 << (32 * i) for i in range(80) if i % 5 == 4)
    xs += [pat(lambda i: 5), pat(lambda i: 0xFFFFFFFF if i == 16 else 7), pat(lambda i: 0xFFFFFFFE)]
    ys += [top, top, top | 1]
    return xs, ys


def carry_ripple_cases():
    xs, ys = carry_ripple_operands()
    return [(A, B, x, y) for A, B in [(1, 1), (3, 1), (1, 0x7FFFFFFF), (0x3FFFFFF, 0x3FFFFFF)] for x, y in zip(xs, ys)]


def divexact_cases():
    """test_divexact: (num, den, quotient) and the quotient limbs asked for"""
    rng = random.Random(33)
    cases = []
    for _ in range(40):
        db = rng.choice([1044, 1280, 522, 33, 32, 31, 1, 64, 700, 1043])
        qb = rng.choice([0, 1, 31, 32, 33, 522, 544, 545, 1044, 1279])
        d = max(1, rnd(rng, db)) | (1 << (db - 1))
        if rng.random() < 0.5:
            d = (d >> rng.choice([1, 2, 5, 31])) << rng.choice([1, 2, 5, 31])      # even divisors
            d = max(d, 2)
        q = rnd(rng, qb)
        if (d * q).bit_length() > 2560:
            continue
        cases.append((d * q, d, q))
    cases += [(0, 12345, 0), (7 << 40, 7 << 35, 32), ((1 << 1279) * 3, 3, 1 << 1279), ((1 << 64) * 5, 1 << 64, 5), (1 << 2000, 1 << 1000, 1 << 1000)]
    # the two-digits-per-pass loop (one carry resolve per pair, pending words fed into the second chain): quotients and
    # divisors of all-ones / sparse limbs (every hand-over word and ripple at its largest), divisors whose second limb is 0 or
    # all ones (the 64-bit inverse), 31 trailing zero bits, odd and even digit counts, numerators that fill both planes
    for _ in range(300):
        db = rng.choice([1044, 1043, 1280, 1100, 65, 64, 63, 97, 160, 161, 320])
        d = rnd(rng, db) | (1 << (db - 1)) | 1
        kind = rng.randrange(6)
        if kind == 0:
            d = (1 << db) - 1
        elif kind == 1:
            d = (d >> 64 << 64) | (0xFFFFFFFF << 32) | (d & 0xFFFFFFFF) | 1
        elif kind == 2:
            d = (d >> 64 << 64) | (d & 0xFFFFFFFF) | 1                          # second limb zero
        elif kind == 3:
            d = ((d >> 31) << 31) | (1 << 31) if db > 40 else d                 # 31 trailing zero bits
        qb = rng.choice([1, 32, 33, 63, 64, 65, 95, 96, 97, 522, 544, 545, 576, 1044, 1056, 1216, 1279])
        q = rnd(rng, qb) | (1 << (qb - 1))
        if rng.random() < 0.3:
            q = (1 << qb) - 1
        elif rng.random() < 0.2:
            q = sum(1 << (32 * t_) for t_ in range(0, (qb + 31) // 32, 2)) % (1 << qb) or 1
        if (d * q).bit_length() > 2560 - 2:
            continue
        cases.append((d * q, d, q))
    nq = [(q.bit_length() + 31) // 32 + (i % 3) for i, (_, _, q) in enumerate(cases)]
    return cases, nq


def divrem_xgcd_cases():
    """test_divrem_and_xgcd: the random family (nums, dens) of the <2,1> division and the operands (xa, ya) of the xgcd"""
    rng = random.Random(3)
    nums = [rnd(rng, rng.choice([2088, 2560, 1566, 1044, 64, 40, 2000])) for _ in range(24)] + [0, 5, M2 - 1, M2 - 1, 1 << 2559]
    dens = [max(1, rnd(rng, rng.choice([1044, 1280, 522, 33, 32, 31, 1, 64, 700]))) for _ in range(24)] + [7, 7, 1, (1 << 1280) - 1, 3]
    xa = [rnd(rng, 1044) | 1 for _ in range(10)] + [rnd(rng, 1280) for _ in range(3)] + [12, 1 << 1000, 5, 1, 6 << 700]
    ya = [rnd(rng, 1040) for _ in range(10)] + [rnd(rng, 600) for _ in range(3)] + [18, 3, 5, 1, 9 << 650]
    xa, ya = [max(a, b) for a, b in zip(xa, ya)], [min(a, b) for a, b in zip(xa, ya)]
    return nums, dens, xa, ya


def word_route_cases():
    """test_word_route_primitives: moduli and numbers of mp_mod_word_fast, numbers of mp_mod_primorial, pairs of word_xgcd16"""
    rng = _pyref().SplitMix64(616)
    ds = [2, 3, 29, 31, 255, 256, 257, 4099, 32749, 65521, 65535] + [2 + rng.below(65534) for _ in range(40)]
    Ws = [d_ * d_ for d_ in ds] + [1, 2, 3, 0xFFFFFFFF, 0xFFFFFFFB, 0x80000000, 0x10001] + [1 + rng.below(0xFFFFFFFF) for _ in range(40)]
    Ws = [w for w in Ws if 0 < w < (1 << 32)]
    xs = []
    for i, w in enumerate(Ws):
        kind = i % 4
        if kind == 0:
            x = rng.bits(2560)
        elif kind == 1:
            x = (1 << 2560) - 1 - rng.bits(40)
        elif kind == 2:
            x = sum(1 << (32 * rng.below(80)) for _ in range(3)) * (1 + rng.below(1 << 16))
            x %= 1 << 2560
        else:
            x = rng.bits(1044)
        xs.append(x)
    # mp_mod_primorial: the constant modulus 2*3*...*23 of the coprime-representative test (tabulated limb weights)
    M = 223092870
    ps = [0, 1, M - 1, M, M + 1, (1 << 1280) - 1, (1 << 1279), (1 << 1043) - 1] + [rng.bits(1280) for _ in range(40)] + \
         [rng.bits(1044) for _ in range(40)] + [M * rng.bits(1200) for _ in range(8)] + [sum(0xFFFFFFFF << (32 * i) for i in range(0, 40, 3))]
    ms, as_ = [], []
    for m_ in [2, 3, 4, 29, 30, 841, 65521, 65535, 46368, 28657] + [2 + rng.below(65534) for _ in range(300)]:
        for a_ in {1, m_ - 1, max(1, m_ // 2), 1 + rng.below(m_ - 1), 1 + rng.below(m_ - 1)}:
            if 0 < a_ < m_:
                ms.append(m_)
                as_.append(a_)
    ms += [46368, 65535, 65534]            # consecutive Fibonacci numbers: the longest remainder sequences of 16-bit operands
    as_ += [28657, 65534, 65533]
    return Ws, xs, ps, ms, as_


def euclid_wg_cases(n):
    """test_euclid_wg_cofactors_and_stops: full sequences (x, y) and partial ones (x, y, stop); n = groups of the workgroup
    (2 n partial sequences)"""
    rng = random.Random(31)
    full, part = [], []
    for bits in (33, 64, 65, 96, 200, 500, 1043, 1044, 1171, 1200):
        for _ in range(2):
            a = rnd(rng, bits) | (1 << (bits - 1))
            full.append((a, rnd(rng, bits - 1) | 1))
    a0 = rnd(rng, 1043) | (1 << 1042)
    full += [(a0, 3), (a0, 5), (a0, 1 << 200), (a0, (1 << 252)), (a0, rnd(rng, 700) | 1), (a0, a0), (a0, 0), (a0, 1), (a0, a0 - 1),
             (6 * (rnd(rng, 500) | 1), 10 * (rnd(rng, 480) | 1))]
    for _ in range(2 * n):
        a = rnd(rng, 1043) | (1 << 1042)
        b = rnd(rng, 1041)
        part.append((a, b, rng.choice([530, 521, 700, 64, 1000, 33])))
    return full, part


def wide_mul_lincomb_shift_cases():
    """test_wide_mul_lincomb_shift: products (xs, ys), linear combinations (A, B, x, y), shifts (sh, value), comparisons"""
    rng = random.Random(5)
    xs = [rnd(rng, rng.choice([1, 31, 32, 33, 64, 65, 522, 1044, 1056, 2088, 2112])) for _ in range(60)] + [0, 1, (1 << 2112) - 1, (1 << 1056) - 1]
    ys = [rnd(rng, rng.choice([1, 31, 32, 33, 64, 65, 522, 1044, 1056, 1984])) for _ in range(60)] + [5, 0, (1 << 1984) - 1, (1 << 1056) - 1]
    # linear combinations: the two's complement over the whole capacity (long runs of all-ones limbs: every carry ripple the
    # generate / propagate ballots have to carry across lanes), all-ones operands, the widest multipliers
    lx = [rnd(rng, rng.choice([4000, 2000, 1044, 64, 63])) for _ in range(40)] + [MW - 1, (1 << 1600) - 1, 1 << 3000]
    ly = [rnd(rng, rng.choice([3990, 1990, 1040, 60, 5])) for _ in range(40)] + [1, 1, 1]
    lin = [(A, B, x, y) for A, B in [(1, 1), (0x3FFFFFF, 0x3FFFFFF), (1, 0xFFFFFFFF), (65535, 3)] for x, y in zip(lx, ly)]
    vals = [rnd(rng, 4096), rnd(rng, 100), rnd(rng, 1280), 0, 1, MW - 1, rnd(rng, 2100)]
    shifts = [(sh, v) for sh in [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 160, 1279, 2000, 4095] for v in vals]
    cmps = [(5, 7), (7, 5), (1 << 4000, 1 << 4000), ((1 << 2000) + 1, 1 << 2000), (0, 0), (0, 1)]
    return xs, ys, lin, shifts, cmps


def wide_euclid_cases():
    """test_wide_remainder_sequence: (x, y, stop)"""
    rng = random.Random(31)
    cases = []
    for bits in (1200, 1279, 640, 130, 129, 128, 127, 65, 64, 63, 33, 20):
        for _ in range(6):
            x = rnd(rng, bits) | (1 << (bits - 1))
            cases.append((x, rnd(rng, bits), -1))
            cases.append((x, rnd(rng, max(1, bits - rng.randrange(1, 40))), -1))
            cases.append((x, rnd(rng, bits), bits // 2))
            cases.append((x, rnd(rng, bits) | 1, bits // 2 + rng.randrange(-8, 8)))
    for gap in (27, 53, 64, 65, 127, 128, 129, 200, 640, 1100):          # far apart: long-division steps, empty views
        x = rnd(rng, 1200) | (1 << 1199)
        cases.append((x, rnd(rng, 1200 - gap) | 1, -1))
        cases.append((rnd(rng, 1200 - gap) | 1, x, -1))
        cases.append((x, rnd(rng, 1200 - gap) | 1, 600))
    x = rnd(rng, 900) | 1
    cases += [(x, x, -1), (x, 0, -1), (0, x, -1), (1 << 1000, 1 << 500, -1), ((1 << 1000) - 1, (1 << 64) - 1, -1), (x, 1, -1), (1, 1, -1),
              (x * 7, x * 3, -1), ((1 << 64), (1 << 64) - 1, -1), ((1 << 128) + 1, (1 << 64) + 1, 40), (x << 130, x << 129, -1)]
    return cases


def wide_division_cases():
    """test_wide_divisions: (num, den) of w_mod and (num, den, quotient), quotient lanes asked for, of w_divexact"""
    rng = random.Random(6)
    mods = []
    for _ in range(200):
        db = rng.choice([1044, 1043, 1056, 1024, 1025, 65, 64, 33, 32, 31, 1, 700])
        nb = rng.choice([2088, 2080, 1044, 1500, db, db + 1, db + 31, db + 32, db + 33, 10, 0])
        d = rnd(rng, db) | (1 << (db - 1))
        n = rnd(rng, nb)
        k = rng.randrange(5)
        if k == 0:
            d = (1 << db) - 1
        if k == 1:
            n = d * rnd(rng, max(nb - db, 1)) + (d - 1)           # remainders at the top of their range
        if k == 2:
            n = d * rnd(rng, max(nb - db, 1))                     # and zero
        if n.bit_length() <= 2200:
            mods.append((n, d))
    mods += [(5, 7), ((1 << 2088) - 1, (1 << 1044) - 1), (1 << 1044, 1 << 1043), (1 << 2000, (1 << 1000) + 1)]
    # exact division, 2-adic with 64-bit digits
    exact = []
    for _ in range(250):
        db = rng.choice([1044, 1043, 1280, 65, 64, 63, 97, 160, 33, 32, 1])
        qb = rng.choice([1, 32, 33, 63, 64, 65, 522, 544, 576, 1044, 1056, 1279])
        d = rnd(rng, db) | (1 << (db - 1))
        k = rng.randrange(6)
        if k == 0:
            d = (1 << db) - 1
        if k == 1:
            d = (d >> rng.choice([1, 5, 31, 40])) << rng.choice([1, 5, 31, 40]) or 2          # even divisors (< 64 trailing zeros)
        q = rnd(rng, qb) | (1 << (qb - 1))
        if rng.random() < 0.3:
            q = (1 << qb) - 1
        if (d * q).bit_length() <= 3900 and (d & ((1 << 64) - 1)):
            exact.append((d * q, d, q))
    nq = [(c[2].bit_length() + 63) // 64 + (i % 3) for i, c in enumerate(exact)]
    # the add-back of w_mod (remainder den - 1: the digit estimate lands one above), divisors whose leading limbs are
    # 0x80000000:00000000 followed by all ones, and all ones
    mods += [(n, d) for n, d, _q in divrem_addback_cases(2200, [33, 64, 65, 522, 1043, 1044], [1, 31, 32, 33, 64, 65, 544, 1044], seed=61)]
    return mods, exact, nq


# ------------------------------------------------------------------------------------------------ new families
DEN_BITS_1 = [33, 64, 65, 522, 1043, 1044, 1279, 1280]          # single-plane divisors
DEN_BITS_2 = [1281, 1300, 1344, 1345, 1600, 1999, 2000]         # divisors that need the second plane (the PD = 2 loop)
QUOT_BITS = [1, 31, 32, 33, 64, 65, 544, 1044]


def special_dens(rng, db):
    """divisors of db bits: random, leading 64 bits 0x80000000:00000000 followed by all ones, all ones (0xFFFFFFFF:FFFFFFFF)"""
    dens = [rnd(rng, db) | (1 << (db - 1)), (1 << db) - 1]
    if db > 64:
        dens.append((1 << (db - 1)) | ((1 << (db - 64)) - 1))
    return dens


def divrem_addback_cases(cap_bits, den_bits, quot_bits=QUOT_BITS, seed=8):
    """(num, den, family) with num = den Q - 1 (family 0) and num = den Q + den - 1 (family 1): the remainder is den - 1,
    so every 32-bit digit estimate that is rounded up lands one above the true digit and the add-back runs.  cap_bits:
    numerators stay below 2^cap_bits (the headroom mp.hpp states for mp_divrem: the top bit of the PN-plane window clear)"""
    rng = random.Random(seed)
    out = []
    for db in den_bits:
        for qb in quot_bits:
            Q = rnd(rng, qb) | (1 << (qb - 1))
            for den in special_dens(rng, db):
                for fam, num in ((0, den * Q - 1), (1, den * Q + den - 1)):
                    if num.bit_length() <= cap_bits:
                        out.append((num, den, fam))
    return out


def divrem_edge_cases(cap_bits, den_bits, seed=9):
    """num < den, num == den, num == 0 for every divisor length; no add-back expected here"""
    rng = random.Random(seed)
    out = []
    for db in den_bits:
        den = rnd(rng, db) | (1 << (db - 1))
        out += [(den - 1, den), (den, den), (0, den), (rnd(rng, db - 1), den)]
    return [(n, d) for n, d in out if n.bit_length() <= cap_bits]


def divrem_cases(pn, pd):
    """(add-back family, everything else) for the <pn, pd> instantiation of mp_divrem; numerators below 2^(1280 pn - 1).
    Word-sized divisors (mp_divrem_word) and, for pd = 2, divisors below 64 bits (mp_divrem_cons) are in the second list."""
    cap = 1280 * pn - 1
    dens = DEN_BITS_1 + (DEN_BITS_2 if pd == 2 else [])
    addback = divrem_addback_cases(cap, dens, seed=8 + 16 * pn + pd)
    rng = random.Random(90 + 16 * pn + pd)
    rest = divrem_edge_cases(cap, dens + [1, 31, 32, 40, 63])
    for db in (1, 2, 31, 32, 33, 40, 63):                       # the word route and (pd = 2) the conservative digits
        for nb in (db, db + 1, 64, 65, 700, cap):
            den = rnd(rng, db) | (1 << (db - 1))
            rest += [(rnd(rng, nb), den), (den * (rnd(rng, max(nb - db, 1)) + 1) - 1, den)]
    if pn == 2 and pd == 1:
        nums, dens_, _, _ = divrem_xgcd_cases()
        rest = list(zip(nums, dens_)) + rest                    # the CPU test's own list (it goes to the top of the window)
    rest = [(n, d) for n, d in rest if n.bit_length() <= (2560 if (pn == 2 and pd == 1) else cap)]
    return addback, rest


def lincomb_bound_cases():
    """(A, B, x, y): the carry chain of lincomb_plane with every h_j and every carry at its maximum (all-ones operands, A + B
    at 2^32), the subtracting form kept at A x >= B y (y shortened or zero where B > A); then the resolve hand-overs: sums
    that carry out of the top plane, a word handed from lane 7 of plane 0 into an all-ones lane 0 of plane 1, 2^2560 - 1 + 1"""
    full = M2 - 1
    out = []
    for A, B in [(0xFFFFFFFF, 1), (1, 0xFFFFFFFF), (0x80000000, 0x80000000), (1, 0), (0, 1)]:
        out.append((A, B, full, full))                              # the sum at its largest (the difference wraps: A x < B y for B > A)
        if A >= B:
            out += [(A, B, full, full - 1), (A, B, full, M1 - 1), (A, B, M1 - 1, (1 << 1279) - 1)]
        elif A:
            out += [(A, B, full, (1 << 2528) - 1), (A, B, full, (1 << 1248) - 1), (A, B, M1 - 1, (1 << 160) - 1)]
        else:
            out += [(A, B, full, 0), (A, B, 0, 0)]
    lane = (1 << 160) - 1
    out += [
        (1, 1, full, 1), (1, 1, full, full), (1, 1, 1 << 2559, 1 << 2559), (1, 1, full - 5, 6),       # the carry leaves the top plane
        (1, 1, (lane << 1120) | (lane << 1280), 1 << 1120),           # word 1 from lane 7 of plane 0 into an all-ones lane 0 of plane 1
        (3, 1, (lane << 1120) | ((lane // 3) << 1280), 0),            # word 2 into A x's all-ones chunk
        (0xFFFFFFFF, 1, (lane << 1120) | ((lane // 0xFFFFFFFF) << 1280), (lane % 0xFFFFFFFF) << 1280),
        (1, 1, (M1 - 1) << 160, 1 << 160), (1, 1, M1 - 1, 1), (1, 1, (full >> 160) << 160, 1 << 160),
        (2, 2, full, full), (0x7FFFFFFF, 0x7FFFFFFF, full, full),
    ]
    return out


EDGE_BITS = [0, 1, 31, 32, 33, 159, 160, 161, 1279, 1280, 1281, 2559]


def shift_edge_cases():
    """(sh, value): lengths and shift amounts at limb, lane (160) and plane (1280) edges"""
    rng = random.Random(44)
    vals = []
    for L in EDGE_BITS + [2560]:
        vals += [(1 << L) - 1, (1 << L) >> 1, rnd(rng, L) | ((1 << L) >> 1)]
    vals = sorted(set(vals))
    return [(sh, v) for sh in EDGE_BITS for v in vals]


def bits_cases():
    """(x, y, pos, idx) for mp_cmp(x, y), mp_bits64(x, pos), mp_bits32(x, pos), mp_get_limb(x, idx): windows whose three limbs
    straddle a lane edge (limbs 4|5) and the plane edge (limbs 39|40), and the top of the number; operands that differ in
    one limb at those edges"""
    rng = random.Random(45)
    out = []
    xs = [rnd(rng, 2560), M2 - 1, sum((i + 1) << (32 * i) for i in range(80))]
    for x in xs:
        for i0 in (0, 3, 4, 5, 33, 34, 35, 37, 38, 39, 40, 44, 45, 77, 78, 79):
            for o in (0, 1, 31):
                out.append((x, x ^ (1 << (32 * i0 + o)), 32 * i0 + o, i0))
    x = xs[0]
    out += [(x, x, 0, 80), (0, 0, 5, -1), (x, x + 1 if x + 1 < M2 else x - 1, 2559, 79), (1 << 1280, (1 << 1280) - 1, 1279, 40),
            ((1 << 1280) - 1, 1 << 1280, 1248, 39), (1 << 160, (1 << 160) - 1, 159, 5), (1, 0, 0, 0), (0, 1, 0, 0)]
    return out


def wide_lincomb_edge_cases():
    """(A, B, x, y) on the wide layout: 2^4096 - 1 + 1, 2^4096 - 1 - x, hand-over words and propagate runs that cross the row
    edges of the wavefront (lanes 15|16, 31|32, 47|48: bits 1024, 2048, 3072), where wave_shr differs from row_shr"""
    rng = random.Random(46)
    full = MW - 1
    out = [(1, 1, full, 1), (1, 1, full, full), (1, 1, full, rnd(rng, 4096)), (1, 1, full, rnd(rng, 2000)), (1, 1, full, 0),
           (0xFFFFFFFF, 1, full, full), (1, 0xFFFFFFFF, full, (1 << 4064) - 1), (0x80000000, 0x80000000, full, full), (1, 0, full, full),
           (0, 1, 0, 0), (0, 1, full, full)]
    w64 = (1 << 64) - 1
    for e in (1024, 2048, 3072):
        for below, above in ((1, 1), (2, 3), (15, 17)):
            run = (((1 << (64 * (below + above))) - 1) << (e - 64 * below)) & full     # all ones from `below` lanes under the edge to `above` over it
            out += [(1, 1, run, 1 << (e - 64 * below)), (1, 1, run | 1, run), (1, 1, 1 << min(e + 64 * above, 4095), 1 << (e - 64 * below)),
                    (1, 1, run, 1)]
        # a word leaves the lane under the edge and lands in an all-ones lane above it
        out += [(3, 1, (w64 << (e - 64)) | ((w64 // 3) << e), 0),
                (0xFFFFFFFF, 1, (w64 << (e - 64)) | ((w64 // 0xFFFFFFFF) << e), (w64 % 0xFFFFFFFF) << e),
                (0x80000000, 0x80000000, w64 << (e - 64), (w64 << (e - 64)) | (w64 << e))]
    return out


WIDE_SHIFTS = [0, 1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049, 4064, 4095]


def wide_shift_edge_cases():
    """(sh, value): even and odd limb counts, the row edges, the top of the capacity"""
    rng = random.Random(47)
    vals = [MW - 1, 1, 1 << 4095, rnd(rng, 4096), rnd(rng, 2049), sum((i + 1) << (32 * i) for i in range(128)), (1 << 1024) - 1, 1 << 2048]
    return [(sh, v) for sh in WIDE_SHIFTS for v in vals]


# ------------------------------------------------------------------------------------------------ models
def staged_loop_overshoots(num, den):
    """the digit estimate of mp_divrem's staged-divisor loop (mp.hpp, PD = 2, divisors of 64 bits and more) restated in
    Python floats (IEEE double, as on the device): the f64 quotient of the 96-bit remainder window by the leading 64 bits
    of the divisor, times (1 + 2^-49), truncated.  Returns how many digits came out above the true digit (each one an
    add-back on the device), or None when the routine does not reach the loop."""
    db, nb = den.bit_length(), num.bit_length()
    if db < 64 or nb < db:
        return None
    rd = 1.0 / float(den >> (db - 64))
    over = 0
    for jq in range((nb - db) // 32, -1, -1):
        pos = db - 64 + 32 * jq
        hi64, lo32 = (num >> (pos + 32)) & ((1 << 64) - 1), (num >> pos) & ONES
        x = (float(hi64) * 4294967296.0 + float(lo32)) * rd
        x += x * 1.7763568394002505e-15
        qd = min(int(x), ONES)
        true = num // (den << (32 * jq))
        assert true <= qd <= true + 4, "estimate outside the add-back's reach"
        over += qd > true
        num -= true * (den << (32 * jq))
    return over
