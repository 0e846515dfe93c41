"""The form gate's case table, shared by the CPU tier (host simulator) and the GPU tier (k_validate_forms, the wire format).

The gate (qf.hpp: qf_form_faults) decides whether a record from outside may enter the arithmetic.  `clauses` restates it
over Python integers, one named boolean per clause; a record is valid iff all are true.  The table holds, for each of five
discriminants, records that must pass and forgeries that each NAME the one clause they are built to fail.

Two clauses cannot be isolated, by arithmetic and not by choice of cases:
  positive   a == 0 or c == 0 gives a c == 0 < (b^2 + |Delta|) / 4, so the equation fails with it (and c == 0 < a fails
             a <= c unless a == 0 too);
  no_carry   b^2 + |Delta| >= 2^2560 needs b^2 > 2^2560 - 2^2400; with |b| <= a <= c then 4 a c >= 4 b^2 > b^2 + |Delta|, so
             a record that fails no_carry also fails one of b_le_a, a_le_c, equation.
Their forgeries are listed in EXCEPTIONS with the further clauses they may fail; every other forgery fails exactly the
clause it names.  The simulator reports the failed clauses one bit each, so these two are still checked one by one there.
"""
import functools
import math
import os
import sys
from collections import namedtuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyref as P  # noqa: E402
from conftest import load_json  # noqa: E402

CLAUSES = ("sign_word", "positive", "b_le_a", "a_le_c", "edge_sign", "zero_sign", "no_carry", "low_bits", "equation", "primitive")
PLANE = 1 << 1280          # a and |b| are below it, c below its square
LANES, LANE_BITS = 8, 160  # a plane is 8 lanes of 5 limbs


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def clauses(a, b_mag, sign_word, c, D):
    """the gate over Python integers: D = |Delta|, the record is (a, |b|, sign word, c), any non-zero sign word reads as b < 0
    (as the arithmetic would read it).  `equation` is the comparison a 2560-bit adder sees; `no_carry` says that the adder
    lost nothing, `low_bits` that the division by four was exact: together they are b^2 + |Delta| == 4 a c."""
    neg = sign_word != 0
    s = b_mag * b_mag + D
    return {
        "sign_word": sign_word in (0, 1),
        "positive": a > 0 and c > 0,
        "b_le_a": b_mag <= a,
        "a_le_c": a <= c,
        "edge_sign": not (neg and b_mag != 0 and (b_mag == a or a == c)),
        "zero_sign": not (neg and b_mag == 0),
        "no_carry": s < PLANE * PLANE,
        "low_bits": s % 4 == 0,
        "equation": a * c == (s % (PLANE * PLANE)) // 4,
        "primitive": math.gcd(a, b_mag, c) == 1,
    }


def failed(rec, D):
    return frozenset(k for k, v in clauses(*rec, D).items() if not v)


def mask_of(names):
    """the simulator's verdict word for a set of failed clauses (qf.hpp: QF_BAD_*, in the order of CLAUSES)"""
    return sum(1 << CLAUSES.index(k) for k in names)


def valid(rec, D):
    return not failed(rec, D)


def expected_mask(case, D):
    """what the gate reports for a table record: the failed clauses of the reference (PARITY_INEXACT: without `primitive`)"""
    return mask_of(failed(case.rec, D) - ({"primitive"} if case.label in PARITY_INEXACT else set()))


def on_wire(rec):
    """whether the wire format can say this record at all: a sign flag, not a word; no minus zero (the flag on a zero is the
    reference's quirk and reads as zero); a and c positive and within their planes (the unpacker's own refusals otherwise)"""
    a, b, sw, c = rec
    return sw in (0, 1) and not (sw == 1 and b == 0) and 0 < a < PLANE and b < PLANE and 0 < c < PLANE * PLANE


def as_form(rec):
    a, b, sw, c = rec
    return P.Form(a, -b if sw else b, c)


# label -> the clauses a forgery may fail BESIDES the one it names (module docstring); there may be no others
EXCEPTIONS = {
    "a_zero": {"equation", "low_bits"},                # (0, 0, 1): b must be 0 to keep |b| <= a, so odd Delta fails low_bits too
    "c_zero": {"a_le_c", "equation"},
    "all_max": {"equation", "low_bits"},               # a = |b| = 2^1280 - 1, c = 2^2560 - 2: the carry out of b^2 + |Delta|
    "all_ones": {"equation", "low_bits", "primitive"},  # the same with c = 2^2560 - 1 = a (2^1280 + 1): content a, which is odd
}
# "not all even" is gcd == 1 for every record of the table but these (the table must not claim more than the gate checks):
# here the gate's parity clause holds although the content is not 1, and the expected verdict leaves `primitive` out
PARITY_INEXACT = {"all_ones"}

Case = namedtuple("Case", "label rec names")           # names: None for a record that must pass, else a clause
Disc = namedtuple("Disc", "name delta cases")


def rec_of(f, sign_word=None):
    return (f.a, abs(f.b), (1 if f.b < 0 else 0) if sign_word is None else sign_word, f.c)


def _first(cands, D, clause):
    """the first candidate record that fits the planes and fails exactly `clause` (a flipped bit may by chance give the three
    coefficients a common odd factor; such a candidate would claim more than the gate checks)"""
    for r in cands:
        if r[0] < PLANE and r[1] < PLANE and r[3] < PLANE * PLANE and failed(r, D) == {clause}:
            return r
    return None


def _lane_flips(x, lane, plane_bits=LANES * LANE_BITS, up=True, lo=1):
    """x with one bit of the given lane set (up) or cleared (down), at offsets lo.. of the lane, nearest first"""
    for off in range(lo, LANE_BITS):
        bit = 1 << (lane * LANE_BITS + off)
        if up and not x & bit:
            yield x | bit
        if not up and x & bit:
            yield x & ~bit


def _cases(delta, rng, extra_pass=(), owned=None):
    D = -delta
    out = []

    def ok(label, f):
        out.append(Case(label, rec_of(f) if isinstance(f, P.Form) else f, None))

    def bad(label, rec, names):
        out.append(Case(label, rec, names))

    big = D.bit_length() > 200
    g = []
    while len(g) < 3:
        f = P.random_form(delta, rng) if big else P.random_form(delta, rng, 12, 10)
        f = f if f.b > 0 else P.inverse(f)                            # b > 0, b < a < c: nothing at an edge
        # the first one carries the near misses: c + 1 and c - 1 must leave it primitive (a odd, for one)
        if 0 < f.b < f.a < f.c and (g or all(failed((f.a, f.b, 0, f.c + e), D) == {"equation"} for e in (1, -1))):
            g.append(f)
    for i, f in enumerate(g):
        ok("random%d" % i, f)
        ok("inverse%d" % i, P.Form(f.a, -f.b, f.c))
    ok("product", P.compose(g[0], g[1]))
    for label, f in extra_pass:
        ok(label, f)
    ident = P.identity(delta)
    ok("identity", ident)
    ell = 3
    while not (P.is_probable_prime(ell) and D % ell and P.jacobi(delta % ell, ell) == 1):
        ell += 2
    pf = P.prime_form(delta, ell)                                     # small a, c of nearly |Delta|'s length
    assert pf.a == ell
    ok("prime_form", pf)
    amb = None
    if D % 16 == 0:
        amb = P.Form(4, 4, 1 + D // 16)                               # b = +a
        ok("b_eq_a", amb)
    if owned:
        ok("a_eq_c", P.Form(owned[0], owned[1], owned[0]))

    g0 = rec_of(g[0])
    a, b, _, c = g0
    for sw in (2, 0x80000000, 0xFFFFFFFF):
        bad("sign_word_%x" % sw, (a, b, sw, c), "sign_word")
    if ident.b == 0:
        bad("minus_zero", (1, 0, 1, ident.c), "zero_sign")
    bad("b_plus_2a", (a, b + 2 * a, 0, a + b + c), "b_le_a")          # the discriminant is right: only the range is wrong
    bad("b_minus_2a", (a, 2 * a - b, 1, a - b + c), "b_le_a")
    for i, f in enumerate(g):
        if f.c < PLANE:
            bad("swapped%d" % i, (f.c, f.b, 1, f.a), "a_le_c")       # (c, -b, a)
    if amb:
        bad("b_eq_minus_a", (4, 4, 1, amb.c), "edge_sign")
    else:
        bad("b_eq_minus_a", (1, 1, 1, ident.c), "edge_sign")         # odd Delta: the identity is the form with b = a
    if owned:
        bad("a_eq_c_negative", (owned[0], owned[1], 1, owned[0]), "edge_sign")
    if D % 2 == 0:
        bad("low_bits", (1, 1, 0, D // 4), "low_bits")
    else:
        bad("low_bits", (1, 0, 0, D // 4), "low_bits")
    # the equation, near misses: one unit, then one bit in every lane of every plane of every coefficient
    bad("c_plus_1", (a, b, 0, c + 1), "equation")
    bad("c_minus_1", (a, b, 0, c - 1), "equation")
    for plane in range(2):
        for lane in range(LANES):
            r = _first(((a, b, 0, x) for x in _lane_flips(c, plane * LANES + lane)), D, "equation")
            assert r, "every lane of c has a bit to set"
            bad("c_bit_p%d_l%d" % (plane, lane), r, "equation")
    for lane in range(LANES):
        r = _first(((a, x, 0, c) for x in _lane_flips(b, lane, up=False)), D, "equation")      # downwards: |b| <= a holds
        if r:
            bad("b_bit_l%d" % lane, r, "equation")
        r = _first(((x, pf.b, 0, pf.c) for x in _lane_flips(pf.a, lane, lo=0) if x <= pf.c), D, "equation")   # upwards, a <= c holds
        if r:
            bad("a_bit_l%d" % lane, r, "equation")
    # a c == (b^2 + |Delta|) / 4 modulo 2^2560 and nowhere else: only the third plane of the product tells
    T = (b * b + D) // 4
    wrap = []
    for k in range(1, 40):
        a2 = (a | 1) + 2 * k
        if T % a2:
            wrap.append((a2, b, 0, T * pow(a2, -1, PLANE * PLANE) % (PLANE * PLANE)))
    r = _first(wrap, D, "equation")
    assert r and r[0] * r[3] >= PLANE * PLANE and r[0] * r[3] % (PLANE * PLANE) == T
    bad("wrap_around", r, "equation")
    # everything at its maximum: the carry out of b^2 + |Delta| (none below 1281 bits of |Delta|: an equation case there)
    for label, cmax in (("all_max", PLANE * PLANE - 2), ("all_ones", PLANE * PLANE - 1)):
        r = (PLANE - 1, PLANE - 1, 0, cmax)
        bad(label, r, "no_carry" if "no_carry" in failed(r, D) else "equation")
    bad("a_zero", (0, 0, 0, 1), "positive")
    bad("c_zero", (a, b, 0, 0), "positive")
    if D % 8 == 0:
        bad("content2_2_0", (2, 0, 0, D // 8), "primitive")
    if D % 32 == 0:
        bad("content2_4_0", (4, 0, 0, D // 16), "primitive")
    if D % 16 == 0:
        gq = P.random_form(delta // 4, rng) if big else P.random_form(delta // 4, rng, 12, 10)
        bad("content2_random", (2 * gq.a, 2 * abs(gq.b), 1 if gq.b < 0 else 0, 2 * gq.c), "primitive")
    assert all(cs.rec is not None for cs in out), [cs.label for cs in out if cs.rec is None]
    return out


def owned_discriminant():
    """a discriminant of exactly 2400 bits, the largest a context takes, that holds a form (a, b, a): |Delta| = 4 a^2 - b^2
    with a odd of 1199 bits (38 limbs: the top lane of the plane holds data) and b = 2 (mod 4) of 1198 bits, coprime"""
    rng = P.SplitMix64(2400)
    while True:
        a = rng.bits(1199) | (7 << 1196) | 1
        b = (rng.bits(1198) | (1 << 1197) | 3) ^ 1
        if math.gcd(a, b) == 1:
            break
    D = 4 * a * a - b * b
    assert D.bit_length() == 2400 and D % 32 == 0 and b % 4 == 2 and a.bit_length() > 37 * 32
    return -D, (a, b)


@functools.lru_cache(maxsize=None)
def discriminants():
    """the five: the three golden parameter sets, an odd fundamental -q of 256 bits, the owned one of 2400 bits"""
    out = []
    for name in ("tiny_k8", "s128_k128", "s128_k256"):
        prm = load_json("params_%s.json" % name)
        delta = hx(prm["delta"])
        fix = [(k, P.Form(hx(prm[k]["a"]), hx(prm[k]["b"]), hx(prm[k]["c"]))) for k in ("f", "h", "pk")]
        out.append(Disc(name, delta, tuple(_cases(delta, P.SplitMix64(11), fix))))
    rng = P.SplitMix64(256)
    q = P.random_prime(256, rng, 3)
    q = q if q % 4 == 3 else P.random_prime(256, rng, 7)
    out.append(Disc("odd_256", -q, tuple(_cases(-q, rng))))
    delta, ab = owned_discriminant()
    out.append(Disc("owned_2400", delta, tuple(_cases(delta, P.SplitMix64(12), owned=ab))))
    return tuple(out)


def too_wide_discriminant():
    """2401 bits, 0 (mod 4): one bit more than a context takes"""
    return -(1 << 2400)


def passes(d):
    return [cs for cs in d.cases if cs.names is None]


def forgeries(d):
    return [cs for cs in d.cases if cs.names is not None]
