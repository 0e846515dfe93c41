"""CPU: the signed floor division mod 2^k of the division by public divisors -- the body of k_plain_divfloor
(cofhe_amd/csrc/plain_div.hpp) compiled for the host and run on the lane-group simulator, one 8-lane group per element as the
kernel runs it, against Python integers.  Exact.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import div_cases as DC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libplaindivsim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "plain_div_sim.cpp")
    deps = [src, os.path.join(HERE, "hostsim", "sim.cpp")] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in
                                                               ("plain_div.hpp", "plain_mm.hpp", "mp.hpp", "lane.hpp", "qf.hpp", "form_io.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-DCOFHE_WG_GROUPS=32", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.sim_status()
    L.sim_flags()
    return L


def run_sim(sim, nums, divs, k, rc_want=0):
    """the quotients' records of nums (pairs (magnitude, sign word)) by divs (integers; element e reads divisor e mod len(divs))"""
    n = len(nums)
    v, d = DC.records(nums), DC.int_records(divs)
    q = np.full(max(n, 1) * 32, 0xA5A5A5A5, dtype=np.uint32)         # the kernel must write every word of every record
    rc = sim.plain_div_sim(v.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint64(len(divs)), q.ctypes.data_as(C.c_void_p),
                           C.c_uint64(n), C.c_uint32(k))
    assert rc == rc_want
    return q[:n * 32]


def test_the_reference_is_the_floor_of_the_centred_residue():
    """the Python reference on small numbers worked by hand, and the negative branch's identity floor(-m / D) =
    -(floor((m - 1) / D) + 1) that the kernel uses"""
    assert DC.divfloor((7, 0), 2, 8) == 3 and DC.divfloor((7, 1), 2, 8) == 256 - 4 and DC.divfloor((128, 0), 1, 8) == 128
    assert DC.divfloor((255, 0), 3, 8) == 255 and DC.divfloor((0, 1), 3, 8) == 0 and DC.divfloor((5, 0), 0, 8) == 0
    rng = random.Random(1)
    for _ in range(2000):
        m, D = rng.randrange(1, 1 << 40), rng.randrange(1, 1 << 20)
        assert (-m) // D == -((m - 1) // D + 1)


@pytest.mark.parametrize("k", DC.KBITS_CPU)
def test_divfloor_body_matches_python_integers(sim, k):
    """exact, element-wise divisors: every divisor family (1, 2, 3, 2^t, 2^(k-1) - 1, one limb, two limbs, full width) with 0,
    1, -1, the most negative and the most positive value, multiples of D and their neighbours of either sign, |v| < D, set sign
    words, magnitudes of 2^k and above, -0; then +-qD, +-(qD - 1), +-(qD + D - 1) on the divisors that reach the add-back of
    mp_divrem_norm (checked, where k leaves room for a divisor beyond one limb); the status word stays clear"""
    cs = DC.cases(k)
    nums, divs = [c[0] for c in cs], [c[1] for c in cs]
    sim.sim_flags()
    DC.check_output(run_sim(sim, nums, divs, k), [DC.divfloor(v, D, k) for v, D in cs], k)
    assert sim.sim_status() == 0
    flags = sim.sim_flags()
    if k >= 64:
        assert flags & 8, "the add-back family did not reach the add-back of mp_divrem_norm"


@pytest.mark.parametrize("k", (8, 128, 300))
@pytest.mark.parametrize("n_div", (1, 3, 12))
def test_broadcast_of_the_divisors(sim, k, n_div):
    """element e reads divisor e mod n_div: a scalar, three channels, element-wise"""
    rng = random.Random(40 * k + n_div)
    n = 12
    nums = [(rng.getrandbits(k), rng.randrange(2)) for _ in range(n)]
    divs = [rng.randrange(1, 1 << (k - 1)) for _ in range(n_div)]
    DC.check_output(run_sim(sim, nums, divs, k), [DC.divfloor(nums[e], divs[e % n_div], k) for e in range(n)], k)
    assert sim.sim_status() == 0


@pytest.mark.parametrize("k", (8, 33, 128, 639))
def test_invalid_divisors_give_zero_and_the_status_bit(sim, k):
    """0, 2^(k-1), 2^k - 1, a residue of 0 and a set sign word: quotient 0, CF_ST_DIV_CAP, and the valid elements next to them
    are divided all the same; each invalid divisor sets the bit on its own"""
    rng = random.Random(k)
    bad = DC.invalid_divisors(k)
    divs = [3] + bad + [1]
    nums = [(rng.getrandbits(k), 0) for _ in divs]
    want = [DC.divfloor(v, D, k) for v, D in zip(nums, divs)]
    assert want[1:-1] == [0] * len(bad) and want[-1] == nums[-1][0]
    DC.check_output(run_sim(sim, nums, divs, k), want, k)
    assert sim.sim_status() == DC.ST_DIV_CAP
    for D in bad:
        DC.check_output(run_sim(sim, [(5, 0)], [D], k), [0], k)
        assert sim.sim_status() == DC.ST_DIV_CAP
    DC.check_output(run_sim(sim, [(5, 0)], [(1 << k) + 3], k), [1], k)          # a magnitude of 2^k and above enters as its residue
    assert sim.sim_status() == 0


def test_refusals(sim):
    """kbits = 0, kbits = 640, no divisor, an element count that is no multiple of the divisor count: refused, nothing written"""
    assert sim.plain_div_sim_max_kbits() == 639
    for k, divs, n in ((0, [3], 2), (640, [3], 2), (128, [], 2), (128, [3, 5], 3)):
        q = run_sim(sim, [(9, 0)] * n, divs, k, rc_want=-1)
        assert (q == 0xA5A5A5A5).all()
    DC.check_output(run_sim(sim, [(9, 0)], [3], 639), [3], 639)
    assert len(run_sim(sim, [], [3], 128)) == 0


@pytest.mark.parametrize("k", DC.KBITS_CPU)
def test_the_pair_and_the_opened_value_give_the_floor_or_one_less(sim, k):
    """the protocol's identity on the simulator: for x and a mask r without a wrap (s(x) = s(r) + s(e), e = x - r mod 2^k),
    r_q + e_q mod 2^k is floor(s(x) / D) or one less -- one less exactly when the remainders of s(r) and s(e) together reach D
    -- and with D = 1 it is exact"""
    rng = random.Random(900 + k)
    M, half = 1 << k, 1 << (k - 1)
    ds = DC.divisors(k, rng)
    xs = [0, 1, M - 1, half, half - 1] + [rng.getrandbits(k) for _ in range(27)]
    divs = [ds[i % len(ds)] for i in range(len(xs))]
    rs = DC.no_wrap_masks(xs, k, rng)
    es = [(x - r) % M for x, r in zip(xs, rs)]
    assert all(DC.centred(x, k) == DC.centred(r, k) + DC.centred(e, k) for x, r, e in zip(xs, rs, es))
    val = lambda q: [int.from_bytes(row[:31].tobytes(), "little") for row in q.reshape(-1, 32)]      # noqa: E731
    rq = val(run_sim(sim, [(r, 0) for r in rs], divs, k))
    eq = val(run_sim(sim, [(e, 0) for e in es], divs, k))
    for x, r, e, D, a, b in zip(xs, rs, es, divs, rq, eq):
        err = (DC.divfloor((x, 0), D, k) - (a + b)) % M
        assert err in (0, 1), (x, D)
        # one less exactly when the two remainders together reach D (never for D = 1)
        assert err == (1 if DC.centred(r, k) % D + DC.centred(e, k) % D >= D else 0), (x, D)
    ones = [1] * len(xs)
    rq, eq = val(run_sim(sim, [(r, 0) for r in rs], ones, k)), val(run_sim(sim, [(e, 0) for e in es], ones, k))
    assert [(a + b) % M for a, b in zip(rq, eq)] == xs
    assert sim.sim_status() == 0
