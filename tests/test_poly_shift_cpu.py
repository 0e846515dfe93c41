"""CPU: the Taylor shift mod 2^k of the polynomial evaluation -- the body of k_poly_shift (cofhe_amd/csrc/poly_shift.hpp)
compiled for the host and run element by element as the kernel runs it, against Python integers with the binomials from
math.comb.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import plain_mm_cases as PM
import poly_cases as PC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libpolyshiftsim.so")
KBITS = (8, 128, 256, 300)                  # one limb with a sub-word mask, L = 4, L = 8 (the last register path), the runtime-L path
DEGREES = (0, 1, 2, 3, 8)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "poly_shift_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("poly_shift.hpp", "pow_dot.hpp", "plain_mm.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


def run_sim(sim, coef, xs, k):
    d, n = len(coef) - 1, len(xs)
    rc_, rx = PM.exp_records(coef), PM.exp_records(xs)
    q = np.full((d + 1) * n * 32, 0xA5A5A5A5, dtype=np.uint32)       # the kernel must write every word of every record
    rc = sim.poly_shift_sim(rc_.ctypes.data_as(C.c_void_p), rx.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), C.c_uint64(n),
                            C.c_uint32(d), C.c_uint32(k))
    assert rc == 0
    return q


def expected(coef, xs, k):
    """power-major: q_i of every element, then q_(i+1) of every element"""
    per = [PC.taylor_shift(coef, x, k) for x in xs]
    return [per[e][i] for i in range(len(coef)) for e in range(len(xs))]


def coefficients(d, k, rng, family):
    top = (1 << k) - 1
    if family == "random":
        return [rng.getrandbits(k) for _ in range(d + 1)]
    if family == "signed":               # sign words set, magnitudes of 2^k and above, -0
        return [rng.choice((-1, 1)) * rng.getrandbits(k + 40) for _ in range(d)] + [-top]
    if family == "top":
        return [top] * (d + 1)
    assert family == "square"
    return [0] * d + [1]


def test_k_values_cover_both_paths(sim):
    L = sim.poly_shift_sim_fixed_limbs()
    assert any((k + 31) // 32 == L for k in KBITS) and any((k + 31) // 32 > L for k in KBITS) and any(k % 32 for k in KBITS)


@pytest.mark.parametrize("k", KBITS)
def test_poly_shift_body_matches_python_integers(sim, k):
    """exact, for every degree and coefficient family at x in {0, 1, 2^k - 1, 2^(k-1), random}, negative x and x of 2^k and above;
    outputs have sign word 0 and nothing at or above bit k"""
    rng = random.Random(7000 + k)
    for d in DEGREES:
        xs = PC.shift_points(k, 9, rng) + [-rng.getrandbits(k), -1, (1 << k) + 3, (1 << 900) + 5]
        for family in ("random", "signed", "top", "square"):
            coef = coefficients(d, k, rng, family)
            PM.check_output(run_sim(sim, coef, xs, k), expected(coef, xs, k), k)


def test_degree_zero_is_the_copy_of_c0(sim):
    q = run_sim(sim, [-5], [3, 4], 128)
    PM.check_output(q, [(1 << 128) - 5] * 2, 128)


def test_q0_is_the_polynomial_at_x(sim):
    rng = random.Random(11)
    coef, xs = [rng.getrandbits(128) for _ in range(4)], PC.shift_points(128, 8, rng)
    got = PM.record_values(run_sim(sim, coef, xs, 128))
    assert [v for v, _ in got[:8]] == [PC.poly(coef, x, 128) for x in xs]


def test_poly_shift_refuses_k_out_of_range(sim):
    z = PM.exp_records([1, 1])
    q = np.zeros(64, dtype=np.uint32)
    args = (z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), q.ctypes.data_as(C.c_void_p), C.c_uint64(1))
    assert sim.poly_shift_sim(*args, C.c_uint32(1), C.c_uint32(0)) == -1
    assert sim.poly_shift_sim(*args, C.c_uint32(1), C.c_uint32(641)) == -1
    assert sim.poly_shift_sim(*args, C.c_uint32(9), C.c_uint32(128)) == -1
    assert sim.poly_shift_sim(*args, C.c_uint32(1), C.c_uint32(640)) == 0 and (q[0], q[32]) == (2, 1)
