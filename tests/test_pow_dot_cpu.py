"""CPU: the schedule of k_pow_dot (cofhe_amd/csrc/pow_dot.hpp) compiled for the host and walked over a multiplicative group of
Python integers: it must end with prod base_i^exp_i after T squarings and (non-zero digits - 1) multiplications; the new entry
points among the library's symbols; the host harness with its new mode.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import poly_cases as PC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libpowdotsim.so")
PRIME = (1 << 61) - 1                       # the group: integers mod a fixed 61-bit prime
COPY, SQUARE, MUL = 1, 2, 3
DEGREES = (1, 2, 3, 8)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "pow_dot_sim.cpp")
    deps = [src, os.path.join(ROOT, "cofhe_amd", "csrc", "pow_dot.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return g


def walk(sim, exps):
    """the operations of the walk over these exponents: [(kind, base, inverted)]"""
    digs = [PC.naf(v) for v in exps]
    npos = max(1, max(len(x) for x in digs))
    m = np.zeros((len(exps), npos), dtype=np.int8)
    for i, x in enumerate(digs):
        m[i, :len(x)] = x
    cap = npos * (len(exps) + 1) + 1
    ops = np.zeros(3 * cap, dtype=np.int32)
    n = sim.pow_dot_sim_walk(m.ctypes.data_as(C.c_void_p), C.c_int(len(exps)), C.c_int(npos), ops.ctypes.data_as(C.c_void_p), C.c_int(cap))
    assert n >= 0
    return [tuple(int(v) for v in ops[3 * r:3 * r + 3]) for r in range(n)]


def run_walk(ops, bases):
    """the accumulator after the walk (1 for a walk without operations: the kernel writes the principal form), squarings, multiplications"""
    acc, sq, mul = None, 0, 0
    for r, (kind, i, inv) in enumerate(ops):
        b = pow(bases[i], -1, PRIME) if inv else bases[i]
        if kind == COPY:
            assert r == 0 and acc is None, "the copy starts the walk and nothing else"
            acc = b
        elif kind == SQUARE:
            acc = acc * acc % PRIME
            sq += 1
        else:
            assert kind == MUL
            acc = acc * b % PRIME
            mul += 1
    return (1 if acc is None else acc), sq, mul


def check(sim, exps, bases):
    ops = walk(sim, exps)
    got, sq, mul = run_walk(ops, bases)
    want = 1
    for b, v in zip(bases, exps):
        want = want * pow(b, v, PRIME) % PRIME
    assert got == want
    assert (sq, mul) == PC.walk_counts(exps)
    if any(exps):
        assert ops[0][0] == COPY                       # never a product with the neutral element
    else:
        assert ops == []


def test_degree_bound(sim):
    assert sim.pow_dot_sim_max_degree() == PC.MAX_DEGREE == max(DEGREES)


@pytest.mark.parametrize("d", DEGREES)
def test_walk_ends_with_the_product_of_powers(sim, d):
    """every exponent family at k = 8 and k = 128, distinct bases and two equal bases"""
    rng = random.Random(61 * d)
    for k in (8, 128):
        for name, exps in PC.exponent_families(d, k, rng):
            bases = [rng.randrange(2, PRIME) for _ in range(d)]
            check(sim, exps, bases)
            if d >= 2:
                bases[1] = bases[0]
                check(sim, exps, bases)


def test_walk_named_cases(sim):
    """exponent 1 alone is one copy; 2^k - 1 is k squarings and one multiplication by the inverse; a negative exponent starts
    from the inverse; bases that share the top digit: one copy, then multiplications at the top position, before any squaring"""
    assert walk(sim, [1]) == [(COPY, 0, 0)]
    assert walk(sim, [-1]) == [(COPY, 0, 1)]
    ops = walk(sim, [(1 << 128) - 1])
    assert ops[0] == (COPY, 0, 0) and ops[-1] == (MUL, 0, 1) and [o[0] for o in ops[1:-1]] == [SQUARE] * 128
    assert walk(sim, [5, 4, 0, -4])[:4] == [(COPY, 0, 0), (MUL, 1, 0), (MUL, 3, 1), (SQUARE, 0, 0)]     # 101, 100, 0, -(100): top 2 three times
    ops = walk(sim, [5, 0, 7, 4])                       # 5 = 101, 7 = 100(-1) with its top at position 3, 4 = 100
    assert ops[0] == (COPY, 2, 0) and ops[1] == (SQUARE, 0, 0)
    assert ops[2:4] == [(MUL, 0, 0), (MUL, 3, 0)] and ops[4][0] == SQUARE
    check(sim, [5, 0, 7, 4], [3, 5, 7, 11])
    check(sim, [6, 6, 6], [3, 3, 7])


def test_walk_random_exponents(sim):
    """d in {1, 2, 3, 8}, lengths up to 992 bits, signs mixed"""
    rng = random.Random(2024)
    for d in DEGREES:
        for _ in range(20):
            exps = [rng.choice((1, -1)) * rng.getrandbits(rng.choice((1, 3, 8, 128, 992))) for _ in range(d)]
            check(sim, exps, [rng.randrange(2, PRIME) for _ in range(d)])


def test_new_entry_points_are_exported(built):
    """fails without the feature: the symbols of the polynomial evaluation and the Engine's wrappers"""
    from cofhe_amd import lib_path
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path()], text=True)
    for name in ("cofhe_hip_pow_dot_records", "cofhe_hip_poly_shift_records", "cofhe_hip_poly_close_records", "cofhe_hip_poly_close_tensors_bytes"):
        assert (" T " + name + "\n") in syms, name
    from cofhe_amd import Engine
    for name in ("pow_dot_records", "poly_shift_records", "poly_close_records", "poly_close_tensors"):
        assert callable(getattr(Engine, name))


def test_local_bench_lists_the_new_mode(built):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1
    assert "poly_activation" in r.stderr
