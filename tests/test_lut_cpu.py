"""CPU: the index arithmetic of the table lookups from one opened value -- lut.hpp (cofhe_amd/csrc), which k_lut_rotate and
k_lut_select call, compiled for the host -- against Python integers.  Exact.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import lut_cases as LC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "liblutsim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "lut_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("lut.hpp", "plain_mm.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


def sim_index(sim, vals, b, rc_want=0):
    recs = LC.records(vals)
    idx = np.full(max(len(vals), 1), 0xA5A5A5A5, dtype=np.uint32)
    rc = sim.lut_sim_index(recs.ctypes.data_as(C.c_void_p), C.c_uint64(len(vals)), C.c_uint32(b), idx.ctypes.data_as(C.c_void_p))
    assert rc == rc_want
    return [int(v) for v in idx[:len(vals)]]


def sim_rotate(sim, tab, n_tab, rs, b, rc_want=0):
    n = len(rs)
    t, r = LC.records(tab), LC.records(rs)
    out = np.full(max(n << b, 1) * 32, 0xA5A5A5A5, dtype=np.uint32)
    rc = sim.lut_sim_rotate(t.ctypes.data_as(C.c_void_p), C.c_uint64(n_tab), r.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                            C.c_uint64(n), C.c_uint32(b))
    assert rc == rc_want
    return out[:(n << b) * 32]


def test_the_reference_by_hand():
    """the Python reference on small numbers worked by hand: 13 = 0b1101 has the low three bits 5; -13 = -16 + 3; -0 is 0;
    -8 mod 8 = 0; 2^k and 2^k + 5 keep their low bits; a rotation by r = 3 of (a, b, c, d) reads from entry 3 on; and the
    protocol's identity (e + r) mod 2^b = x mod 2^b for e = x - r mod 2^k"""
    assert LC.index((13, 0), 3) == 5 and LC.index((13, 1), 3) == 3 and LC.index((0, 1), 3) == 0 and LC.index((8, 1), 3) == 0
    assert LC.index((1, 1), 1) == 1 and LC.index((1, 1), 12) == 4095 and LC.index(((1 << 128) + 5, 0), 8) == 5
    assert LC.index(((1 << 128) + 5, 1), 8) == 251 and LC.index((1 << 128, 1), 8) == 0
    tab = [(10, 0), (11, 0), (12, 1), (13, 0)]
    assert LC.rotate(tab, 1, [(3, 0)], 2) == [(13, 0), (10, 0), (11, 0), (12, 1)]
    assert LC.rotate(tab, 1, [(1, 1)], 2) == [(13, 0), (10, 0), (11, 0), (12, 1)]          # -1 = 3 mod 4
    assert LC.rotate(tab + tab[::-1], 2, [(0, 0), (1, 0)], 2)[4:] == [(12, 1), (11, 0), (10, 0), (13, 0)]
    assert LC.selected([(5, 0), (5, 1)], 2) == [1, 4 + 3]
    assert LC.relu_table(3) == [0, 1, 2, 3, 0, 0, 0, 0] and LC.signed(5, 3) == -3 and LC.signed(3, 3) == 3
    rng = random.Random(1)
    for _ in range(2000):
        k = rng.choice((8, 33, 128))
        b = rng.randrange(1, min(k, 12) + 1)
        x, r = rng.getrandbits(k), rng.getrandbits(k)
        e = (x - r) % (1 << k)
        tab = list(range(100, 100 + (1 << b)))
        assert LC.rotate([(t, 0) for t in tab], 1, [(r, 0)], b)[LC.index((e, 0), b)] == (tab[x % (1 << b)], 0)


@pytest.mark.parametrize("b", LC.BITS_CPU)
def test_index_matches_python_integers(sim, b):
    """0, 1, 2^b - 1, 2^b, 2^k - 1, set sign words, -0, magnitudes of 2^k and above and random values of up to 992 bits, at
    three values of k: two words of the record decide, whatever the others hold"""
    for k in (max(b, 8), 128, 639):
        vals = LC.values(b, k, 200, random.Random(100 * b + k))
        assert sim_index(sim, vals, b) == [LC.index(v, b) for v in vals]
    every = [(m, s) for m in range(1 << min(b, 8)) for s in (0, 1)]
    assert sim_index(sim, every, b) == [LC.index(v, b) for v in every]


@pytest.mark.parametrize("b", LC.BITS_CPU)
def test_rotate_matches_python_integers(sim, b):
    """the rows of the tuples word for word: one table, three, one per element; masks from every family"""
    rng = random.Random(b)
    rs = LC.values(b, 128, 14 if b < 12 else 3, rng)              # 14 masks: one of every fixed family
    for n_tab in (1, 3, len(rs)):
        use = rs[:len(rs) - len(rs) % n_tab]
        tab = LC.table(b, n_tab, rng)
        got = sim_rotate(sim, tab, n_tab, use, b)
        assert np.array_equal(got, LC.records(LC.rotate(tab, n_tab, use, b)))


def test_every_rotation_of_a_small_table(sim):
    """b = 3: all 8 rotations, each row a cyclic shift, every entry present once"""
    tab = LC.table(3, 1, random.Random(3))
    for r in range(8):
        got = sim_rotate(sim, tab, 1, [(r, 0)], 3).reshape(8, 32)
        want = LC.records(tab).reshape(8, 32)
        assert np.array_equal(got, np.roll(want, -r, axis=0))


def test_refusals(sim):
    """bits = 0 and 13, no table, an element count that is no multiple of the table count: refused, nothing written"""
    assert sim.lut_sim_max_bits() == LC.MAX_BITS == 12
    tab = LC.table(3, 2, random.Random(0))
    for b, n_tab, n in ((0, 1, 2), (13, 1, 2), (3, 0, 2), (3, 2, 3)):
        t, r = LC.records(tab), LC.records([(1, 0)] * n)
        buf = np.full(64 * 32, 0xA5A5A5A5, dtype=np.uint32)
        rc = sim.lut_sim_rotate(t.ctypes.data_as(C.c_void_p), C.c_uint64(n_tab), r.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p),
                                C.c_uint64(n), C.c_uint32(b))
        assert rc == -1 and (buf == 0xA5A5A5A5).all()
    for b in (0, 13):
        assert sim_index(sim, [(1, 0)], b, rc_want=-1) == [0xA5A5A5A5]


def test_the_tuples_shape_gives_the_bits_or_is_refused():
    """cofhe_hip_lut_tuples_shape_bits (host only): shape S + [2^bits], 1 <= bits <= 12, for S of 0 to 7 dimensions; everything
    else is COFHE_HIP_ESHAPE and leaves *bits alone"""
    from cofhe_amd import load_library
    L = load_library()

    def bits(se, st):
        b = C.c_uint32(77)
        rc = L.cofhe_hip_lut_tuples_shape_bits(C.c_uint32(len(se)), (C.c_uint32 * 8)(*se), C.c_uint32(len(st)), (C.c_uint32 * 9)(*st), C.byref(b))
        assert rc in (0, -2) and (rc == 0 or b.value == 77)
        return b.value if rc == 0 else None

    for b in range(1, 13):
        assert bits([5], [5, 1 << b]) == b
    assert bits([], [8]) == 3 and bits([2, 3], [2, 3, 2]) == 1 and bits([0], [0, 4]) == 2
    assert bits([1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 16]) == 4
    for se, st in (([5], [5, 1]), ([5], [5, 1 << 13]), ([5], [5, 12]), ([5], [5, 0]), ([5], [80]), ([5], [16, 5]), ([5], [4, 16]),
                   ([5], [5, 1, 16]), ([5, 1], [5, 16]), ([], []), ([5], []), ([1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 1, 2])):
        assert bits(se, st) is None, (se, st)
