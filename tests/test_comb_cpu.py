"""CPU: the fixed-base comb's recoding and slot map (cofhe_amd/csrc/comb.hpp, compiled for the host as k_comb_first runs
it), and how its launcher chunks and carves the workspace (cofhe_hip_comb_shape, cofhe_hip_workspace_plan "comb").  No
kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libcombsim.so")
EXP_BITS = 992
WIDTHS = range(2, 11)
REC_BYTES = 168 * 4
KINDS = (0, 1, 2)         # powers, fresh encryption, re-randomisation


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "comb_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("comb.hpp", "qf.hpp", "mp.hpp", "lane.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cofhe_amd import load_library
    return load_library()


def exp_rec(v):
    r = np.zeros(32, dtype=np.uint32)
    r[:31] = np.frombuffer(abs(v).to_bytes(124, "little"), dtype="<u4")
    r[31] = 1 if v < 0 else 0
    return r


def digits(sim, v, w, nbits=EXP_BITS, npos=None):
    npos = npos if npos is not None else nbits // w + 1
    out = np.zeros(npos, dtype=np.int32)
    e = exp_rec(v)
    sim.comb_sim_digits(e.ctypes.data_as(C.c_void_p), C.c_int(w), C.c_int(nbits), C.c_int(npos), out.ctypes.data_as(C.c_void_p))
    return [int(d) for d in out]


def edge_exponents(w, rng):
    vals = [0, 1, -1, (1 << 992) - 1, -((1 << 991) + 1)]
    for s in range(1, 992 // w + 1):
        for t in (w * s - 1, w * s, w * s + 1):
            if 0 < t < 992:
                vals += [1 << t, (1 << t) - 1]
    bound = 1 << 966                                    # exponent_bound of the s128 parameter sets
    vals += [rng.randrange(bound) for _ in range(40)] + [-rng.randrange(bound) for _ in range(10)]
    return vals


@pytest.mark.parametrize("w", WIDTHS)
def test_booth_digits_reproduce_the_exponent(sim, w):
    """sum_j d_j 2^(wj) = |e| with |d_j| <= 2^(w-1), in floor(B/w) + 1 positions for a B-bit magnitude; the digits beyond
    are zero"""
    rng = random.Random(w)
    for v in edge_exponents(w, rng):
        m = abs(v)
        B = m.bit_length()
        npos = B // w + 1
        d = digits(sim, v, w, npos=EXP_BITS // w + 1)
        assert all(abs(x) <= 1 << (w - 1) for x in d), (w, v)
        assert all(x == 0 for x in d[npos:]), (w, v)
        assert sum(x << (w * j) for j, x in enumerate(d[:npos])) == m, (w, v)


@pytest.mark.parametrize("w", WIDTHS)
def test_digits_of_the_low_k_bits(sim, w):
    """the plaintext's digits read its low k bits only: they give |m| mod 2^k in floor(k/w) + 1 positions"""
    rng = random.Random(100 + w)
    for k in (8, 128, 256):
        for v in [0, 1, (1 << k) - 1, 1 << k, (1 << k) + 7, rng.getrandbits(400), (1 << 991) - 1]:
            d = digits(sim, v, w, nbits=k, npos=k // w + 1)
            assert sum(x << (w * j) for j, x in enumerate(d)) == v % (1 << k)
            assert all(abs(x) <= 1 << (w - 1) for x in d)


def slot_map(sim, w, npos_r, npos_m, leaf, halves, kbits, h, r, m):
    er, em = exp_rec(r), exp_rec(m)
    n = (npos_r + npos_m + leaf + 1) & ~1
    sel = np.zeros(4 * n, dtype=np.int32)
    ns = C.c_uint32()
    sim.comb_sim_slots(C.c_uint32(w), C.c_uint32(npos_r), C.c_uint32(npos_m), C.c_uint32(leaf), C.c_uint32(halves), C.c_uint32(kbits),
                       C.c_uint32(h), er.ctypes.data_as(C.c_void_p), em.ctypes.data_as(C.c_void_p), sel.ctypes.data_as(C.c_void_p), C.byref(ns))
    assert ns.value == n
    return sel.reshape(n, 4)


@pytest.mark.parametrize("w", [2, 5, 8, 10])
@pytest.mark.parametrize("kind", KINDS)
def test_slot_map_reproduces_r_and_m(sim, w, kind):
    """over all slots of a column, the selected (table, position, digit) multiply out to base^r (and, in the c2 column of an
    encryption, f^(m mod 2^k)); each entry record is position * 2^(w-1) + |digit| - 1; the leaf slot is there exactly once
    in a re-randomisation and the padding is principal"""
    rng = random.Random(7 * w + kind)
    k = 128
    halves = 1 if kind == 0 else 2
    for r, m in [(0, 0), (1, -1), (-5, (1 << k) - 1), (rng.randrange(1 << 966), -rng.getrandbits(200)),
                 ((1 << 966) - 1, rng.getrandbits(k)), (-(rng.randrange(1 << 966)), 1 << k)]:
        bits = max(abs(r).bit_length(), 1)
        npos_r = bits // w + 1
        npos_m = k // w + 1 if kind == 1 else 0
        leaf = 1 if kind == 2 else 0
        for h in range(halves):
            sel = slot_map(sim, w, npos_r, npos_m, leaf, halves, k, h, r, m)
            acc = {0: 0, 1: 0, 2: 0}
            leaves = 0
            for s, row in enumerate(sel):
                table, pos, dg, entry = (int(x) for x in row)
                if table in (0, 1, 2):
                    assert dg != 0 and abs(dg) <= 1 << (w - 1)
                    assert entry == pos * (1 << (w - 1)) + abs(dg) - 1
                    acc[table] += dg << (w * pos)
                elif table == 3:
                    leaves += 1
                    assert s == npos_r + npos_m
                else:
                    assert table == -1
            assert acc[1 - h] == 0 or halves == 1                # a column reads the r table of its own half only
            assert acc[h] == r
            if kind == 1 and h == 1:
                want = abs(m) % (1 << k)
                assert acc[2] == (-want if m < 0 else want)
            else:
                assert acc[2] == 0
            assert leaves == leaf


def test_comb_shape_and_workspace_plan(lib):
    """chunks on both sides of a boundary and up to 2^22 items: the regions of one pass are disjoint and 256-byte aligned, the
    first level holds slots / 2 records per column and the second ceil(slots / 4), the total stays within 4 GiB; the pins
    are honoured; bad arguments are refused"""
    from cofhe_amd import engine
    for kind in KINDS:
        halves = 1 if kind == 0 else 2
        for w in (0, 2, 6, 8, 10):
            for bits in (0, 5, 966, 992):
                k = 128 if kind == 1 else 0
                ww, slots, big = engine.comb_shape(kind, 1 << 22, bits, k, w, 0)
                assert ww == (w or ww) and 2 <= ww <= 10
                want_slots = bits // ww + 1 + ((k // ww + 1) if kind == 1 else 0) + (1 if kind == 2 else 0)
                assert slots == (want_slots + 1) // 2 * 2
                for n in (1, big - 1, big, big + 1, 2 * big + 1, 1 << 22):
                    if n < 1:
                        continue
                    ww2, slots2, chunk = engine.comb_shape(kind, n, bits, k, w, 0)
                    assert (ww2, slots2) == (ww, slots) and chunk == min(n, big)
                    regs, total = engine.workspace_plan("comb", kind, n, bits, k, w, 0)
                    end = 0
                    for name, off, nbytes in regs:
                        assert off % 256 == 0 and off >= end
                        end = off + nbytes
                    assert end == total <= 4 << 30
                    r = {name: (off, nbytes) for name, off, nbytes in regs}
                    cols = chunk * halves
                    assert r["level_a"][1] == slots // 2 * cols * REC_BYTES
                    assert r["level_b"][1] == (slots + 3) // 4 * cols * REC_BYTES
    # a pinned chunk is taken as it is, and capped where the bound needs it
    assert engine.comb_shape(1, 1000, 966, 128, 8, 33)[2] == 33
    assert engine.comb_shape(1, 20, 966, 128, 8, 33)[2] == 20
    assert engine.comb_shape(1, 1 << 22, 966, 128, 2, 1 << 30)[2] < 1 << 30
    for bad in [(3, 1, 0, 0, 0, 0), (0, 1, 993, 0, 0, 0), (0, 1, 10, 0, 1, 0), (0, 1, 10, 0, 11, 0), (1, 1, 10, 0, 8, 0),
                (1, 1, 10, 992, 8, 0), (0, 1 << 41, 10, 0, 0, 0)]:
        with pytest.raises(Exception):
            engine.comb_shape(*bad)
        with pytest.raises(Exception):
            engine.workspace_plan("comb", *bad)
    with pytest.raises(Exception):
        engine.workspace_plan("comb", 0, 1, 10, 0, 0)              # wrong argument count
