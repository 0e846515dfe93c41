"""CPU: the piecewise-polynomial activations from one opened value -- the protocol's identity in Python integers, spline.hpp
(cofhe_amd/csrc), whose functions k_spline_rows, k_spline_powers and k_spline_close call, compiled for the host against Python
integers, the table builder (cofhe_amd/host/spline_table.hpp) against numpy, and the host-only shape check of the C ABI.  No
kernel runs."""
import ctypes as C
import os
import random
import re
import subprocess

import numpy as np
import pytest

import spline_cases as SC
from conftest import ROOT
from plain_mm_cases import check_output

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libsplinesim.so")
_TABLE_EXE = os.path.join(HERE, "hostsim", "spline_table_main")
FILL = 0xA5A5A5A5


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(d) > os.path.getmtime(target) for d in deps)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "spline_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("spline.hpp", "poly_shift.hpp", "pow_dot.hpp", "plain_mm.hpp")]
    if _stale(_SO, deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def sim_index(sim, vals, b, t, k, rc_want=0):
    recs = SC.records(vals)
    idx = np.full(max(len(vals), 1), FILL, dtype=np.uint32)
    assert sim.spline_sim_index(ptr(recs), C.c_uint64(len(vals)), C.c_uint32(b), C.c_uint32(t), C.c_uint32(k), ptr(idx)) == rc_want
    return [int(v) for v in idx[:len(vals)]]


def sim_rows(sim, pieces, n_tab, rs, b, t, d, k, rc_want=0):
    n = len(rs)
    tab, r = SC.piece_records(pieces), SC.records(rs)
    out = np.full(max((n << b) * (d + 1), 1) * 32, FILL, dtype=np.uint32)
    rc = sim.spline_sim_rows(ptr(tab), C.c_uint64(n_tab), ptr(r), ptr(out), C.c_uint64(n), C.c_uint32(b), C.c_uint32(t), C.c_uint32(d), C.c_uint32(k))
    assert rc == rc_want
    return out


def sim_powers(sim, es, d, k):
    e = SC.records(es)
    out = np.full(max(len(es) * d, 1) * 32, FILL, dtype=np.uint32)
    assert sim.spline_sim_powers(ptr(e), ptr(out), C.c_uint64(len(es)), C.c_uint32(d), C.c_uint32(k)) == 0
    return out


def test_the_reference_by_hand():
    """small numbers worked by hand: at b = 2, t = 3 the value 0b10110 = 22 lies in segment 2, whose origin is -2 * 8 = -16; -22 mod
    256 = 234 = 0b11101010 lies in segment 1; the field of -0 is 0; 2^k + (5 << t) keeps its field; piece 3 (sigma = -1) of the
    table x -> 7 + 2 (x - o) evaluates 7 + 2 (x + 8)"""
    assert SC.index((22, 0), 3, 2, 8) == 2 and SC.origin(2, 3, 2) == -16 and SC.origin(1, 3, 2) == 8 and SC.origin(3, 3, 2) == -8
    assert SC.index((22, 1), 3, 2, 8) == 1 and SC.index((0, 1), 3, 2, 8) == 0 and SC.index(((1 << 8) + (5 << 3), 0), 3, 2, 8) == 1
    assert SC.index((1 << 33, 0), 30, 4, 128) == 8 and SC.index((1, 1), 30, 4, 128) == 15
    assert SC.piece_value([7, 2], 3, 250, 3, 2, 8) == (7 + 2 * (250 + 8)) % 256
    assert SC.powers([(3, 0), (2, 1)], 2, 8) == [3, 254, 9, 4]
    assert SC.closed([5, 2, 1], 3, 8) == 5 + 6 + 9


@pytest.mark.parametrize("b,t,d", SC.IDENTITY_CASES)
def test_the_identity_exhaustively_at_8_bits(b, t, d):
    """k = 8, every x and every r: the row j = seg(e) of the tuple of r, closed with the powers of e = x - r, is S_{seg(x) - c}(x)
    with c the carry of the low t bits of e and r -- the element's own piece or the one below, and its own when t = 0"""
    k, M = 8, 256
    rng = random.Random(100 * b + 10 * t + d)
    table = [[rng.randrange(M) for _ in range(d + 1)] for _ in range(1 << b)]
    pieces = [[(c, 0) for c in p] for p in table]
    below = 0
    for r in range(M):
        rows = SC.rows(pieces, 1, [(r, 0)], b, t, d, k)
        for x in range(M):
            e = (x - r) % M
            j = SC.segment(e, t, b)
            want, p = SC.expected(table, x, r, b, t, k)
            assert SC.closed(rows[j * (d + 1):(j + 1) * (d + 1)], e, k) == want, (x, r)
            assert p in (SC.segment(x, t, b), (SC.segment(x, t, b) - 1) % (1 << b))
            below += p != SC.segment(x, t, b)
    assert (below == 0) == (t == 0)


INDEX_WINDOWS = [(0, 4), (31, 4), (32, 4), (30, 4)]              # (t, b): the bottom, a word's last bit, a word's first, straddling


@pytest.mark.parametrize("k", [8, 128, 256, 639])
def test_index_matches_python_integers(sim, k):
    """set sign words, -0, magnitudes of 2^k and above and random values of up to 992 bits; t at 0, 31, 32 and 30 with b = 4
    (straddling a word) where k has room, t + b = k, and the field in the top word of k"""
    windows = [(t, b) for t, b in INDEX_WINDOWS if t + b <= k] + [(k - 4, 4), (k - 1, 1), (max(k - 11, 0), min(k, 11)), (0, 1)]
    for t, b in windows:
        vals = SC.values(t, b, k, 120, random.Random(1000 * k + 10 * t + b))
        assert sim_index(sim, vals, b, t, k) == [SC.index(v, t, b, k) for v in vals], (t, b)
    every = [(m, s) for m in range(512) for s in (0, 1)]
    assert sim_index(sim, every, 3, 2, 8) == [SC.index(v, 2, 3, 8) for v in every]


@pytest.mark.parametrize("d", [1, 2, 8])
@pytest.mark.parametrize("k", [8, 128, 256, 639])
def test_rows_match_python_integers(sim, k, d):
    """the rows of the tuples word for word (values below 2^k, zero words above, sign word 0, every word written): one table,
    three, one per element; masks from every family; coefficients with set sign words and of 992 bits; windows at the bottom, across
    a word, and with t + b = k"""
    windows = [(0, 3), (30, 4) if k >= 34 else (1, 4), (k - 2, 2)]
    for t, b in windows:
        rng = random.Random(10000 * k + 100 * d + t)
        rs = SC.values(t, b, k, 6, rng)
        for n_tab in (1, 3, len(rs)):
            pieces = SC.table(b, d, k, n_tab, rng)
            got = sim_rows(sim, pieces, n_tab, rs, b, t, d, k)
            check_output(got, SC.rows(pieces, n_tab, rs, b, t, d, k), k)


@pytest.mark.parametrize("d", [1, 2, 8])
@pytest.mark.parametrize("k", [8, 128, 256, 639])
def test_powers_match_python_integers(sim, k, d):
    """e, e^2, .., e^d mod 2^k, power-major, for opened values of every family (0, 2^(k-1), whose higher powers vanish, set sign
    words, magnitudes of 2^k and above)"""
    es = SC.values(0, 1, k, 40, random.Random(77 * k + d))
    check_output(sim_powers(sim, es, d, k), SC.powers(es, d, k), k)
    assert SC.powers([(1 << (k - 1), 0)], 2, k) == [1 << (k - 1), 0]


def test_refusals(sim):
    """what the launchers refuse, decided by the function they call: bits = 0, d = 0 and 9, a tuple of more than 4096 ciphertexts,
    shift + bits > k, k = 0 and 640, no table, an element count that is no multiple of the table count: nothing written"""
    assert sim.spline_sim_max_tuple() == SC.MAX_TUPLE == 4096
    rng = random.Random(0)
    pieces = SC.table(2, 2, 8, 2, rng)
    for b, t, d, k, n_tab, n in ((0, 3, 2, 8, 1, 2), (2, 3, 0, 8, 1, 2), (2, 3, 9, 8, 1, 2), (11, 0, 2, 128, 1, 2), (12, 0, 1, 128, 1, 2),
                                 (2, 7, 2, 8, 1, 2), (2, 3, 2, 0, 1, 2), (2, 3, 2, 640, 1, 2), (2, 3, 2, 8, 0, 2), (2, 3, 2, 8, 2, 3)):
        got = sim_rows(sim, pieces, n_tab, [(1, 0)] * n, b, t, d, k, rc_want=-1)
        assert (got == FILL).all(), (b, t, d, k, n_tab, n)
    assert sim.spline_sim_check(11, 0, 1, 128, C.c_uint64(1), C.c_uint64(2)) == 0 and sim.spline_sim_check(9, 0, 7, 128, C.c_uint64(1), C.c_uint64(2)) == 0      # 4096 itself
    assert sim.spline_sim_check(2, 6, 2, 8, C.c_uint64(1), C.c_uint64(2)) == 0 and sim.spline_sim_check(2, 0, 8, 639, C.c_uint64(3), C.c_uint64(0)) == 0
    assert sim_index(sim, [(1, 0)], 0, 0, 8, rc_want=-1) == [FILL]


def test_the_sigmoid_table_stays_within_its_bound():
    """make_spline_table for the logistic sigmoid at the bench defaults (32 pieces of degree 2 over a 16-bit window on [-8, 8),
    40 fraction bits out): every x of the window outside the lowest segment, on its own piece and on the one below, lies within
    the Chebyshev interpolation bound max |g'''| (w / 2)^3 / (2^2 3!) plus the rounding term sum_i 2^((t+1) i) / 2^(out_frac + 1);
    the function is numpy's, and the builder's reported error is the test's own"""
    b, t, d, fin, fout = 5, 11, 2, 12, 40
    src = os.path.join(HERE, "hostsim", "spline_table_main.cpp")
    if _stale(_TABLE_EXE, [src, os.path.join(ROOT, "cofhe_amd", "host", "spline_table.hpp"), os.path.join(ROOT, "cofhe_amd", "host", "tensor.hpp")]):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-o", _TABLE_EXE, src])
    r = subprocess.run([_TABLE_EXE] + [str(v) for v in (b, t, d, fin, fout)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    reported = float(re.fullmatch(r"max_error (\S+)", lines[0]).group(1))
    tab = [[int(v) for v in ln.split()] for ln in lines[1:]]
    assert len(tab) == 1 << b and all(len(p) == d + 1 for p in tab)
    g = lambda x: 1.0 / (1.0 + np.exp(-x))       # noqa: E731
    w = 2.0 ** (t + 1) / 2.0 ** fin
    # g''' = g' (1 - 6 g + 6 g^2): its largest magnitude, 1/8, is at 0
    grid = np.linspace(-9.0, 9.0, 180001)
    g3 = float(np.abs(g(grid) * (1 - g(grid)) * (1 - 6 * g(grid) + 6 * g(grid) ** 2)).max())
    assert abs(g3 - 0.125) < 1e-9
    bound = g3 * (w / 2) ** 3 / (2 ** 2 * 6) + sum(2.0 ** ((t + 1) * i) for i in range(d + 1)) / 2.0 ** (fout + 1)
    worst = SC.sigmoid_table_check(tab, b, t, d, fin, fout, g)
    print("sigmoid table: worst %.3e, reported %.3e, bound %.3e" % (worst, reported, bound))
    assert worst <= bound
    assert abs(reported - worst) <= 1e-9
    # the refusals of the builder
    for bad in ((0, 11, 2, 12, 40), (5, 11, 0, 12, 40), (5, 11, 9, 12, 40), (12, 0, 1, 12, 40), (5, 60, 2, 12, 40)):
        assert subprocess.run([_TABLE_EXE] + [str(v) for v in bad], capture_output=True, text=True, timeout=60).returncode == 1


def test_the_tuples_shape_gives_bits_and_degree_or_is_refused():
    """cofhe_hip_spline_tuples_shape (host only) through Engine.spline_tuples_shape: shape S + [2^bits, d + 1] for S of 0 to 6
    dimensions; everything else is COFHE_HIP_ESHAPE and leaves *bits and *d alone; and the library exports every spline symbol
    that the header declares"""
    from cofhe_amd import load_library
    from cofhe_amd.engine import CofheHipError, Engine
    L = load_library()
    hdr = open(os.path.join(ROOT, "include", "cofhe_hip.h")).read()
    names = set(re.findall(r"\b(cofhe_hip_spline_[a-z0-9_]+)\s*\(", hdr))
    assert names == {"cofhe_hip_spline_rows_records", "cofhe_hip_spline_tuples_records", "cofhe_hip_spline_powers_records",
                     "cofhe_hip_spline_close_records", "cofhe_hip_spline_tuples_shape"}
    for n in names:
        assert hasattr(L, n), n
    eng = Engine.__new__(Engine)          # the shape check needs no GPU context
    eng.L = L
    for b in range(1, 12):
        assert eng.spline_tuples_shape([5], [5, 1 << b, 2]) == (b, 1)
    for d in range(1, 9):
        assert eng.spline_tuples_shape([2, 3], [2, 3, 4, d + 1]) == (2, d)
    assert eng.spline_tuples_shape([], [8, 3]) == (3, 2) and eng.spline_tuples_shape([0], [0, 4, 2]) == (2, 1)
    assert eng.spline_tuples_shape([1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 32, 3]) == (5, 2)
    assert eng.spline_tuples_shape([5], [5, 512, 8]) == (9, 7)                 # 4096 ciphertexts, the bound itself
    for se, st in (([5], [5, 1, 3]), ([5], [5, 12, 3]), ([5], [5, 4, 1]), ([5], [5, 4, 0]), ([5], [5, 4, 10]), ([5], [5, 1 << 12, 2]),
                   ([5], [5, 512, 9]), ([5], [5, 8]), ([5], [4, 8, 3]), ([5], [8, 3, 5]), ([5, 1], [5, 8, 3]), ([5], [5, 1, 8, 3]),
                   ([], []), ([], [8]), ([1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 1, 1, 2, 2])):
        bits, d = C.c_uint32(77), C.c_uint32(78)
        rc = L.cofhe_hip_spline_tuples_shape(C.c_uint32(len(se)), (C.c_uint32 * 8)(*se), C.c_uint32(len(st)), (C.c_uint32 * 9)(*st),
                                             C.byref(bits), C.byref(d))
        assert rc == -2 and (bits.value, d.value) == (77, 78), (se, st)
        with pytest.raises(CofheHipError) as ei:
            eng.spline_tuples_shape(se, st)
        assert ei.value.code == -2
