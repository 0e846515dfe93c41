"""CPU: the wavefront-wide layout of the latency kernels (cofhe_amd/csrc/wide.hpp: two limbs per lane over 64 lanes, carries
from two 64-bit ballots; qfw.hpp: reduction and the common route of the composition) on the host emulation, against Python
integers and the independent model oracle/pyref.py.  The GPU tier runs the same code through cofhe_hip_compose_wide_records
and the decryption ladder."""
import ctypes as C
import os
import random
import sys

import numpy as np
import pytest

from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402
import prim_cases as PC  # noqa: E402
import simlib as S8  # noqa: E402  (record packing helpers)
import simwlib as W  # noqa: E402


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def rb(rng, b):
    return rng.getrandbits(b) if b else 0


def _check_wide_lincomb(L, cases):
    groups = {}
    for A, B, x, y in cases:
        groups.setdefault((A, B), []).append((x, y))
    for (A, B), pairs in groups.items():
        xs, ys = [p[0] for p in pairs], [p[1] for p in pairs]
        r = np.zeros(128 * len(xs), dtype=np.uint32)
        s = np.zeros(128 * len(xs), dtype=np.uint32)
        top = np.zeros(2 * len(xs), dtype=np.uint32)
        L.simw_lincomb(W.P(W.pack(xs)), W.P(W.pack(ys)), C.c_uint32(A), C.c_uint32(B), W.P(r), W.P(s), W.P(top), len(xs))
        assert W.unpack(r) == [(A * a - B * b) % W.M for a, b in zip(xs, ys)], (A, B)
        assert W.unpack(s) == [(A * a + B * b) % W.M for a, b in zip(xs, ys)], (A, B)
        assert [int(t) for t in top[0::2]] == [(A * a - B * b) // W.M + B for a, b in zip(xs, ys)], (A, B)
        assert [int(t) for t in top[1::2]] == [(A * a + B * b) // W.M for a, b in zip(xs, ys)], (A, B)


def _check_wide_shifts(L, cases):
    groups = {}
    for sh, v in cases:
        groups.setdefault(sh, []).append(v)
    for sh, vals in groups.items():
        l = np.zeros(128 * len(vals), dtype=np.uint32)
        r = np.zeros(128 * len(vals), dtype=np.uint32)
        bits = np.zeros(len(vals), dtype=np.int32)
        L.simw_shift(W.P(W.pack(vals)), sh, W.P(l), W.P(r), bits.ctypes.data_as(C.POINTER(C.c_int)), len(vals))
        assert W.unpack(l) == [(a << sh) % W.M for a in vals], sh
        assert W.unpack(r) == [a >> sh for a in vals], sh
        assert [int(b) for b in bits] == [a.bit_length() for a in vals]


def test_wide_mul_lincomb_shift():
    L = W.lib()
    xs, ys, lin, shifts, cmps = PC.wide_mul_lincomb_shift_cases()
    out = np.zeros(128 * len(xs), dtype=np.uint32)
    L.simw_mul(W.P(W.pack(xs)), W.P(W.pack(ys)), W.P(out), len(xs))
    assert W.unpack(out) == [(a * b) % W.M for a, b in zip(xs, ys)]
    _check_wide_lincomb(L, lin)
    _check_wide_shifts(L, shifts)
    for a, b in cmps:
        assert L.simw_cmp(W.P(W.pack([a])), W.P(W.pack([b]))) == (a > b) - (a < b)


def test_wide_row_edges_and_capacity():
    """2^4096 - 1 + 1 and 2^4096 - 1 - x, hand-over words and propagate runs across the row edges of the wavefront (lanes
    15|16, 31|32, 47|48), shifts that move even and odd limb counts up to the top of the capacity"""
    L = W.lib()
    _check_wide_lincomb(L, PC.wide_lincomb_edge_cases())
    _check_wide_shifts(L, PC.wide_shift_edge_cases())


def test_wide_remainder_sequence():
    """qfw.hpp: w_euclid -- both lengths and both windows of a round come from ONE view of the pair's leading lanes
    (wide.hpp: w_top_pair) and the batch is the single-chain form: pairs of equal length, pairs far apart (the shorter
    number ends below the view), equal numbers, powers of two, a zero, single words, full and partial sequences.
    Invariants: x == sx ux y0, y == sy uy y0 (mod x0); the gcd is kept; x >= y; a full sequence ends at y == 0, a partial
    one with the first remainder at or below its stop"""
    from math import gcd
    L = W.lib()
    cases = PC.wide_euclid_cases()
    out, sg = np.zeros(512, dtype=np.uint32), np.zeros(2, dtype=np.int32)
    for x0, y0, stop in cases:
        ok = L.simw_euclid(W.P(W.pack([x0])), W.P(W.pack([y0])), stop, W.P(out), sg.ctypes.data_as(C.POINTER(C.c_int)))
        assert ok == 1, (x0, y0, stop)
        x, y, ux, uy = (W.unpack(out[128 * k:128 * (k + 1)])[0] for k in range(4))
        sx, sy = int(sg[0]), int(sg[1])
        assert x >= y and gcd(x, y) == gcd(x0, y0), (x0, y0, stop)
        if x0:
            assert (x - sx * ux * y0) % x0 == 0 and (y - sy * uy * y0) % x0 == 0, (x0, y0, stop)
        if stop < 0:
            assert y == 0
        else:
            assert y.bit_length() <= stop or y == 0
            assert x.bit_length() > stop or max(x0, y0).bit_length() <= stop or min(x0, y0).bit_length() <= stop, (x0, y0, stop)
    assert W.lib().simw_status() == 0


def test_wide_divisions():
    L = W.lib()
    cases, exact, nql = PC.wide_division_cases()
    rem = np.zeros(128 * len(cases), dtype=np.uint32)
    assert L.simw_mod(W.P(W.pack([c[0] for c in cases])), W.P(W.pack([c[1] for c in cases])), W.P(rem), len(cases)) == 1
    assert W.unpack(rem) == [n % d for n, d in cases]
    # exact division, 2-adic with 64-bit digits
    cases = exact
    nq = np.array(nql, dtype=np.int32)
    quo = np.zeros(128 * len(cases), dtype=np.uint32)
    assert L.simw_divexact(W.P(W.pack([c[0] for c in cases])), W.P(W.pack([c[1] for c in cases])), nq.ctypes.data_as(C.POINTER(C.c_int)),
                           W.P(quo), len(cases)) == 1
    assert W.unpack(quo) == [c[2] for c in cases]
    # a divisor whose low 64 bits are zero is declined (the composition then takes the 8-lane route)
    assert L.simw_divexact(W.P(W.pack([3 << 64])), W.P(W.pack([1 << 64])), np.array([1], dtype=np.int32).ctypes.data_as(C.POINTER(C.c_int)),
                           W.P(quo), 1) == 0


def _compose_w(pairs, d):
    L = W.lib()
    half = ((-d).bit_length() + 1) // 2
    n = len(pairs)
    f1 = np.concatenate([S8.form_record(a.a, a.b, a.c) for a, _ in pairs])
    f2 = np.concatenate([S8.form_record(b.a, b.b, b.c) for _, b in pairs])
    out = np.zeros(n * S8.REC_WORDS, dtype=np.uint32)
    fl = np.zeros(n, dtype=np.int32)
    L.simw_compose(S8.P(f1), S8.P(f2), S8.P(out), fl.ctypes.data_as(C.POINTER(C.c_int)), n, half, S8.P(S8.to_limbs(-d, 80)))
    return [S8.record_form(out[i * S8.REC_WORDS:(i + 1) * S8.REC_WORDS]) for i in range(n)], fl


@pytest.mark.parametrize("name", ["s128_k128", "s128_k256", "tiny_k8"])
def test_wide_composition_against_the_model(name):
    """wf_compose on random pairs, squarings, a ladder-like chain (the common route: taken for all but a few per cent --
    pairs that keep a common factor after the coprime-representative step) and on the lopsided pool (short first
    coefficients, inverse pairs, the identity: mostly declined).  Whatever it accepts must equal the independent model;
    what it declines is left untouched for the 8-lane route, which the GPU tier exercises."""
    from lopsided import lopsided_pool
    prm = load_json("params_%s.json" % name)
    d, k = hx(prm["delta"]), prm["k"]
    rng = P.SplitMix64(199)
    pool = [P.random_form(d, rng) for _ in range(40)]
    pairs = [(pool[rng.below(40)], pool[rng.below(40)]) for _ in range(300)] + [(x, x) for x in pool]
    f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    lop = lopsided_pool(d, k, f)
    pairs += [(lop[rng.below(len(lop))], lop[rng.below(len(lop))]) for _ in range(100)]
    x, chain = pool[0], []
    for i in range(60):
        y = x if i % 3 else pool[1 + i % 7]
        chain.append((x, y))
        x = P.compose(x, y)
    pairs += chain + [(P.identity(d), pool[0]), (pool[1], P.identity(d)), (pool[2], P.inverse(pool[2]))]
    got, fl = _compose_w(pairs, d)
    for g, (a, b), flag in zip(got, pairs, fl):
        if not flag:
            w = P.compose(a, b)
            assert tuple(g) == (w.a, w.b, w.c)
    assert fl[:300].sum() <= 30 and fl[300:340].sum() == 0 and fl[440:500].sum() <= 6        # random pairs, squarings, the chain
    assert W.lib().simw_status() == 0
