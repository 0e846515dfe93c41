"""CPU: the one-plane tail of the composition -- mp_mul_half2 and mp_sqr_low (cofhe_amd/csrc/mp.hpp), nucomp_ab and nucomp_c
on both of their routes (cofhe_amd/csrc/qf.hpp) -- compiled for the host (tests/hostsim/onep_sim.cpp: the 8 lanes of a limb
group as 8 threads), against Python integers.  The cases are tests/onep_cases.py, shared with the GPU tier.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import onep_cases as OC
import simlib as S
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libonepsim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "onep_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("lane.hpp", "mp.hpp", "qf.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.onep_sim_status.restype = C.c_uint
    L.onep_sim_c_serves.argtypes = [C.c_int, C.c_uint32]
    assert L.onep_sim_compiled_in() == 3
    return L


def run(fn, sim, recs, out_words):
    ins = np.concatenate(recs)
    out = np.full(len(recs) * out_words, 0xA5A5A5A5, dtype=np.uint32)
    fn(S.P(ins), S.P(out), len(recs))
    assert sim.onep_sim_status() == 0
    return out.reshape(len(recs), out_words)


def test_mul_half2_matches_python_integers(sim):
    """both full products, each in a plane of its own; limbs 20..39 of the operands do not matter"""
    cases = OC.mul_cases()
    out = run(sim.onep_sim_mul, sim, [OC.pack_mul(c) for c in cases], OC.MUL_OUT)
    for i, (c, rec) in enumerate(zip(cases, out)):
        assert np.array_equal(rec, OC.expected_mul(c)), i


def test_mul_cases_cover_what_they_claim():
    cases = OC.mul_cases()
    lens = {OC.bl(c[0] % OC.HALF) for c in cases} | {OC.bl(c[3] % OC.HALF) for c in cases}
    assert set(OC.MUL_LENGTHS) <= lens
    ones = OC.HALF - 1
    assert (ones, ones, ones, ones) in cases
    assert any(c[0] * c[1] == 0 and c[2] * c[3] != 0 for c in cases) and any(c[0] * c[1] != 0 and c[2] * c[3] == 0 for c in cases)
    assert any(c[0] >= OC.HALF and c[3] >= OC.HALF for c in cases)                     # garbage above limb 19
    prods = [(c[0] % OC.HALF) * (c[1] % OC.HALF) for c in cases]
    assert any(p and p & (p + 1) == 0 and OC.bl(p) >= 640 for p in prods)               # all ones over four chunks and more
    assert any(p and OC.tz(p) >= 639 for p in prods)


def test_sqr_low_matches_python_integers(sim):
    cases = OC.sqr_cases()
    assert OC.PLANE - 1 in cases and (1 << 640) in cases and any(x and (x * x) % OC.PLANE == 0 for x in cases)
    assert any(((x * x) % OC.PLANE) >> 161 == (1 << 1119) - 1 for x in cases)           # a run of ones through seven chunks
    out = run(sim.onep_sim_sqr, sim, [S.to_limbs(x, 40) for x in cases], OC.SQR_OUT)
    for i, (x, rec) in enumerate(zip(cases, out)):
        assert np.array_equal(rec, OC.expected_sqr(x)), i


def test_ab_both_routes_match_python_integers(sim):
    """a' and b' equal Python's on whichever route the bound sends the group, and the route is the one the bound says"""
    named = OC.ab_cases()
    out = run(sim.onep_sim_ab, sim, [OC.pack_ab(c) for _, c in named], OC.AB_OUT)
    for (name, c), rec in zip(named, out):
        an, bn, one = OC.unpack_ab(rec)
        assert (an, bn) == OC.ab_expected(c), name
        assert one == (1 if OC.ab_one_plane(c) else 0), name


def test_c_both_routes_match_python_integers(sim):
    named = OC.c_cases()
    out = run(sim.onep_sim_c, sim, [OC.pack_c(c) for _, c in named], OC.C_OUT)
    for (name, c), rec in zip(named, out):
        cn, low = OC.unpack_c(rec)
        assert cn == OC.c_expected(c), name
        assert low == (1 if OC.c_low(c) else 0), name


def test_case_lists_cover_what_they_claim():
    ab = OC.ab_cases()
    by = {}
    for n, c in ab:
        by.setdefault(n, []).append(c)
    assert {"signs", "cancel", "op640", "op641", "prod1277", "prod1278", "b1_1279", "b1_1280", "no rounds", "m2 two planes", "two-plane ab"} <= set(by)
    # real compositions of every parameter set: random pairs, squarings, a form with its inverse, powers of f
    assert {"%s %s" % (p, k) for p in ("tiny_k8", "s128_k128", "s128_k256") for k in ("random", "squaring", "inverse", "f power")} <= set(by)
    sg = lambda v: (v > 0) - (v < 0)
    assert {(sg(c[1]), sg(c[4]), sg(c[5])) for c in by["signs"] if OC.ab_one_plane(c)} == {(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)}
    assert any(OC.ab_expected(c)[0] == 0 for c in by["cancel"]) and any(0 < abs(OC.ab_expected(c)[0]) < 1 << 700 for c in by["cancel"])
    assert all(OC.ab_one_plane(c) for c in by["op640"] + by["prod1277"] + by["b1_1279"])
    assert not any(OC.ab_one_plane(c) for c in by["op641"] + by["prod1278"] + by["b1_1280"] + by["no rounds"] + by["m2 two planes"] + by["two-plane ab"])
    assert any(max(OC.bl(v) for v in OC.ab_expected(c)) > 1280 for c in by["two-plane ab"])
    assert any(OC.bl(OC.ab_expected(c)[1]) == 1280 for c in by["b1_1279"])               # b' fills the plane on the one-plane route
    # real operands of the 2088-bit discriminant take the new routes: random pairs and squarings at the composition's own
    # stopping point do, the same pairs after no rounds do not; a form with its inverse never does: with the representative
    # (c, -b, a) it ends at a' = 1 under a full-plane R0, without one (c beyond the representative's range) a' has two planes
    for p in ("s128_k128", "s128_k256"):
        assert sum(1 for c in by[p + " random"] if OC.ab_one_plane(c)) >= 4 and any(not OC.ab_one_plane(c) for c in by[p + " random"])
        assert sum(1 for c in by[p + " squaring"] if OC.ab_one_plane(c)) >= 2 and any(not OC.ab_one_plane(c) for c in by[p + " squaring"])
        assert not any(OC.ab_one_plane(c) for c in by[p + " inverse"])
    assert all(OC.ab_expected(c)[0] == 1 for c in by["s128_k128 inverse"])
    assert all(OC.bl(OC.ab_expected(c)[0]) > 1280 for c in by["s128_k256 inverse"])
    cs = OC.c_cases()
    cby = {}
    for n, c in cs:
        cby.setdefault(n, []).append(c)
    assert {OC.tz(c[0]) for _, c in cs if OC.c_low(c)} >= {0, 1, 31} and all(OC.tz(c[0]) == 32 and not OC.c_low(c) for c in cby["tz32"])
    for t in (0, 5):
        assert all(OC.c_bound(c) + 2 + t == 1280 and OC.c_low(c) for c in cby["edge1280 tz%d" % t])
        assert all(OC.c_bound(c) + 2 + t == 1281 and not OC.c_low(c) for c in cby["edge1281 tz%d" % t])
    assert sum(1 for c in cby["s128_k128 random"] if OC.c_low(c)) >= 4 and any(OC.c_low(c) for c in cby["s128_k128 squaring"])
    assert any(OC.c_low(c) for c in cby["s128_k256 squaring"]) and "s128_k128 f power" in cby
    assert any(OC.c_expected(c) >= OC.PLANE for _, c in cs)


def test_predicates_at_the_boundary(sim):
    for args, want in (((640, 640, 637, 637), 1), ((641, 1, 1, 1), 0), ((1, 641, 1, 1), 0), ((1, 1, 641, 1), 0), ((1, 1, 1, 641), 0),
                       ((640, 0, 638, 0), 0), ((0, 640, 0, 638), 0), ((639, 640, 638, 637), 1), ((0, 0, 0, 0), 1)):
        assert sim.onep_sim_dot_serves(*args) == want == (1 if max(args) <= 640 and args[0] + args[2] <= 1277 and args[1] + args[3] <= 1277 else 0)
    for args in ((1044, 2088, 1043), (10, 2087, 1044), (889, 100, 500), (0, 2088, 1)):
        assert sim.onep_sim_c_bound(*args) == max(2 * args[0], args[1]) - args[2]
    for t in range(32):
        w = (0x9E3779B1 >> t << t | (1 << t)) & 0xFFFFFFFF
        assert OC.tz(w) == t
        assert sim.onep_sim_c_serves(1278 - t, w) == 1 and sim.onep_sim_c_serves(1279 - t, w) == 0
    assert sim.onep_sim_c_serves(100, 0) == 0 and sim.onep_sim_c_serves(0, 1) == 0 and sim.onep_sim_c_serves(1, 1) == 1
