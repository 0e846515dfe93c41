"""CPU: the low-half products (cofhe_amd/csrc/mp.hpp: mp_mul_low2) and nucomp_m12 on both of its routes
(cofhe_amd/csrc/qf.hpp) compiled for the host (tests/hostsim/lowmul_sim.cpp: the 8 lanes of a limb group as 8 threads),
against Python integers.  The cases are tests/lowmul_cases.py, shared with the GPU tier.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lowmul_cases as LC
import simlib as S
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "liblowmulsim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "lowmul_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("lane.hpp", "mp.hpp", "qf.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.lowmul_sim_status.restype = C.c_uint
    L.lowmul_sim_serves.argtypes = [C.c_int, C.c_uint32]
    assert L.lowmul_sim_compiled_in() == 1
    return L


def run_m12(sim, cases, try_low):
    ins = np.concatenate([LC.pack_m12(c, try_low) for c in cases])
    out = np.full(len(cases) * LC.M12_OUT, 0xA5A5A5A5, dtype=np.uint32)
    sim.lowmul_sim_m12(S.P(ins), S.P(out), len(cases))
    assert sim.lowmul_sim_status() == 0
    return [LC.unpack_m12(r) for r in out.reshape(len(cases), LC.M12_OUT)]


def test_mul_low2_matches_python_integers(sim):
    """both products modulo 2^640, each in its half of the group; limbs 20..39 of the operands do not matter"""
    cases = LC.mul_cases()
    ins = np.concatenate([LC.pack_mul(c) for c in cases])
    out = np.full(len(cases) * LC.MUL_OUT, 0xA5A5A5A5, dtype=np.uint32)
    sim.lowmul_sim_mul(S.P(ins), S.P(out), len(cases))
    for i, (c, rec) in enumerate(zip(cases, out.reshape(len(cases), LC.MUL_OUT))):
        assert np.array_equal(rec, LC.expected_mul(c)), i


def test_m12_both_routes_match_python_integers(sim):
    """the same inputs through the low-half route (where the bound allows it) and through the full products: M1 and M2
    equal Python's exact quotients on both, and the route taken is the one the bound says"""
    named = LC.m12_cases()
    cases = [c for _, c in named]
    want = [LC.expected(c) for c in cases]
    for try_low in (1, 0):
        got = run_m12(sim, cases, try_low)
        for (name, c), (M1, M2, low), w in zip(named, got, want):
            assert (M1, M2) == w, (name, try_low)
            assert low == (1 if try_low and LC.low_route(c) else 0), (name, try_low)


def test_case_list_covers_what_it_claims():
    named = LC.m12_cases()
    cases = [c for _, c in named]
    names = {n for n, _ in named}
    assert {"tiny_k8", "s128_k128", "s128_k256", "largest", "below", "above", "C=1", "two planes"} <= names
    signs = {(c[1] < 0, c[4] < 0, c[5] < 0) for c in cases if LC.low_route(c)}
    assert len(signs) == 8                                              # every sign combination of C, m, s on the low route
    ms = [LC.expected(c) for c in cases if LC.low_route(c)]
    for k in (0, 1):
        assert any(m[k] == 0 for m in ms) and any(m[k] > 0 for m in ms) and any(m[k] < 0 for m in ms)
    assert {LC.tz(c[2]) for c in cases if LC.low_route(c)} >= {0, 1, 31} and any(LC.tz(c[2]) >= 32 for c in cases)
    assert any(abs(LC.expected(c)[1]) >= LC.PLANE for c in cases)       # an M2 of two planes
    assert any(not LC.low_route(c) for n, c in named if n in ("tiny_k8", "s128_k128", "s128_k256"))
    assert any(LC.low_route(c) for n, c in named if n == "s128_k256")


def test_bound_and_predicate_at_the_boundary(sim):
    """m12_bound against its formula; m12_low_half_serves flips exactly between nb + 1 + tz == 640 and 641 for every tz
    below 32 and refuses a limb 0 of zero (32 or more trailing zero bits)"""
    for args in ((1040, 522, 1043, 520, 1044), (5, 5, 700, 600, 40), (1, 1, 1, 1, 900), (319, 319, 319, 319, 1), (0, 0, 0, 0, 1)):
        assert sim.lowmul_sim_bound(*args) == LC.bound(*args)
    for t in range(32):
        w = (0x9E3779B1 >> t << t | (1 << t)) & 0xFFFFFFFF
        assert LC.tz(w) == t
        assert sim.lowmul_sim_serves(639 - t, w) == 1 and sim.lowmul_sim_serves(640 - t, w) == 0
        assert sim.lowmul_sim_serves(0, w) == 1
    assert sim.lowmul_sim_serves(0, 0) == 0 and sim.lowmul_sim_serves(100, 0) == 0
    by_name = dict(LC.m12_cases())
    assert LC.low_route(by_name["edge640 tz0"]) and LC.low_route(by_name["edge640 tz3"]) and LC.low_route(by_name["edge m637"])
    assert not (LC.low_route(by_name["edge641 tz0"]) or LC.low_route(by_name["edge641 tz3"]) or LC.low_route(by_name["edge m638"]))
