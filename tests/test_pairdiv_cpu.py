"""CPU: the paired 2-adic division (cofhe_amd/csrc/mp.hpp: mp_divexact_pair; qf.hpp: m12_low_quot_pair), mp_divexact with a
one-plane numerator, mp_sqr_low from every chunk pair once, and whole compositions through nucomp_m12, nucomp_ab and nucomp_c,
compiled for the host (tests/hostsim/pairdiv_sim.cpp: the 8 lanes of a limb group as 8 threads), against Python integers.
The cases are tests/pairdiv_cases.py, shared with the GPU tier.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lowmul_cases as LC
import onep_cases as OC
import pairdiv_cases as PC
import simlib as S
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libpairdivsim.so")
OP_DIVP, OP_QUOTP, OP_DIVX, OP_SQR, OP_M12, OP_AB, OP_C = range(7)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "pairdiv_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("lane.hpp", "mp.hpp", "qf.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.pairdiv_sim_status.restype = C.c_uint
    assert L.pairdiv_sim_compiled_in() == 7
    return L


def run(sim, op, packed):
    io = (C.c_int * 2)()
    assert sim.pairdiv_sim_words(op, io) == 0
    ins = np.concatenate(packed)
    assert len(ins) == len(packed) * io[0]
    out = np.full(len(packed) * io[1], 0xA5A5A5A5, dtype=np.uint32)
    assert sim.pairdiv_sim_run(op, S.P(ins), S.P(out), len(packed)) == 0
    assert sim.pairdiv_sim_status() == 0
    return out.reshape(len(packed), io[1])


def test_divexact_pair_matches_python_integers(sim):
    """both halves' digits against the 2-adic quotient modulo 2^(32 nq); the limbs from nq on are zero; an all-ones chunk 3 of
    half 0 leaves half 1 alone"""
    cases = PC.divp_cases()
    out = run(sim, OP_DIVP, [PC.pack_divp(c) for c in cases])
    for i, (c, rec) in enumerate(zip(cases, out)):
        assert np.array_equal(rec, PC.divp_expected(c)), i


def test_quot_pair_matches_python_integers(sim):
    """sign and magnitude of both quotients: digit counts 1 | 20, 20 | 1, odd, even; a zero quotient by its bound in one half;
    0 and 31 trailing zero bits; one negative half; the sign bit at bit 0 and bit 31 of its limb; nb + 1 + tz == 640"""
    named = PC.quotp_cases() + PC.quotp_raw_cases()
    names = {n for n, _ in named}
    assert {"digits 1 20", "digits 20 1", "digits odd", "digits even", "nb<0 half 0", "nb<0 half 1", "tz0", "tz31", "neg half 0", "neg half 1",
            "nb&31", "edge640 tz0", "edge640 tz31", "chunk 3 ones", "all ones"} <= names
    out = run(sim, OP_QUOTP, [PC.pack_quotp(c) for _, c in named])
    for (name, c), rec in zip(named, out):
        assert PC.unpack_quotp(rec) == PC.quotp_model(c), name


def test_divexact_one_plane_without_high_limbs(sim):
    """quotients of 1, 2, 39 and 40 limbs of exact numerators; a numerator cut modulo 2^1280 gives the low nbc bits"""
    named = PC.divx_cases()
    out = run(sim, OP_DIVX, [PC.pack_divx(c) for _, c in named])
    for (name, c), rec in zip(named, out):
        got = S.from_limbs(rec)
        assert got < 1 << (32 * c[2]), name
        assert got % (1 << c[3]) == PC.divx_expected(c) % (1 << c[3]), name


def test_sqr_low_matches_python_integers(sim):
    cases = PC.sqr_cases()
    out = run(sim, OP_SQR, [S.to_limbs(x, 40) for x in cases])
    for i, (x, rec) in enumerate(zip(cases, out)):
        assert np.array_equal(rec, OC.expected_sqr(x)), i


def test_whole_compositions(sim):
    """the operands of real compositions of the three parameter sets through nucomp_m12, nucomp_ab and nucomp_c: exact
    results, and the route each bound announces for the group alone"""
    m12, ab, cc = PC.composition_cases()
    kinds = {n.split(" ", 1)[1] for n, _ in ab}
    assert kinds == {"random", "squaring", "inverse", "f power"} and any(LC.low_route(c) for _, c in m12)
    out = run(sim, OP_M12, [LC.pack_m12(c, 1) for _, c in m12])
    for (name, c), rec in zip(m12, out):
        M1, M2, low = LC.unpack_m12(rec)
        assert (M1, M2) == LC.expected(c), name
        assert low == (1 if LC.low_route(c) else 0), name
    out = run(sim, OP_AB, [OC.pack_ab(c) for _, c in ab])
    for (name, c), rec in zip(ab, out):
        an, bn, one = OC.unpack_ab(rec)
        assert (an, bn) == OC.ab_expected(c), name
        assert one == (1 if OC.ab_one_plane(c) else 0), name
    out = run(sim, OP_C, [OC.pack_c(c) for _, c in cc])
    for (name, c), rec in zip(cc, out):
        cn, low = OC.unpack_c(rec)
        assert cn == OC.c_expected(c), name
        assert low == (1 if OC.c_low(c) else 0), name


def test_bound_of_641_takes_the_full_products(sim):
    """nb + 1 + tz == 640 is served by the paired division, 641 is not: the same quotients from the full products"""
    by_name = dict(LC.m12_cases())
    for name, low in (("edge640 tz0", 1), ("edge640 tz3", 1), ("edge m637", 1), ("edge641 tz0", 0), ("edge641 tz3", 0), ("edge m638", 0)):
        c = by_name[name]
        M1, M2, got = LC.unpack_m12(run(sim, OP_M12, [LC.pack_m12(c, 1)])[0])
        assert (M1, M2) == LC.expected(c) and got == low, name
