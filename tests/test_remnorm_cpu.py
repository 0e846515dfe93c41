"""CPU: the remainder-only long division (cofhe_amd/csrc/mp.hpp: mp_rem_norm with mp_lincomb_sub_carry_sparse) and the step
r = y1 m mod a1 of the composition (qf.hpp: smod with its remainder-only flag), compiled for the host
(tests/hostsim/remnorm_sim.cpp: the 8 lanes of a limb group as 8 threads), against Python integers and against the remainder
of mp_divrem_norm.  The cases are tests/remnorm_cases.py, shared with the GPU tier.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import remnorm_cases as RC
import simlib as S
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libremnormsim.so")
OP_REM2, OP_DIVREM2, OP_REM1, OP_STEP = range(4)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "remnorm_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("lane.hpp", "mp.hpp", "qf.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.remnorm_sim_status.restype = C.c_uint
    assert L.remnorm_sim_compiled_in() == 1
    return L


def run(sim, op, packed):
    io = (C.c_int * 2)()
    assert sim.remnorm_sim_words(op, io) == 0
    ins = np.concatenate(packed)
    assert len(ins) == len(packed) * io[0]
    out = np.full(len(packed) * io[1], 0xA5A5A5A5, dtype=np.uint32)
    assert sim.remnorm_sim_run(op, S.P(ins), S.P(out), len(packed)) == 0
    assert sim.remnorm_sim_status() == 0
    return out.reshape(len(packed), io[1])


def stats(sim):
    st = (C.c_long * 3)()
    sim.remnorm_sim_stats(st)
    return tuple(st)


def test_the_required_cases_are_in_the_list():
    names = {n for n, _ in RC.rem_cases()}
    assert set(RC.REQUIRED) <= names, set(RC.REQUIRED) - names
    kinds = {n.split(" ", 1)[1] for n, _ in RC.step_cases() if n.split(" ", 1)[0] in ("tiny_k8", "s128_k128", "s128_k256")}
    assert set(RC.STEP_KINDS) <= kinds, kinds


def test_rem_norm_matches_python_integers_and_takes_its_rare_paths(sim):
    """every case: num mod den, the upper plane zero.  Over the list the add-back ran and the general carry resolve ran, by the
    simulator's own counters; digit by digit they are the counts the Python model of the division announces"""
    named = RC.rem_cases()
    stats(sim)
    out = run(sim, OP_REM2, [RC.pack_rem(c) for _, c in named])
    digits, addbacks, general = stats(sim)
    for (name, (num, den)), rec in zip(named, out):
        assert S.from_limbs(rec) == num % den, name
    assert addbacks >= 1, "no case reached the add-back of mp_rem_norm"
    assert general >= 1, "no case reached the general carry resolve of mp_rem_norm"
    mo = [RC.model(*c) for _, c in named]
    assert (digits, addbacks) == (sum(m[1] for m in mo), sum(m[2] for m in mo))
    assert general == sum(m[3] for m in mo)
    # a case of the general resolve that is not an add-back: alone
    alone = [c for n, c in named if n.startswith("limb 1 all ones, lane")]
    for c in alone:
        assert S.from_limbs(run(sim, OP_REM2, [RC.pack_rem(c)])[0]) == c[0] % c[1]
        _, a, g = stats(sim)
        assert a == 0 and g >= 1


def test_rem_norm_equals_the_remainder_of_divrem_norm(sim):
    named = RC.rem_cases()
    packed = [RC.pack_rem(c) for _, c in named]
    a, b = run(sim, OP_REM2, packed), run(sim, OP_DIVREM2, packed)
    for (name, _), x, y in zip(named, a, b):
        assert np.array_equal(x, y), name


def test_rem_norm_one_plane(sim):
    named = RC.rem1_cases()
    assert len(named) >= 10
    out = run(sim, OP_REM1, [RC.pack_rem1(c) for _, c in named])
    for (name, (num, den)), rec in zip(named, out):
        assert S.from_limbs(rec) == num % den, name


def test_whole_steps(sim):
    """r = y1 m mod a1 as qf_compose computes it: the product, the remainder, the sign rule"""
    named = RC.step_cases()
    out = run(sim, OP_STEP, [RC.pack_step(c) for _, c in named])
    for (name, c), rec in zip(named, out):
        assert S.from_limbs(rec) == RC.step_expected(c), name
