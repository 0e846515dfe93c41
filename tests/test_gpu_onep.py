"""GPU: the one-plane tail of the composition -- mp_mul_half2 and mp_sqr_low (cofhe_amd/csrc/mp.hpp), nucomp_ab and nucomp_c
on both of their routes (cofhe_amd/csrc/qf.hpp) -- on the MI355X against Python integers.  tests/gpu_kernels/onep_gpu.hip
compiles the product headers into small kernels of its own (built by __graft_entry__.build() into libonep_gpu.so); the cases
are those of the CPU tier (tests/onep_cases.py).

Every case list runs in the three arrangements of tests/test_gpu_lowmul.py, each compared with Python integer arithmetic and
never with another arrangement or route: `solo` (the case in slot i % 8 of a wavefront whose other seven groups are switched
off), `uniform` (all eight groups hold the same case) and `mixed` (the list shuffled with a fixed seed and dealt eight
distinct cases to a wavefront, once per rotation 0..7, the last wavefront partly filled).  The route decisions are ballots over
the wavefront: a group reports the new route exactly when every live group of its wavefront is within the bound, and its
results are right on whichever route that made it take."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import onep_cases as OC
import simlib as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

OP_MUL, OP_SQR, OP_AB, OP_C = 0, 1, 2, 3
U32 = C.POINTER(C.c_uint32)
CHUNK = 40                       # cases per solo / uniform launch: 320 groups
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "tests", "gpu_kernels", "libonep_gpu.so")
        assert os.path.exists(so), "tests/gpu_kernels/libonep_gpu.so is built by __graft_entry__.build()"
        import torch  # noqa: F401  (PyTorch's HIP runtime first)
        torch.cuda.init()
        _lib = C.CDLL(so)
        assert _lib.onep_gpu_compiled_in() == 3
    return _lib


def run_groups(op, recs, active):
    io = (C.c_int * 2)()
    assert lib().onep_gpu_words(op, io) == 0
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, io[0]) and len(active) == n
    act = np.ascontiguousarray(active, dtype=np.uint8)
    out = np.zeros((n, io[1]), dtype=np.uint32)
    st = C.c_uint32(0xFFFFFFFF)
    rc = lib().onep_gpu_run(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), act.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(st))
    assert rc == 0, "onep_gpu_run(%d) returned %d" % (op, rc)
    return out, st.value


def arrangements(n):
    """(name, slots): slots[g] = index of the case in group g of the launch, -1 for a group that is switched off"""
    for lo in range(0, n, CHUNK):
        idx = np.arange(lo, min(n, lo + CHUNK))
        solo = np.full(8 * len(idx), -1, dtype=np.int64)
        solo[[8 * i + i % 8 for i in range(len(idx))]] = idx
        yield "solo", solo
        yield "uniform", np.repeat(idx, 8)
    order = list(range(n))
    random.Random(20261020).shuffle(order)
    if n % 8 == 0:
        order += order[:3]                       # the last wavefront stays partly filled
    for rot in range(8):
        o = order[rot:] + order[:rot]
        slots = np.full(8 * ((len(o) + 7) // 8), -1, dtype=np.int64)
        slots[:len(o)] = o
        yield "mixed%d" % rot, slots


def run_arranged(op, ins, check):
    """ins[n, IN]: the packed cases; check(i, record, slots of the live groups of the wavefront, where).  The groups that
    were switched off must have written nothing; the status word must be clear after every launch."""
    ins = np.asarray(ins, dtype=np.uint32)
    for name, slots in arrangements(len(ins)):
        recs = np.zeros((len(slots), ins.shape[1]), dtype=np.uint32)
        live = slots >= 0
        recs[live] = ins[slots[live]]
        out, st = run_groups(op, recs, live)
        assert st == 0, (name, st)
        assert not out[~live].any(), name
        for g in np.nonzero(live)[0]:
            w = slots[8 * (g // 8):8 * (g // 8) + 8]
            check(int(slots[g]), out[g], [int(x) for x in w if x >= 0], (name, int(g)))


def test_mul_half2():
    cases = OC.mul_cases()
    exp = [OC.expected_mul(c) for c in cases]

    def check(i, rec, _wave, where):
        assert np.array_equal(rec, exp[i]), (where, i)
    run_arranged(OP_MUL, [OC.pack_mul(c) for c in cases], check)


def test_sqr_low():
    cases = OC.sqr_cases()
    exp = [OC.expected_sqr(x) for x in cases]

    def check(i, rec, _wave, where):
        assert np.array_equal(rec, exp[i]), (where, i)
    run_arranged(OP_SQR, [S.to_limbs(x, 40) for x in cases], check)


@pytest.fixture(scope="module")
def ab():
    named = OC.ab_cases()
    return named, [OC.ab_expected(c) for _, c in named], [OC.ab_one_plane(c) for _, c in named], [bool(c[7]) for _, c in named]


@pytest.fixture(scope="module")
def cc():
    named = OC.c_cases()
    return named, [OC.c_expected(c) for _, c in named], [OC.c_low(c) for _, c in named]


def test_ab_in_three_arrangements(ab):
    """a', b' against Python's; the route is the verdict of the groups that vote.  In the product m2_one_plane is uniform over
    the wavefront (nucomp_m12's own ballot); here every group brings its own flag, a group without it goes to the double-width
    dots before the ballot and is not among the lanes that vote."""
    named, want, ok, flag = ab

    def check(i, rec, wave, where):
        an, bn, one = OC.unpack_ab(rec)
        assert (an, bn) == want[i], (where, named[i][0])
        assert one == (1 if flag[i] and all(ok[j] for j in wave if flag[j]) else 0), (where, named[i][0])
    run_arranged(OP_AB, [OC.pack_ab(c) for _, c in named], check)


def test_c_in_three_arrangements(cc):
    """c' against Python's exact quotient; the route is the wavefront's verdict"""
    named, want, ok = cc

    def check(i, rec, wave, where):
        cn, low = OC.unpack_c(rec)
        assert cn == want[i], (where, named[i][0])
        assert low == (1 if all(ok[j] for j in wave) else 0), (where, named[i][0])
    run_arranged(OP_C, [OC.pack_c(c) for _, c in named], check)


def one_outside(named, ok, outside_names, votes=None):
    """slots of eight wavefronts of seven groups within the bound and one outside it, in slot w of wavefront w, and a ninth
    wavefront with all eight within; votes[i]: the case takes part in the ballot (all do when None)"""
    inside = [i for i in range(len(named)) if ok[i]]
    outside = [i for i, (n, _) in enumerate(named) if n in outside_names and not ok[i] and (votes is None or votes[i])]
    assert len(inside) >= 15 and len(outside) >= 8
    slots = []
    for w in range(8):
        row = [inside[(7 * w + k) % len(inside)] for k in range(7)]
        row.insert(w, outside[w])
        slots += row
    return slots + inside[7:15]


def test_one_group_outside_a_bound_takes_its_wavefront_along(ab, cc):
    """only the ninth wavefront reports the new route, every result is right"""
    named, want, ok, flag = ab
    slots = one_outside(named, ok, ("two-plane ab", "no rounds", "b1_1280", "prod1278", "op641"), flag)
    out, st = run_groups(OP_AB, np.stack([OC.pack_ab(named[i][1]) for i in slots]), np.ones(len(slots), dtype=np.uint8))
    assert st == 0
    for g, i in enumerate(slots):
        an, bn, one = OC.unpack_ab(out[g])
        assert (an, bn) == want[i], (g, named[i][0])
        assert one == (1 if g >= 64 else 0), (g, named[i][0])
    named, want, ok = cc
    slots = one_outside(named, ok, ("tz32", "edge1281 tz0", "edge1281 tz5", "c two planes", "runs", "a one"))
    out, st = run_groups(OP_C, np.stack([OC.pack_c(named[i][1]) for i in slots]), np.ones(len(slots), dtype=np.uint8))
    assert st == 0
    for g, i in enumerate(slots):
        cn, low = OC.unpack_c(out[g])
        assert cn == want[i], (g, named[i][0])
        assert low == (1 if g >= 64 else 0), (g, named[i][0])
