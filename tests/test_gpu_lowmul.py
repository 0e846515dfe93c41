"""GPU: the low-half products (cofhe_amd/csrc/mp.hpp: mp_mul_low2) and nucomp_m12 on both of its routes
(cofhe_amd/csrc/qf.hpp) on the MI355X against Python integers.  tests/gpu_kernels/lowmul_gpu.hip compiles the product
headers into small kernels of its own (built by __graft_entry__.build() into liblowmul_gpu.so); the cases are those of the
CPU tier (tests/lowmul_cases.py).

Every case list runs in the three arrangements of tests/test_gpu_prims.py, each compared with Python integer arithmetic and
never with another arrangement: `solo` (the case in slot i % 8 of a wavefront whose other seven groups are switched off),
`uniform` (all eight groups hold the same case) and `mixed` (the list shuffled with a fixed seed and dealt eight distinct
cases to a wavefront, once per rotation 0..7, the last wavefront partly filled).  The route decision is a ballot over the
wavefront: a group reports the low-half route exactly when every live group of its wavefront is within the bound, and its
quotients are right on whichever route that made it take."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import lowmul_cases as LC
from conftest import ROOT

pytestmark = pytest.mark.gpu

OP_MUL, OP_M12 = 0, 1
U32 = C.POINTER(C.c_uint32)
CHUNK = 40                       # cases per solo / uniform launch: 320 groups
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "tests", "gpu_kernels", "liblowmul_gpu.so")
        assert os.path.exists(so), "tests/gpu_kernels/liblowmul_gpu.so is built by __graft_entry__.build()"
        import torch  # noqa: F401  (PyTorch's HIP runtime first)
        torch.cuda.init()
        _lib = C.CDLL(so)
        assert _lib.lowmul_gpu_compiled_in() == 1
    return _lib


def run_groups(op, recs, active):
    io = (C.c_int * 2)()
    assert lib().lowmul_gpu_words(op, io) == 0
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, io[0]) and len(active) == n
    act = np.ascontiguousarray(active, dtype=np.uint8)
    out = np.zeros((n, io[1]), dtype=np.uint32)
    st = C.c_uint32(0xFFFFFFFF)
    rc = lib().lowmul_gpu_run(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), act.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(st))
    assert rc == 0, "lowmul_gpu_run(%d) returned %d" % (op, rc)
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


def test_mul_low2():
    cases = LC.mul_cases()
    exp = [LC.expected_mul(c) for c in cases]

    def check(i, rec, _wave, where):
        assert np.array_equal(rec, exp[i]), (where, i)
    run_arranged(OP_MUL, [LC.pack_mul(c) for c in cases], check)


@pytest.fixture(scope="module")
def m12():
    named = LC.m12_cases()
    cases = [c for _, c in named]
    return named, [LC.expected(c) for c in cases], [LC.low_route(c) for c in cases]


@pytest.mark.parametrize("try_low", [1, 0])
def test_m12_in_three_arrangements(m12, try_low):
    """M1, M2 against Python's exact quotients; with try_low the route is the wavefront's verdict, without it the full products"""
    named, want, ok = m12

    def check(i, rec, wave, where):
        M1, M2, low = LC.unpack_m12(rec)
        assert (M1, M2) == want[i], (where, named[i][0])
        assert low == (1 if try_low and all(ok[j] for j in wave) else 0), (where, named[i][0])
    run_arranged(OP_M12, [LC.pack_m12(c, try_low) for _, c in named], check)


def test_one_group_outside_the_bound_takes_its_wavefront_along(m12):
    """eight wavefronts of seven groups within the bound and one outside it, in slot w of wavefront w, and a ninth wavefront
    with all eight within: only the ninth reports the low-half route, every quotient is right"""
    named, want, ok = m12
    inside = [i for i in range(len(named)) if ok[i]]
    outside = [i for i, (n, _) in enumerate(named) if n in ("above", "edge641 tz0", "edge641 tz3", "edge m638", "tz32", "two planes")]
    assert len(inside) >= 15 and len(outside) >= 8 and not any(ok[i] for i in outside)
    slots = []
    for w in range(8):
        row = [inside[(7 * w + k) % len(inside)] for k in range(7)]
        row.insert(w, outside[w])
        slots += row
    slots += inside[7:15]
    out, st = run_groups(OP_M12, np.stack([LC.pack_m12(named[i][1], 1) for i in slots]), np.ones(len(slots), dtype=np.uint8))
    assert st == 0
    for g, i in enumerate(slots):
        M1, M2, low = LC.unpack_m12(out[g])
        assert (M1, M2) == want[i], (g, named[i][0])
        assert low == (1 if g >= 64 else 0), (g, named[i][0])
