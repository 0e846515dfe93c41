"""GPU: the paired 2-adic division (cofhe_amd/csrc/mp.hpp: mp_divexact_pair; qf.hpp: m12_low_quot_pair), mp_divexact with a
one-plane numerator, mp_sqr_low from every chunk pair once, and whole compositions through nucomp_m12, nucomp_ab and nucomp_c
on the MI355X against Python integers.  tests/gpu_kernels/pairdiv_gpu.hip compiles the product headers into small kernels of
its own (built by __graft_entry__.build() into libpairdiv_gpu.so); the cases are those of the CPU tier
(tests/pairdiv_cases.py).

Every case list runs in the three arrangements of tests/test_gpu_prims.py, each compared with Python integer arithmetic and
never with another arrangement: `solo` (the case in slot i % 8 of a wavefront whose other seven groups are switched off),
`uniform` (all eight groups hold the same case) and `mixed` (the list shuffled with a fixed seed and dealt eight distinct
cases to a wavefront, once per rotation 0..7, the last wavefront partly filled)."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import lowmul_cases as LC
import onep_cases as OC
import pairdiv_cases as PC
import simlib as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

OP_DIVP, OP_QUOTP, OP_DIVX, OP_SQR, OP_M12, OP_AB, OP_C = range(7)
U32 = C.POINTER(C.c_uint32)
CHUNK = 40                       # cases per solo / uniform launch: 320 groups
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "tests", "gpu_kernels", "libpairdiv_gpu.so")
        assert os.path.exists(so), "tests/gpu_kernels/libpairdiv_gpu.so is built by __graft_entry__.build()"
        import torch  # noqa: F401  (PyTorch's HIP runtime first)
        torch.cuda.init()
        _lib = C.CDLL(so)
        assert _lib.pairdiv_gpu_compiled_in() == 7
    return _lib


def run_groups(op, recs, active):
    io = (C.c_int * 2)()
    assert lib().pairdiv_gpu_words(op, io) == 0
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, io[0]) and len(active) == n
    act = np.ascontiguousarray(active, dtype=np.uint8)
    out = np.zeros((n, io[1]), dtype=np.uint32)
    st = C.c_uint32(0xFFFFFFFF)
    rc = lib().pairdiv_gpu_run(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), act.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(st))
    assert rc == 0, "pairdiv_gpu_run(%d) returned %d" % (op, rc)
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


def test_divexact_pair():
    cases = PC.divp_cases()
    exp = [PC.divp_expected(c) for c in cases]

    def check(i, rec, _wave, where):
        assert np.array_equal(rec, exp[i]), (where, i)
    run_arranged(OP_DIVP, [PC.pack_divp(c) for c in cases], check)


def test_quot_pair():
    named = PC.quotp_cases() + PC.quotp_raw_cases()
    exp = [PC.quotp_model(c) for _, c in named]

    def check(i, rec, _wave, where):
        assert PC.unpack_quotp(rec) == exp[i], (where, named[i][0])
    run_arranged(OP_QUOTP, [PC.pack_quotp(c) for _, c in named], check)


def test_divexact_one_plane_without_high_limbs():
    named = PC.divx_cases()
    exp = [PC.divx_expected(c) % (1 << c[3]) for _, c in named]

    def check(i, rec, _wave, where):
        got = S.from_limbs(rec)
        assert got < 1 << (32 * named[i][1][2]) and got % (1 << named[i][1][3]) == exp[i], (where, named[i][0])
    run_arranged(OP_DIVX, [PC.pack_divx(c) for _, c in named], check)


def test_sqr_low():
    cases = PC.sqr_cases()
    exp = [OC.expected_sqr(x) for x in cases]

    def check(i, rec, _wave, where):
        assert np.array_equal(rec, exp[i]), (where, i)
    run_arranged(OP_SQR, [S.to_limbs(x, 40) for x in cases], check)


@pytest.fixture(scope="module")
def comp():
    return PC.composition_cases()


def test_compositions_m12(comp):
    """the route is the wavefront's verdict: a group reports the paired division exactly when every live group of its
    wavefront is within the bound, and its quotients are right on whichever route that made it take"""
    named = comp[0]
    want, ok = [LC.expected(c) for _, c in named], [LC.low_route(c) for _, c in named]

    def check(i, rec, wave, where):
        M1, M2, low = LC.unpack_m12(rec)
        assert (M1, M2) == want[i], (where, named[i][0])
        assert low == (1 if all(ok[j] for j in wave) else 0), (where, named[i][0])
    run_arranged(OP_M12, [LC.pack_m12(c, 1) for _, c in named], check)


def test_compositions_ab(comp):
    """the route is the verdict of the groups that vote: here every group brings its own m2_one_plane flag, and a group
    without it goes to the double-width dots before the ballot (tests/test_gpu_onep.py)"""
    named = comp[1]
    want, ok, flag = [OC.ab_expected(c) for _, c in named], [OC.ab_one_plane(c) for _, c in named], [bool(c[7]) for _, c in named]

    def check(i, rec, wave, where):
        an, bn, one = OC.unpack_ab(rec)
        assert (an, bn) == want[i], (where, named[i][0])
        assert one == (1 if flag[i] and all(ok[j] for j in wave if flag[j]) else 0), (where, named[i][0])
    run_arranged(OP_AB, [OC.pack_ab(c) for _, c in named], check)


def test_compositions_c(comp):
    named = comp[2]
    want, ok = [OC.c_expected(c) for _, c in named], [OC.c_low(c) for _, c in named]

    def check(i, rec, wave, where):
        cn, low = OC.unpack_c(rec)
        assert cn == want[i], (where, named[i][0])
        assert low == (1 if all(ok[j] for j in wave) else 0), (where, named[i][0])
    run_arranged(OP_C, [OC.pack_c(c) for _, c in named], check)


def test_one_group_outside_the_bound_takes_its_wavefront_along():
    """eight wavefronts of seven groups within the bound and one outside it (nb + 1 + tz == 641 among them), in slot w of
    wavefront w, and a ninth wavefront with all eight within (nb + 1 + tz == 640 among them): only the ninth reports the
    paired division, every quotient is right"""
    named = LC.m12_cases()
    want, ok = [LC.expected(c) for _, c in named], [LC.low_route(c) for _, c in named]
    inside = [i for i, (n, _) in enumerate(named) if n in ("edge640 tz0", "edge640 tz3", "edge m637", "largest", "largest neg", "below")]
    inside += [i for i in range(len(named)) if ok[i] and i not in inside]
    outside = [i for i, (n, _) in enumerate(named) if n in ("edge641 tz0", "edge641 tz3", "edge m638", "above", "tz32", "two planes")]
    assert len(inside) >= 15 and len(outside) >= 8 and not any(ok[i] for i in outside) and all(ok[i] for i in inside)
    slots = []
    for w in range(8):
        row = [inside[(7 * w + k) % len(inside)] for k in range(7)]
        row.insert(w, outside[w])
        slots += row
    slots += inside[:8]
    out, st = run_groups(OP_M12, np.stack([LC.pack_m12(named[i][1], 1) for i in slots]), np.ones(len(slots), dtype=np.uint8))
    assert st == 0
    for g, i in enumerate(slots):
        M1, M2, low = LC.unpack_m12(out[g])
        assert (M1, M2) == want[i], (g, named[i][0])
        assert low == (1 if g >= 64 else 0), (g, named[i][0])
