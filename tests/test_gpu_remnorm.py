"""GPU: the remainder-only long division (cofhe_amd/csrc/mp.hpp: mp_rem_norm with mp_lincomb_sub_carry_sparse), the step
r = y1 m mod a1 of the composition (qf.hpp: smod with its remainder-only flag) and whole compositions through the kernels that
take it, on the MI355X against Python integers.  tests/gpu_kernels/remnorm_gpu.hip compiles the product headers into small
kernels of its own (built by __graft_entry__.build() into libremnorm_gpu.so); the cases are those of the CPU tier
(tests/remnorm_cases.py).

Every case list runs in the three arrangements of tests/test_gpu_prims.py, each compared with Python integer arithmetic and
never with another arrangement: `solo` (the case in slot i % 8 of a wavefront whose other seven groups are switched off),
`uniform` (all eight groups hold the same case) and `mixed` (the list shuffled with a fixed seed and dealt eight distinct
cases to a wavefront, once per rotation 0..7, the last wavefront partly filled).  In `mixed` the groups of a wavefront divide
with different digit counts, and one group's all-ones limb sends every group of its wavefront through the general resolve."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import remnorm_cases as RC
import simlib as S
from conftest import ROOT, load_json
from gpu_inputs import P, engine, form_record, hx

pytestmark = pytest.mark.gpu

OP_REM2, OP_DIVREM2, OP_REM1, OP_STEP = range(4)
U32 = C.POINTER(C.c_uint32)
CHUNK = 40                       # cases per solo / uniform launch: 320 groups
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "tests", "gpu_kernels", "libremnorm_gpu.so")
        assert os.path.exists(so), "tests/gpu_kernels/libremnorm_gpu.so is built by __graft_entry__.build()"
        import torch  # noqa: F401  (PyTorch's HIP runtime first)
        torch.cuda.init()
        _lib = C.CDLL(so)
        assert _lib.remnorm_gpu_compiled_in() == 1
    return _lib


def run_groups(op, recs, active):
    io = (C.c_int * 2)()
    assert lib().remnorm_gpu_words(op, io) == 0
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, io[0]) and len(active) == n
    act = np.ascontiguousarray(active, dtype=np.uint8)
    out = np.zeros((n, io[1]), dtype=np.uint32)
    st = C.c_uint32(0xFFFFFFFF)
    rc = lib().remnorm_gpu_run(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), act.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(st))
    assert rc == 0, "remnorm_gpu_run(%d) returned %d" % (op, rc)
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
        for lo in range(0, len(o), 8 * CHUNK):   # at most 320 groups per launch
            part = o[lo:lo + 8 * CHUNK]
            slots = np.full(8 * ((len(part) + 7) // 8), -1, dtype=np.int64)
            slots[:len(part)] = part
            yield "mixed%d" % rot, slots


def run_arranged(op, ins, want, names):
    """ins[n, IN]: the packed cases; want[i]: the expected value of case i.  The groups that were switched off must have
    written nothing; the status word must be clear after every launch."""
    ins = np.asarray(ins, dtype=np.uint32)
    for name, slots in arrangements(len(ins)):
        assert len(slots) <= 8 * CHUNK
        recs = np.zeros((len(slots), ins.shape[1]), dtype=np.uint32)
        live = slots >= 0
        recs[live] = ins[slots[live]]
        out, st = run_groups(op, recs, live)
        assert st == 0, (name, st)
        assert not out[~live].any(), name
        for g in np.nonzero(live)[0]:
            i = int(slots[g])
            assert S.from_limbs(out[g]) == want[i], (name, int(g), names[i])


def test_rem_norm_two_planes():
    named = RC.rem_cases()
    assert set(RC.REQUIRED) <= {n for n, _ in named}
    run_arranged(OP_REM2, [RC.pack_rem(c) for _, c in named], [c[0] % c[1] for _, c in named], [n for n, _ in named])


def test_rem_norm_one_plane():
    named = RC.rem1_cases()
    run_arranged(OP_REM1, [RC.pack_rem1(c) for _, c in named], [c[0] % c[1] for _, c in named], [n for n, _ in named])


def test_whole_steps():
    named = RC.step_cases()
    run_arranged(OP_STEP, [RC.pack_step(c) for _, c in named], [RC.step_expected(c) for _, c in named], [n for n, _ in named])


@pytest.fixture(scope="module")
def forms():
    """64 pairs of the k = 128 parameter set: random forms, squarings, forms with their inverses, powers of f, small first
    coefficients; composed once by the Python reference"""
    prm = load_json("params_s128_k128.json")
    d, k = hx(prm["delta"]), prm["k"]
    rng = P.SplitMix64(1880)
    g = [P.random_form(d, rng) for _ in range(12)]
    f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    special = [(g[0], g[0]), (g[1], P.inverse(g[1])), (g[2], f), (P.compose(f, f), g[3]), (P.power(f, 1 << (k - 2), d), g[4]),
               (P.inverse(g[5]), P.inverse(g[6])), (f, f), (g[7], P.identity(d))]
    pairs = special + [(g[rng.below(12)], g[rng.below(12)]) for _ in range(64 - len(special))]
    return d, pairs, [P.compose(a, b) for a, b in pairs]


@pytest.mark.parametrize("n", [1, 33, 64])
def test_compose_records(forms, n):
    """one partly filled workgroup, one record past a workgroup, two workgroups: every record against the Python composition;
    the kernel that ran is one of the two that take the remainder-only step"""
    import torch
    d, pairs, want = forms
    E = engine(d)
    E.set_option("profile_kernels", 1)
    try:
        E.profile_read("k_compose_wg", clear=True)
        pick = pairs[-n:] if n < 64 else pairs                   # n == 1: a random pair; n == 33: the specials' tail and the random pairs
        exp = want[-n:] if n < 64 else want
        dev = lambda fs: torch.from_numpy(np.concatenate([form_record(x.a, x.b, x.c) for x in fs]).view(np.int32)).cuda()
        a, b = dev([p[0] for p in pick]), dev([p[1] for p in pick])
        out = torch.zeros_like(a)
        E.compose_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
        torch.cuda.synchronize()
        ran = {k: E.profile_read(k)[1] for k in ("k_compose_wg", "k_compose_wg3")}
    finally:
        E.profile_read("k_compose_wg", clear=True)
        E.set_option("profile_kernels", 0)
    assert sum(ran.values()) == 1, ran
    got = out.cpu().numpy().view(np.uint32).reshape(n, 168)
    for i, w in enumerate(exp):
        assert np.array_equal(got[i], form_record(w.a, w.b, w.c)), i
