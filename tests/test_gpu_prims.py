"""GPU: the device arithmetic primitives (cofhe_amd/csrc/lane.hpp, mp.hpp, wide.hpp, and the remainder sequences on top of
them) one primitive at a time on the MI355X, against Python integers.  tests/gpu_kernels/prims_gpu.hip compiles the product
headers into small kernels of its own (built by __graft_entry__.build() into libprims_gpu.so); the cases are those of the
CPU tier (tests/prim_cases.py), where the host simulators replace exactly the code that can only go wrong here: the DPP /
ds_bpermute / ballot primitives under a partial EXEC mask, the inline-asm carry chain, the wave shifts and readlanes of the
wide layout, and any_lane, which on the device looks at the whole wavefront.

Every arithmetic op runs its whole case list in three arrangements, each compared with Python integer arithmetic and never
with another arrangement: `solo` (the case in slot i % 8 of a wavefront whose other seven groups are switched off),
`uniform` (all eight groups hold the same case) and `mixed` (the list shuffled with a fixed seed and dealt eight distinct
cases to a wavefront, once per rotation 0..7 of the list so that every case visits every slot, the last wavefront partly
filled) -- rare-route cases then sit beside common ones, and code guarded by any_lane runs in groups that did not ask for it.

The harness inlines the headers into its own kernels, so register allocation and instruction scheduling differ from the
product's kernels: a pass proves the source-level routes on the device, not the product's code object (that is what the
parity tests of whole compositions are for)."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

import prim_cases as PC
import simlib as S
import simwlib as W
from conftest import ROOT

pytestmark = pytest.mark.gpu

OPS = {n: i for i, n in enumerate(["LANE", "MUL11", "MUL21", "LINCOMB", "SHIFT", "BITS", "DIVREM21", "DIVREM11", "DIVREM22", "WORD", "PRIMORIAL",
                                   "DIVEXACT", "XGCD"])}
WOPS = {n: i for i, n in enumerate(["MUL", "LINCOMB", "SHIFT", "CMP", "MOD", "DIVEXACT", "EUCLID"])}
M2 = PC.M2
U32 = C.POINTER(C.c_uint32)
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(ROOT, "tests", "gpu_kernels", "libprims_gpu.so")
        assert os.path.exists(so), "tests/gpu_kernels/libprims_gpu.so is built by __graft_entry__.build()"
        import torch  # noqa: F401  (PyTorch's HIP runtime first)
        torch.cuda.init()
        _lib = C.CDLL(so)
    return _lib


def words(op, wide=False):
    io = (C.c_int * 2)()
    assert (lib().prims_gpu_wide_words if wide else lib().prims_gpu_words)(op, io) == 0
    return io[0], io[1]


def run_groups(op, recs, active):
    """one launch: recs[n_groups, IN] -> (out[n_groups, OUT], status word)"""
    wi, wo = words(op)
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, wi) and len(active) == n
    act = np.ascontiguousarray(active, dtype=np.uint8)
    out = np.zeros((n, wo), dtype=np.uint32)
    st = C.c_uint32(0xFFFFFFFF)
    rc = lib().prims_gpu_run(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), act.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(st))
    assert rc == 0, "prims_gpu_run(%d) returned %d" % (op, rc)
    return out, st.value


def arrangements(n):
    """(name, slots): slots[g] = index of the case in group g of the launch, -1 for a group that is switched off"""
    solo = np.full(8 * n, -1, dtype=np.int64)
    solo[[8 * i + i % 8 for i in range(n)]] = np.arange(n)
    yield "solo", solo
    yield "uniform", np.repeat(np.arange(n), 8)
    order = list(range(n))
    random.Random(20261018).shuffle(order)
    if n % 8 == 0:
        order += order[:3]                       # the last wavefront stays partly filled
    for rot in range(8):
        o = order[rot:] + order[:rot]
        slots = np.full(8 * ((len(o) + 7) // 8), -1, dtype=np.int64)
        slots[:len(o)] = o
        yield "mixed%d" % rot, slots


def run_arranged(op, ins, check, status=0):
    """ins[n, IN]: the packed cases; check(i, out_record) asserts case i against Python.  All three arrangements; the groups
    that were switched off must have written nothing; the status word must be `status` after every launch."""
    ins = np.asarray(ins, dtype=np.uint32)
    for name, slots in arrangements(len(ins)):
        recs = np.zeros((len(slots), ins.shape[1]), dtype=np.uint32)
        live = slots >= 0
        recs[live] = ins[slots[live]]
        out, st = run_groups(op, recs, live)
        assert st == status, (name, st)
        assert not out[~live].any(), name
        for g in np.nonzero(live)[0]:
            check(int(slots[g]), out[g], (name, int(g)))


def exact(expected):
    def check(i, rec, where):
        assert np.array_equal(rec, expected[i]), (where, i)
    return check


def limbs(v, n):
    return S.to_limbs(v, n)


def word(v):
    return np.array([v % (1 << 32)], dtype=np.uint32)


def cat(*parts):
    return np.concatenate(parts)


# ------------------------------------------------------------------------------------------------ lane primitives
def test_lane_primitives_under_every_group_mask():
    """one launch of 256 wavefronts, wavefront w with group mask w: every active lane has read only lanes of its own group
    (the input word is different in every lane of the launch), ballot8 holds the group's predicates, any_lane is the OR
    over the ACTIVE groups of the wavefront, the groups switched off write nothing"""
    rng = random.Random(77)
    n_groups = 256 * 8
    v = np.array([(i * 2654435761 + 12345) % (1 << 32) for i in range(n_groups * 8)], dtype=np.uint64).reshape(n_groups, 8)
    pred = np.zeros((n_groups, 8), dtype=np.uint64)
    for w in range(256):
        kind = w % 4           # 0: random, 1: nobody, 2: only groups that are switched off (or nobody), 3: one lane of one group
        for g in range(8):
            on = (w >> g) & 1
            for l in range(8):
                if kind == 0:
                    pred[8 * w + g, l] = rng.getrandbits(1)
                elif kind == 2:
                    pred[8 * w + g, l] = 0 if on else 1
        if kind == 3:
            pred[8 * w + rng.randrange(8), rng.randrange(8)] = 1
    recs = np.stack([v, pred], axis=2).reshape(n_groups, 16).astype(np.uint32)
    active = np.array([(g // 8 >> (g % 8)) & 1 for g in range(n_groups)], dtype=np.uint8)
    out, st = run_groups(OPS["LANE"], recs, active)
    assert st == 0
    out = out.reshape(n_groups, 8, 18)
    assert not out[active == 0].any()
    for w in range(256):
        groups = [g for g in range(8) if (w >> g) & 1]
        any_w = int(any(pred[8 * w + g].any() for g in groups))
        for g in groups:
            vals = [int(x) for x in v[8 * w + g]]
            ballot = sum(int(pred[8 * w + g, l]) << l for l in range(8))
            for l in range(8):
                me = vals[l]
                want = vals + [vals[l - 1] if l else me ^ 0xFFFFFFFF, vals[l + 1] if l < 7 else me ^ 0xFFFFFFFF, vals[l ^ 1], vals[l ^ 2],
                               vals[7 - l], vals[0], vals[7], ballot, any_w, max(vals)]
                assert [int(x) for x in out[8 * w + g, l]] == want, (w, g, l)


# ------------------------------------------------------------------------------------------------ arithmetic ops
def test_mul():
    xs, ys, xs2, ys2 = PC.mul_cases()
    run_arranged(OPS["MUL11"], [cat(limbs(a, 40), limbs(b, 40)) for a, b in zip(xs, ys)], exact([limbs(a * b, 80) for a, b in zip(xs, ys)]))
    run_arranged(OPS["MUL21"], [cat(limbs(a, 80), limbs(b, 40)) for a, b in zip(xs2, ys2)], exact([limbs(a * b, 120) for a, b in zip(xs2, ys2)]))


def test_lincomb_add_and_the_words_that_leave_the_top_plane():
    """mp_lincomb_sub_carry, mp_lincomb_add and mp_add on two planes: the CPU tier's lists, the carry chain at its bounds
    (A + B = 2^32 on all-ones operands: every h_j and every carry of lincomb_plane at its maximum), sums that carry out of
    the top plane, a word handed from lane 7 of plane 0 into an all-ones lane 0 of plane 1, the pat(...) operands of the
    sparse resolve.  A x - B y == r + (word - B) 2^2560, A x + B y == s + word 2^2560"""
    cases = PC.lincomb_shift_cases()[0] + PC.carry_ripple_cases() + PC.lincomb_bound_cases()
    ins = [cat(limbs(x, 80), limbs(y, 80), word(A), word(B)) for A, B, x, y in cases]
    exp = [cat(limbs((A * x - B * y) % M2, 80), limbs((A * x + B * y) % M2, 80), limbs((x + y) % M2, 80), word((A * x - B * y) // M2 + B),
               word((A * x + B * y) // M2), word((x + y) // M2)) for A, B, x, y in cases]
    run_arranged(OPS["LINCOMB"], ins, exact(exp))


def test_shifts_and_bit_positions():
    """mp_shl / mp_shr / mp_shr1 / mp_bitlen at limb, lane (160) and plane (1280) edges, every group of a wavefront with a
    shift amount of its own; mp_cmp / mp_bits64 / mp_bits32 / mp_get_limb on windows that straddle those edges"""
    cases = PC.lincomb_shift_cases()[1] + PC.shift_edge_cases()
    ins = [cat(limbs(v, 80), word(sh)) for sh, v in cases]
    exp = [cat(limbs((v << sh) % M2, 80), limbs(v >> sh, 80), limbs(v >> 1, 80), word(v.bit_length())) for sh, v in cases]
    run_arranged(OPS["SHIFT"], ins, exact(exp))
    cases = PC.bits_cases()
    ins = [cat(limbs(x, 80), limbs(y, 80), word(p), word(k)) for x, y, p, k in cases]
    exp = [cat(word((x > y) - (x < y)), limbs((x >> p) & ((1 << 64) - 1), 2), word((x >> p) & PC.ONES),
               word((x >> (32 * k)) & PC.ONES if 0 <= k < 80 else 0)) for x, y, p, k in cases]
    run_arranged(OPS["BITS"], ins, exact(exp))


@pytest.mark.parametrize("pn,pd", [(2, 1), (1, 1), (2, 2)])
def test_divrem(pn, pd):
    """mp_divrem in the instantiations of qf.hpp (<2,1>: mp_divrem_word and mp_divrem_norm; <1,1>) and with a two-plane
    divisor (<2,2>: mp_divrem_cons below 64 bits, the staged-divisor loop and its add-back above): the add-back families
    num = den Q - 1 and num = den Q + den - 1 (the CPU tier proves that they reach the add-back), num < den, num == den,
    num == 0, word-sized divisors, the CPU tier's random list.  Then a zero divisor, alone in its launch: quotient 0, the
    numerator untouched, CF_ST_DIV_CAP in the status word, a normal return."""
    op = OPS["DIVREM%d%d" % (pn, pd)]
    addback, rest = PC.divrem_cases(pn, pd)
    pairs = [(n, d) for n, d, _ in addback] + rest
    ins = [cat(limbs(n, 40 * pn), limbs(d, 40 * pd)) for n, d in pairs]
    run_arranged(op, ins, exact([cat(limbs(n // d, 40 * pn), limbs(n % d, 40 * pn)) for n, d in pairs]))
    num = 12345 << 700
    recs = np.zeros((8, 40 * (pn + pd)), dtype=np.uint32)
    recs[3] = cat(limbs(num, 40 * pn), limbs(0, 40 * pd))
    out, st = run_groups(op, recs, [0, 0, 0, 1, 0, 0, 0, 0])
    assert st == PC.ST_DIV_CAP
    assert np.array_equal(out[3], cat(limbs(0, 40 * pn), limbs(num, 40 * pn))) and not out[[0, 1, 2, 4, 5, 6, 7]].any()


def test_word_divisions_and_residues():
    """mp_divrem_word, mp_mod_word, mp_mod_word_fast (one and two planes) and mp_mod_primorial"""
    Ws, xs, ps, _ms, _as = PC.word_route_cases()
    ins = [cat(limbs(x, 80), word(w)) for x, w in zip(xs, Ws)]
    exp = [cat(limbs(x // w, 80), word(x % w), word(x % w), word((x % PC.M1) % w), word(x % w)) for x, w in zip(xs, Ws)]
    run_arranged(OPS["WORD"], ins, exact(exp))
    run_arranged(OPS["PRIMORIAL"], [limbs(x, 40) for x in ps], exact([word(x % 223092870) for x in ps]))


def test_divexact():
    """mp_divexact <2,2>: the CPU tier's list (odd / even / word-sized divisors, 32 and more trailing zero bits: the
    long-division route, the two-digits-per-pass loop at its largest hand-over words); then a zero divisor alone in its
    launch: it reaches mp_divrem, which flags it and returns quotient 0"""
    cases, nq = PC.divexact_cases()
    ins = [cat(limbs(n, 80), limbs(d, 40), word(k)) for (n, d, _q), k in zip(cases, nq)]
    run_arranged(OPS["DIVEXACT"], ins, exact([limbs(q, 80) for _n, _d, q in cases]))
    recs = np.zeros((8, 121), dtype=np.uint32)
    recs[5] = cat(limbs(7 << 64, 80), limbs(0, 40), word(3))
    out, st = run_groups(OPS["DIVEXACT"], recs, [0, 0, 0, 0, 0, 1, 0, 0])
    assert st == PC.ST_DIV_CAP and not out.any()


def test_xgcd():
    """euclid_run down to the gcd: d == gcd(x, y) and sign u y == d (mod x), as on the CPU tier"""
    _n, _d, xa, ya = PC.divrem_xgcd_cases()

    def check(i, rec, where):
        d, u, s = S.from_limbs(rec[:40]), S.from_limbs(rec[40:80]), int(np.int32(rec[80]))
        assert d == math.gcd(xa[i], ya[i]), (where, i)
        assert s in (-1, 1) and (s * u * ya[i] - d) % xa[i] == 0, (where, i)
    run_arranged(OPS["XGCD"], [cat(limbs(a, 40), limbs(b, 40)) for a, b in zip(xa, ya)], check)


# ------------------------------------------------------------------------------------------------ served Euclid
def test_euclid_wg_cofactors_and_stops():
    """euclid_run_wg with the kernels' workgroup (WG_BLOCK threads, make_served_ctx): the cases and the assertions of the
    CPU tier's test of the same name; a workgroup that is not full (the last groups duplicate its last pair) and two
    workgroups in one launch"""
    L = lib()
    n = L.prims_gpu_wg_groups()

    def run(pairs, stops):
        m = len(pairs)
        x = np.concatenate([S.to_limbs(a, 40) for a, _ in pairs])
        y = np.concatenate([S.to_limbs(b, 40) for _, b in pairs])
        out = np.zeros(160 * m, dtype=np.uint32)
        sg = np.zeros(2 * m, dtype=np.int32)
        stp = np.array(stops, dtype=np.int32)
        st = C.c_uint32(0xFFFFFFFF)
        rc = L.prims_gpu_euclid_wg(S.P(x), S.P(y), m, stp.ctypes.data_as(C.c_void_p), S.P(out), sg.ctypes.data_as(C.c_void_p), C.byref(st))
        assert rc == 0 and st.value == 0, (rc, st.value)
        res = []
        for i in range(m):
            o = out[160 * i:160 * i + 160]
            res.append((S.from_limbs(o[:40]), S.from_limbs(o[40:80]), int(sg[2 * i]) * S.from_limbs(o[80:120]),
                        int(sg[2 * i + 1]) * S.from_limbs(o[120:160])))
        return res

    full, part = PC.euclid_wg_cases(n)
    assert len(full) < n < len(part)
    for (a, b), (x, y, cx, cy) in zip(full, run(full, [-1] * len(full))):
        assert x == math.gcd(a, b) and y == 0, (a.bit_length(), b.bit_length())
        assert (cx * b - x) % a == 0 and (cy * b) % a == 0
    res = run([(a, b) for a, b, _ in part], [s for _, _, s in part])
    for (a, b, stop), (x, y, cx, cy) in zip(part, res):
        assert x >= y and y.bit_length() <= stop, (stop, x.bit_length(), y.bit_length())
        assert (cx * b - x) % a == 0 and (cy * b - y) % a == 0
        assert x * abs(cy) + y * abs(cx) == a                     # consecutive remainders of one sequence


# ------------------------------------------------------------------------------------------------ wide layout
def run_wide(op, recs, waves):
    wi, wo = words(op, wide=True)
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n = recs.shape[0]
    assert recs.shape == (n, wi)
    out = np.zeros((n, wo), dtype=np.uint32)
    rc = lib().prims_gpu_wide(op, recs.ctypes.data_as(U32), out.ctypes.data_as(U32), n, waves)
    assert rc == 0, "prims_gpu_wide(%d) returned %d" % (op, rc)
    return out


def wl(v):
    return W.pack([v])


@pytest.mark.parametrize("waves", [1, 4])
def test_wide_mul_lincomb_shift_cmp(waves):
    """w_mul, w_lincomb_sub / w_lincomb_add with the word that leaves the top, w_shl / w_shr / w_bitlen, w_cmp: one number
    per wavefront, one and four wavefronts per workgroup (lane_id() is threadIdx.x & 63: every cross-lane op must stay in
    its wavefront).  The CPU tier's lists, 2^4096 - 1 + 1, 2^4096 - 1 - x, hand-over words and propagate runs across the
    row edges (lanes 15|16, 31|32, 47|48: wave_shr differs from row_shr there), shifts of even and odd limb counts"""
    xs, ys, lin, shifts, cmps = PC.wide_mul_lincomb_shift_cases()
    out = run_wide(WOPS["MUL"], [cat(wl(a), wl(b)) for a, b in zip(xs, ys)], waves)
    assert W.unpack(out) == [(a * b) % W.M for a, b in zip(xs, ys)]
    lin = lin + PC.wide_lincomb_edge_cases()
    out = run_wide(WOPS["LINCOMB"], [cat(wl(x), wl(y), word(A), word(B)) for A, B, x, y in lin], waves)
    for (A, B, x, y), o in zip(lin, out):
        assert W.unpack(o[:128]) == [(A * x - B * y) % W.M] and W.unpack(o[128:256]) == [(A * x + B * y) % W.M], (A, B)
        assert int(o[256]) == (A * x - B * y) // W.M + B and int(o[257]) == (A * x + B * y) // W.M, (A, B)
    shifts = shifts + PC.wide_shift_edge_cases()
    out = run_wide(WOPS["SHIFT"], [cat(wl(v), word(sh)) for sh, v in shifts], waves)
    for (sh, v), o in zip(shifts, out):
        assert W.unpack(o[:128]) == [(v << sh) % W.M] and W.unpack(o[128:256]) == [v >> sh] and int(o[256]) == v.bit_length(), sh
    cmps = cmps + [(W.M - 1, W.M - 2), (1 << 1024, (1 << 1024) - 1), ((1 << 2048) - 1, 1 << 2048), (1 << 3072, 1 << 3071)]
    out = run_wide(WOPS["CMP"], [cat(wl(a), wl(b)) for a, b in cmps], waves)
    assert [int(np.int32(o[0])) for o in out] == [(a > b) - (a < b) for a, b in cmps]


@pytest.mark.parametrize("waves", [1, 4])
def test_wide_divisions(waves):
    """w_mod (with the add-back family: remainder den - 1) and w_divexact; a divisor whose low 64 bits are zero is declined"""
    mods, exact_, nq = PC.wide_division_cases()
    out = run_wide(WOPS["MOD"], [cat(wl(n), wl(d)) for n, d in mods], waves)
    assert all(int(o[128]) == 1 for o in out)
    assert W.unpack(out[:, :128]) == [n % d for n, d in mods]
    out = run_wide(WOPS["DIVEXACT"], [cat(wl(n), wl(d), word(k)) for (n, d, _q), k in zip(exact_, nq)], waves)
    assert all(int(o[128]) == 1 for o in out)
    assert W.unpack(out[:, :128]) == [q for _n, _d, q in exact_]
    out = run_wide(WOPS["DIVEXACT"], [cat(wl(3 << 64), wl(1 << 64), word(1))], waves)
    assert int(out[0, 128]) == 0
    out = run_wide(WOPS["MOD"], [cat(wl(12345), wl(0))], waves)         # zero divisor: declined, no fault
    assert int(out[0, 128]) == 0


@pytest.mark.parametrize("waves", [1, 4])
def test_wide_remainder_sequence(waves):
    """w_euclid: the cases and the invariants of the CPU tier's test of the same name"""
    cases = PC.wide_euclid_cases()
    out = run_wide(WOPS["EUCLID"], [cat(wl(x), wl(y), word(s)) for x, y, s in cases], waves)
    for (x0, y0, stop), o in zip(cases, out):
        assert int(o[514]) == 1, (x0, y0, stop)
        x, y, ux, uy = (W.unpack(o[128 * k:128 * (k + 1)])[0] for k in range(4))
        sx, sy = int(np.int32(o[512])), int(np.int32(o[513]))
        assert x >= y and math.gcd(x, y) == math.gcd(x0, y0), (x0, y0, stop)
        if x0:
            assert (x - sx * ux * y0) % x0 == 0 and (y - sy * uy * y0) % x0 == 0, (x0, y0, stop)
        if stop < 0:
            assert y == 0
        else:
            assert y.bit_length() <= stop or y == 0
            assert x.bit_length() > stop or max(x0, y0).bit_length() <= stop or min(x0, y0).bit_length() <= stop, (x0, y0, stop)
