"""CPU: ciphertext differences and the plaintext addend without a GPU.  The body of k_sub_ct / k_invert_records
(cofhe_amd/csrc/affine.hpp) on the host simulator's 32-group workgroup against the pure-Python model, the comb's slot map
with the addend's shape fields (comb.hpp), and how the launcher shapes and carves kinds 3 and 4 (cofhe_hip_comb_shape,
cofhe_hip_workspace_plan "comb").  No kernel runs."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import simlib as S
from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libaffinesim.so")
REC = S.REC_WORDS
REC_BYTES = REC * 4


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "affine_sim.cpp")
    deps = [src, os.path.join(HERE, "hostsim", "sim.cpp")] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in
                                                              ("affine.hpp", "comb.hpp", "qf.hpp", "mp.hpp", "lane.hpp", "form_io.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        # the kernels' workgroup geometry: 32 groups = 256 host threads = four wavefronts
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-DCOFHE_WG_GROUPS=32", "-o", _SO, src])
    L = C.CDLL(_SO)
    assert L.sim_wg_groups() == 32
    return L


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cofhe_amd import load_library
    return load_library()


def t3(x):
    return (x.a, x.b, x.c)


def sub_wg(sim, pairs, d):
    """a o b^-1 for up to 32 pairs in one simulated workgroup; returns the forms and the simulator's status word"""
    n = len(pairs)
    half = ((-d).bit_length() + 1) // 2
    ad = S.to_limbs(-d, 80)
    fa = np.concatenate([S.form_record(*t3(a)) for a, _ in pairs])
    fb = np.concatenate([S.form_record(*t3(b)) for _, b in pairs])
    out = np.zeros(n * REC, dtype=np.uint32)
    sim.affine_sim_sub_wg(S.P(fa), S.P(fb), S.P(out), n, half, S.P(ad))
    return [S.record_form(out[i * REC:(i + 1) * REC]) for i in range(n)], sim.sim_status()


def boundary_forms(prm):
    d, k = hx(prm["delta"]), prm["k"]
    f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    one = P.identity(d)
    half_f = P.power(f, 1 << (k - 1), d)            # the element of order two of <f>: (4, 4, c), its own inverse
    assert (half_f.a, half_f.b) == (4, 4) and t3(P.inverse(half_f)) == t3(half_f)
    return d, k, f, one, half_f


@pytest.mark.parametrize("name", ["tiny_k8", "s128_k128"])
def test_subtraction_body_on_a_workgroup_of_32(sim, name):
    """load, qf_inverse, qf_compose<true>, store for 32 pairs at a time equals compose(a, inverse(b)): random pairs, x - x in
    every group at once (all principal) and among others, b the principal form, b = f^(2^(k-1)) = (4, 4, c) whose sign must
    not flip, a ragged last workgroup"""
    prm = load_json("params_%s.json" % name)
    d, k, f, one, half_f = boundary_forms(prm)
    rng = P.SplitMix64(4141 + k)
    pool = [P.random_form(d, rng, 12, 10) for _ in range(12)] if name == "tiny_k8" else [P.random_form(d, rng) for _ in range(12)]
    pool += [f, P.inverse(f)]
    pick = lambda: pool[rng.below(len(pool))]            # noqa: E731
    same = [(x, x) for x in (pool * 3)[:32]]
    mixed = [(pick(), pick()) for _ in range(16)] + [(pick(), one) for _ in range(3)] + [(one, pick()) for _ in range(2)]
    mixed += [(pick(), half_f) for _ in range(3)] + [(half_f, half_f), (one, one), (half_f, one), (one, half_f)]
    mixed += [(x, x) for x in pool[:4]]
    ragged = [(pick(), pick()) for _ in range(5)] + [(pool[0], pool[0]), (pool[1], half_f)]
    assert len(same) == 32 and len(mixed) == 32
    for chunk in (same, mixed, ragged):
        got, status = sub_wg(sim, chunk, d)
        assert [tuple(g) for g in got] == [t3(P.compose(a, P.inverse(b))) for a, b in chunk]
        assert status == 0
    got, _ = sub_wg(sim, same, d)
    assert all(tuple(g) == t3(one) for g in got)


def test_invert_record_body(sim):
    """qf_invert_record equals the model's inverse, boundary forms included (b = 0, b = a: unchanged), in place too, and
    inverting twice gives the input back"""
    prm = load_json("params_s128_k128.json")
    d, k, f, one, half_f = boundary_forms(prm)
    rng = P.SplitMix64(77)
    forms = [one, half_f, f, P.inverse(f)] + [P.random_form(d, rng) for _ in range(12)]
    rec = np.concatenate([S.form_record(*t3(x)) for x in forms])
    out = np.zeros_like(rec)
    sim.affine_sim_invert(S.P(rec), S.P(out), len(forms))
    assert [S.record_form(out[i * REC:(i + 1) * REC]) for i in range(len(forms))] == [t3(P.inverse(x)) for x in forms]
    sim.affine_sim_invert(S.P(out), S.P(out), len(forms))
    assert np.array_equal(out, rec)


def exp_rec(v):
    r = np.zeros(32, dtype=np.uint32)
    r[:31] = np.frombuffer(abs(v).to_bytes(124, "little"), dtype="<u4")
    r[31] = 1 if v < 0 else 0
    return r


def slot_map(sim, shape9, h, r, m):
    er, em = exp_rec(r), exp_rec(m)
    sh = np.array(shape9, dtype=np.uint32)
    n = (shape9[1] + shape9[2] + shape9[3] + 1) & ~1
    sel = np.zeros(4 * n, dtype=np.int32)
    ns = C.c_uint32()
    sim.affine_sim_slots(sh.ctypes.data_as(C.c_void_p), C.c_uint32(h), er.ctypes.data_as(C.c_void_p), em.ctypes.data_as(C.c_void_p),
                         sel.ctypes.data_as(C.c_void_p), C.byref(ns))
    assert ns.value == n
    return sel.reshape(n, 4)


@pytest.mark.parametrize("w", [2, 5, 8, 10])
@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_slot_map_of_the_plaintext_addend(sim, w, kind, mode):
    """over a column the selected entries multiply out to r (its own half's table) and, in the c2 column, to +-(|m| mod 2^k)
    with the sign of m, negated for ct - m; the leaf is there exactly once, after the positions; kind 3 has no r slots and
    one column (half 1); the c1 column of kind 4 reads nothing of f"""
    rng = random.Random(31 * w + 7 * kind + mode)
    k = 128
    M = 1 << k
    ms = [0, 1, -1, M - 1, M, M + 5, -(M + 9), (M << 40) + 3, rng.getrandbits(k), -rng.getrandbits(200)]
    for m in ms:
        r = 0 if kind == 3 else rng.choice([0, 1, -5, rng.randrange(1 << 966), (1 << 966) - 1])
        npos_r = 0 if kind == 3 else max(abs(r).bit_length(), 1) // w + 1
        npos_m = k // w + 1
        halves = 1 if kind == 3 else 2
        shape = [w, npos_r, npos_m, 1, halves, k, 1 if kind == 3 else 0, 1 if mode == 1 else 0, 1 if mode == 2 else 0]
        for h in ([1] if kind == 3 else [0, 1]):
            sel = slot_map(sim, shape, h, r, m)
            acc = {0: 0, 1: 0, 2: 0}
            leaves = 0
            for s, row in enumerate(sel):
                table, pos, dg, entry = (int(x) for x in row)
                if table in (0, 1, 2):
                    assert dg != 0 and abs(dg) <= 1 << (w - 1)
                    assert entry == pos * (1 << (w - 1)) + abs(dg) - 1
                    acc[table] += dg << (w * pos)
                    assert (s < npos_r) == (table != 2)
                elif table == 3:
                    leaves += 1
                    assert s == npos_r + npos_m
                else:
                    assert table == -1
            assert leaves == 1
            assert acc[1 - h] == 0
            assert acc[h] == r
            if kind == 3:
                assert acc[0] == acc[1] == 0
            if h == 1:
                want = abs(m) % M
                want = -want if m < 0 else want
                assert acc[2] == (-want if mode == 1 else want)
            else:
                assert acc[2] == 0


@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_addend_columns_multiply_out_in_the_group(sim, kind, mode):
    """the slots of a column, taken as k_comb_first takes them -- table entry T[pos][|d|] = base^(|d| 2^(w pos)), inverted for a
    negative digit, the input record for the leaf, inverted for m - ct, the principal form elsewhere -- compose (in the
    model's arithmetic, tiny_k8) to c2^(+-1) o pk^r o f^(+-m mod 2^k) and c1^(+-1) o h^r"""
    prm = load_json("params_tiny_k8.json")
    d, k = hx(prm["delta"]), prm["k"]
    F = lambda o: P.Form(hx(o["a"]), hx(o["b"]), hx(o["c"]))       # noqa: E731
    bases = {0: F(prm["h"]), 1: F(prm["pk"]), 2: F(prm["f"])}
    rng = P.SplitMix64(800 + 10 * kind + mode)
    leafs = [P.random_form(d, rng, 12, 10), P.random_form(d, rng, 12, 10)]
    M = 1 << k
    for w in (2, 5):
        for m in (0, 1, -1, M - 1, M + 5, -(M + 9), 77):
            r = 0 if kind == 3 else [0, 5, -3, 12345][abs(m) % 4]
            npos_r = 0 if kind == 3 else max(abs(r).bit_length(), 1) // w + 1
            shape = [w, npos_r, k // w + 1, 1, 1 if kind == 3 else 2, k, 1 if kind == 3 else 0, 1 if mode == 1 else 0, 1 if mode == 2 else 0]
            for h in ([1] if kind == 3 else [0, 1]):
                acc = P.identity(d)
                for table, pos, dg, _ in (tuple(int(x) for x in row) for row in slot_map(sim, shape, h, r, m)):
                    if table in (0, 1, 2):
                        e = P.power(bases[table], abs(dg) << (w * pos), d)
                        acc = P.compose(acc, P.inverse(e) if dg < 0 else e)
                    elif table == 3:
                        acc = P.compose(acc, P.inverse(leafs[h]) if mode == 2 else leafs[h])
                want = P.compose(P.inverse(leafs[h]) if mode == 2 else leafs[h], P.power(bases[h], r % (1 << 64), d) if r >= 0
                                 else P.inverse(P.power(bases[h], -r, d)))
                if h == 1:
                    want = P.compose(want, P.power(bases[2], (-m if mode == 1 else m) % M, d))
                assert t3(acc) == t3(want), (w, m, r, h)


def test_comb_shape_and_workspace_plan_of_kinds_3_and_4(lib):
    """kind 3: the width follows k (10 from k = 64 up), slots = k // w + 2 rounded up to even, ONE column per ciphertext --
    level_a holds slots / 2 records per ciphertext, so nothing is composed for c1 -- whatever exp_bits says; kind 4: an
    encryption's positions plus the leaf, two columns.  Regions disjoint and 256-byte aligned, total within 4 GiB, chunks
    on both sides of a boundary, pins honoured, bad arguments refused"""
    from cofhe_amd import engine
    assert engine.comb_shape(3, 1, 0, 128, 0, 0)[:2] == (10, 14)
    assert engine.comb_shape(3, 1, 0, 8, 0, 0)[:2] == (4, 4)
    assert engine.comb_shape(3, 1, 966, 128, 0, 0) == engine.comb_shape(3, 1, 0, 128, 0, 0)
    for kind in (3, 4):
        halves = 1 if kind == 3 else 2
        for w in (0, 2, 5, 8, 10):
            for k in (8, 128, 256):
                for bits in (0, 966):
                    ww, slots, big = engine.comb_shape(kind, 1 << 22, bits, k, w, 0)
                    assert ww == (w or ww) and 2 <= ww <= 10
                    want_slots = (0 if kind == 3 else bits // ww + 1) + k // ww + 1 + 1
                    assert slots == (want_slots + 1) // 2 * 2
                    for n in (1, big - 1, big, big + 1, 2 * big + 1, 1 << 22):
                        if n < 1:
                            continue
                        ww2, slots2, chunk = engine.comb_shape(kind, n, bits, k, w, 0)
                        assert (ww2, slots2) == (ww, slots) and chunk == min(n, big)
                        regs, total = engine.workspace_plan("comb", kind, n, bits, k, w, 0)
                        end = 0
                        for name, off, nbytes in regs:
                            assert off % 256 == 0 and off >= end
                            end = off + nbytes
                        assert end == total <= 4 << 30
                        r = {name: (off, nbytes) for name, off, nbytes in regs}
                        assert r["level_a"][1] == slots // 2 * chunk * halves * REC_BYTES
                        assert r["level_b"][1] == (slots + 3) // 4 * chunk * halves * REC_BYTES
    assert engine.comb_shape(3, 1000, 0, 128, 8, 33)[2] == 33
    assert engine.comb_shape(3, 20, 0, 128, 8, 33)[2] == 20
    assert engine.comb_shape(4, 1 << 22, 966, 128, 2, 1 << 30)[2] < 1 << 30
    for bad in [(3, 1, 0, 0, 0, 0), (4, 1, 10, 0, 8, 0), (3, 1, 0, 992, 8, 0), (4, 1, 993, 128, 0, 0), (3, 1, 0, 128, 11, 0),
                (5, 1, 0, 128, 0, 0), (3, 1 << 41, 0, 128, 0, 0)]:
        with pytest.raises(Exception):
            engine.comb_shape(*bad)
        with pytest.raises(Exception):
            engine.workspace_plan("comb", *bad)


def test_entry_points_refuse_bad_arguments_without_a_gpu(lib):
    """a mode outside 0..2 is COFHE_HIP_EINVAL before anything touches the device"""
    L = lib
    L.cofhe_hip_last_error.restype = C.c_char_p
    assert L.cofhe_hip_add_plain_records(None, None, None, None, None, None, None, None, C.c_uint64(0), C.c_uint32(128), C.c_int(3), None) == -1          # COFHE_HIP_EINVAL
    assert b"mode" in L.cofhe_hip_last_error()
