"""CPU: the sign from digit comparisons -- the Python reference by hand, compare.hpp (cofhe_amd/csrc), which k_cmp_rows and
k_cmp_close call, compiled for the host against that reference, the host-only shape entry of the C ABI, and the host harness's
usage.  Exact.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import compare_cases as CC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libcomparesim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "compare_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("compare.hpp", "plain_mm.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_reference_by_hand():
    """small numbers worked by hand, then the protocol's identity on Python integers.  l = 4, d = 2: u = 3 gives A = 8 - 3 = 5,
    B = 16 - 3 = 13, no wrap; u = 9 gives A = 15, B = 7, wrap.  r = 6 = (2, 1) in base 4 against t = 5 = (1, 1): S = +1 + 0 = 1,
    r >= t; against t = 13 = (1, 3): S = 1 - 2 = -1, r < t.  -13 mod 16 = 3; -0 is 0; 2^k + 5 keeps its low bits."""
    assert CC.thresholds(3, 4) == (5, 13, 0) and CC.thresholds(9, 4) == (15, 7, 1) and CC.thresholds(0, 4) == (8, 0, 1)
    assert CC.thresholds(8, 4) == (0, 8, 0)
    assert [CC.digit(6, j, 2) for j in range(2)] == [2, 1] and [CC.digit(13, j, 2) for j in range(2)] == [1, 3]
    assert CC.s_value(6, 5, 4, 2) == 1 and CC.s_value(6, 13, 4, 2) == -1 and CC.s_value(6, 6, 4, 2) == 0
    assert CC.low((13, 1), 4) == 3 and CC.low((0, 1), 4) == 0 and CC.low(((1 << 128) + 5, 0), 64) == 5
    assert CC.low(((1 << 128) + 5, 1), 64) == (1 << 64) - 5 and CC.low((1, 1), 64) == (1 << 64) - 1 and CC.low((1 << 64, 1), 64) == 0
    assert CC.rows([(6, 0)], 4, 2) == [(1, 0), (1, 0), (0, 0), (1, 1), (2, 0), (0, 0), (2, 1), (2, 1)]
    assert CC.sign_table(2) == [1, 1, 1, 1, 0, 0, 0, 0]
    assert CC.digits_of(17, 5) == 4 and CC.digits_of(64, 7) == 10 and CC.digits_of(32, 6) == 6
    # 32 bits: d = 5, 6, 7 cost 7 32 + 512 = 736, 6 64 + 256 = 640, 5 128 + 128 = 768; 8 bits: d = 3, 4, 5 cost 56, 48, 80;
    # 64 bits: d = 7, 8 cost 10 128 + 4096 = 5376, 8 256 + 1024 = 3072; 16 bits: d = 3, 4, 5 cost 304, 128, 192
    assert [CC.pick_digit_bits(b, k) for b, k in ((32, 128), (8, 8), (64, 128), (16, 128))] == [6, 4, 8, 4]
    assert CC.pick_digit_bits(2, 2) == 2 and CC.pick_digit_bits(65, 128) is None        # one digit of 2 bits: 4 + 8; no window of 65 bits
    rng = random.Random(20)
    for trial in range(20000):
        k = rng.choice((8, 128, 256))
        bits = rng.randrange(2, min(k, 64) + 1)
        d = rng.randrange(1, 9)
        if not CC.shape_ok(bits, d, k):
            continue
        x = rng.choice(CC.edges(bits)) if trial % 4 == 0 else rng.randrange(-(1 << (bits - 1)), 1 << (bits - 1))
        r = rng.choice((0, 1 << (bits - 1), (1 << k) - 1, rng.getrandbits(k)))
        assert CC.nonneg_by_protocol(x, r, k, bits, d) == int(x >= 0), (k, bits, d, x, r)
        # the opened value as a record with a set sign word, -0 and a magnitude of 2^k and above: the same u
        e = (x - r) % (1 << k)
        u = e % (1 << bits)
        assert CC.low(((1 << k) - e, 1), bits) == u and CC.low((e + (1 << k), 0), bits) == u
        assert CC.low((0, 1), bits) == 0
        # A and B differ in bit bits - 1 only, hence share every digit but the top one
        a, b, _ = CC.thresholds(u, bits)
        assert a ^ b == 1 << (bits - 1)
        n = CC.digits_of(bits, d)
        assert [CC.digit(a, j, d) for j in range(n - 1)] == [CC.digit(b, j, d) for j in range(n - 1)]
        assert CC.digit(a, n - 1, d) != CC.digit(b, n - 1, d)


def sim_thresholds(sim, vals, k, bits, d):
    n, cnt = CC.digits_of(bits, d), len(vals)
    e = CC.records(vals)
    u, a, b = (np.zeros(cnt, dtype=np.uint64) for _ in range(3))
    wrap = np.zeros(cnt, dtype=np.uint32)
    dig = np.zeros(cnt * 2 * n, dtype=np.uint32)
    ent = np.zeros(cnt * 2 * n, dtype=np.uint64)
    rc = sim.cmp_sim_thresholds(ptr(e), C.c_uint64(cnt), C.c_uint32(bits), C.c_uint32(d), C.c_uint32(k), ptr(u), ptr(a), ptr(b), ptr(wrap),
                                ptr(dig), ptr(ent))
    assert rc == 0
    return u, a, b, wrap, dig.reshape(cnt, 2, n), ent.reshape(cnt, 2, n)


@pytest.mark.parametrize("k,bits,d", CC.PARAMS)
def test_thresholds_digits_and_wrap_match_python_integers(sim, k, bits, d):
    """u, A, B, wrap, every digit of both thresholds and the tuple entry each selects, over the edge values and random ones"""
    vals = CC.values(bits, k, 300, random.Random(1000 * k + 10 * bits + d))
    u, a, b, wrap, dig, ent = sim_thresholds(sim, vals, k, bits, d)
    n = CC.digits_of(bits, d)
    for i, v in enumerate(vals):
        uu = CC.low(v, bits)
        aa, bb, ww = CC.thresholds(uu, bits)
        assert (int(u[i]), int(a[i]), int(b[i]), int(wrap[i])) == (uu, aa, bb, ww), v
        assert [int(x) for x in dig[i, 0]] == [CC.digit(aa, j, d) for j in range(n)]
        assert [int(x) for x in dig[i, 1]] == [CC.digit(bb, j, d) for j in range(n)]
        assert [int(x) for x in ent[i, 0]] == CC.entries(i, aa, bits, d) and [int(x) for x in ent[i, 1]] == CC.entries(i, bb, bits, d)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("k,bits,d", CC.PARAMS)
def test_rows_match_python_integers_word_for_word(sim, k, bits, d, shift):
    """the rows of the tuples through the body of k_cmp_rows, by 16-byte pieces into an aligned buffer and by dwords into one
    shifted by 4 bytes; the words behind the last record stay as they were"""
    rs = CC.values(bits, k, 5 if d >= 7 else 24, random.Random(k + bits + d))
    want = CC.records(CC.rows(rs, bits, d))
    raw = np.full(want.size + 16, 0xA5A5A5A5, dtype=np.uint32)
    off = (-(raw.ctypes.data // 4)) % 4 + shift
    out = raw[off:off + want.size]
    r = CC.records(rs)
    rc = sim.cmp_sim_rows(ptr(r), C.c_void_p(raw.ctypes.data + 4 * off), C.c_uint64(len(rs)), C.c_uint32(bits), C.c_uint32(d), C.c_uint32(k))
    assert rc == (4 if shift else 16)
    assert np.array_equal(out, want)
    assert (raw[:off] == 0xA5A5A5A5).all() and (raw[off + want.size:] == 0xA5A5A5A5).all()


def test_the_simulator_refuses_what_the_launchers_refuse(sim):
    assert sim.cmp_sim_max_digits() == CC.MAX_DIGITS
    rng = random.Random(3)
    for _ in range(3000):
        bits, d, k, lm = rng.randrange(0, 70), rng.randrange(0, 11), rng.choice((1, 2, 5, 8, 12, 64, 128, 639, 640)), rng.choice((4, 12))
        assert sim.cmp_sim_shape_ok(bits, d, k, lm) == int(CC.shape_ok(bits, d, k, lm)), (bits, d, k, lm)


def cmp_shape(L, bits, d, k, se=None, st=None):
    dg, en = C.c_uint32(77), C.c_uint32(77)
    if st is None:
        rc = L.cofhe_hip_cmp_shape(C.c_uint32(bits), C.c_uint32(d), C.c_uint32(k), C.c_uint32(0), None, C.c_uint32(0), None, C.byref(dg), C.byref(en))
    else:
        rc = L.cofhe_hip_cmp_shape(C.c_uint32(bits), C.c_uint32(d), C.c_uint32(k), C.c_uint32(len(se)), (C.c_uint32 * 8)(*se), C.c_uint32(len(st)),
                                   (C.c_uint32 * 9)(*st), C.byref(dg), C.byref(en))
    assert rc == 0 or (dg.value, en.value) == (77, 77)          # a refusal writes nothing
    return (dg.value, en.value) if rc == 0 else rc


def test_cmp_shape_gives_the_digits_or_refuses():
    """cofhe_hip_cmp_shape (host only): n and n 2^d; every parameter bound is COFHE_HIP_EINVAL (-1), every wrong tuple shape
    COFHE_HIP_ESHAPE (-2), one by one"""
    from cofhe_amd import load_library
    L = load_library()
    for k, bits, d in CC.PARAMS:
        n = CC.digits_of(bits, d)
        assert cmp_shape(L, bits, d, k) == (n, n << d)
        assert cmp_shape(L, bits, d, k, [33], [33, n, 1 << d]) == (n, n << d)
        assert cmp_shape(L, bits, d, k, [], [n, 1 << d]) == (n, n << d)
    assert cmp_shape(L, 2, 1, 8) == (2, 4) and cmp_shape(L, 64, 6, 128) == (11, 11 << 6)
    assert cmp_shape(L, 16, 4, 128, [1, 2, 3, 4, 5, 6], [1, 2, 3, 4, 5, 6, 4, 16]) == (4, 64)
    refused = {"bits = 1": (1, 1, 128), "bits = 0": (0, 1, 128), "bits = 65": (65, 8, 128), "bits > k": (9, 3, 8), "d = 0": (16, 0, 128),
               "d = 9": (16, 9, 128), "n + 1 = 13 > 12": (64, 5, 128), "n + 1 = 9 > k = 8": (8, 1, 8), "k = 0": (2, 1, 0),
               "k = 640": (16, 4, 640)}
    for why, (bits, d, k) in refused.items():
        assert cmp_shape(L, bits, d, k) == -1, why
        assert cmp_shape(L, bits, d, k, [5], [5, 4, 16]) == -1, why
    shapes = {"one dimension short": ([5], [5, 64]), "digits and entries swapped": ([5], [5, 16, 4]), "another n": ([5], [5, 3, 16]),
              "another 2^d": ([5], [5, 4, 8]), "another S": ([5], [6, 4, 16]), "S longer": ([5, 1], [5, 4, 16]), "no S": ([5], [4, 16]),
              "7 dimensions": ([1] * 7, [1] * 7 + [4, 16]), "empty": ([], [])}
    for why, (se, st) in shapes.items():
        assert cmp_shape(L, 16, 4, 128, se, st) == -2, why


def test_local_bench_lists_compare():
    import __graft_entry__ as g
    g.build()
    r = subprocess.run([os.path.join(ROOT, "cofhe_amd", "host", "local_bench")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    lines = [ln.strip() for ln in r.stderr.splitlines()]
    assert "compare [elements=256 [bits=32 [digit_bits=0 [runs=0]]]]" in lines
