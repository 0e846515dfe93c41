"""CPU: the exact floor division by small public divisors -- the bodies of k_plain_divmod, k_divx_prep and k_divx_rows
(cofhe_amd/csrc/plain_divmod.hpp) compiled for the host and run on the lane-group simulator against Python integers, the
protocol in Python integers exhaustively at k = 8, and the power-of-two identity of the rows.  Exact.  No kernel runs."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import div_cases as DC
import divx_cases as XC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libdivxsim.so")
PREFILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "divx_sim.cpp")
    deps = [src, os.path.join(HERE, "hostsim", "sim.cpp")] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in
                                                               ("plain_divmod.hpp", "plain_div.hpp", "plain_mm.hpp", "mp.hpp", "lane.hpp", "qf.hpp",
                                                                "form_io.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-DCOFHE_WG_GROUPS=32", "-o", _SO, src])
    L = C.CDLL(_SO)
    L.divx_entry_sim.restype = C.c_uint64
    L.sim_status()
    L.sim_flags()
    return L


def run_divmod(sim, nums, divs, k, rows, rc_want=0):
    """(the quotients' records, the remainders) of nums (pairs (magnitude, sign word)) by divs (element e reads divisor e mod len)"""
    n = len(nums)
    v, d = DC.records(nums), DC.int_records(divs)
    q = np.full(max(n, 1) * 32, PREFILL, dtype=np.uint32)              # the kernel must write every word of every record
    rem = np.full(max(n, 1), PREFILL, dtype=np.uint32)
    rc = sim.divx_divmod_sim(v.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint64(len(divs)), q.ctypes.data_as(C.c_void_p),
                             rem.ctypes.data_as(C.c_void_p), C.c_uint64(n), C.c_uint32(rows), C.c_uint32(k))
    assert rc == rc_want
    return q[:n * 32], rem[:n]


def run_rows(sim, rs, divs, k, rows, width, rc_want=0):
    n = len(rs)
    r, d = DC.int_records(rs), DC.int_records(divs)
    out = np.full(max(n, 1) * rows * 32, PREFILL, dtype=np.uint32)
    rc = sim.divx_rows_sim(r.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p), C.c_uint64(len(divs)), out.ctypes.data_as(C.c_void_p),
                           C.c_uint64(n), C.c_uint32(rows), C.c_uint32(k), C.c_uint32(width))
    assert rc == rc_want
    return out[:n * rows * 32]


def test_the_reference_and_the_negative_branch_identity():
    """the Python reference on small numbers worked by hand, and the identity the kernel uses on a negative residue -m: with
    q', rho' the quotient and the remainder of m - 1, the floor quotient is -(q' + 1) and the remainder D - 1 - rho'"""
    assert XC.divmod_centred((7, 0), 2, 8) == (3, 1) and XC.divmod_centred((7, 1), 2, 8) == (256 - 4, 1)
    assert XC.divmod_centred((255, 0), 3, 8) == (255, 2) and XC.divmod_centred((0, 1), 3, 8) == (0, 0)
    assert XC.divmod_centred((100, 0), 5, 8, rows=4) == (0, 0) and XC.divmod_centred((100, 0), 4097, 128) == (0, 0)
    assert XC.row_values(7, 3, 8, 5) == [2, 2, 3, 0, 0] and XC.row_values(256 - 7, 3, 8, 3) == [253, 254, 254]
    rng = random.Random(2)
    for _ in range(2000):
        m, D = rng.randrange(1, 1 << 40), rng.randrange(1, 4097)
        qp, rp = divmod(m - 1, D)
        assert divmod(-m, D) == (-(qp + 1), D - 1 - rp)


@pytest.mark.parametrize("k", DC.KBITS_CPU)
def test_divmod_body_matches_python_integers(sim, k):
    """C1: every case of div_cases with D <= 4096, element-wise divisors: set sign words, -0, magnitudes of 2^k and above, +-qD,
    +-(qD - 1), +-(qD + D - 1); quotient and remainder against Python's divmod of the centred residue; the status word stays
    clear"""
    cs = XC.cases(k)
    assert len(cs) >= 30 and {1, 2, 3} <= {D for _, D in cs}
    nums, divs = [c[0] for c in cs], [c[1] for c in cs]
    q, rem = run_divmod(sim, nums, divs, k, XC.MAX_ROWS)
    want = [XC.divmod_centred(v, D, k) for v, D in cs]
    DC.check_output(q, [w[0] for w in want], k)
    assert rem.tolist() == [w[1] for w in want]
    assert sim.sim_status() == 0


@pytest.mark.parametrize("k", (8, 128, 300))
@pytest.mark.parametrize("n_div", (1, 3, 12))
def test_divmod_broadcast_of_the_divisors(sim, k, n_div):
    """element e reads divisor e mod n_div: a scalar, three channels, element-wise"""
    rng = random.Random(41 * k + n_div)
    n = 12
    nums = [(rng.getrandbits(k), rng.randrange(2)) for _ in range(n)]
    divs = [rng.randrange(1, min(4097, 1 << (k - 1))) for _ in range(n_div)]
    q, rem = run_divmod(sim, nums, divs, k, XC.MAX_ROWS)
    want = [XC.divmod_centred(nums[e], divs[e % n_div], k) for e in range(n)]
    DC.check_output(q, [w[0] for w in want], k)
    assert rem.tolist() == [w[1] for w in want]
    assert sim.sim_status() == 0


@pytest.mark.parametrize("k", (8, 33, 128, 639))
def test_invalid_divisors_give_zero_zero_and_the_status_bit(sim, k):
    """C1: the invalid divisors of div_cases, a divisor above rows and D = 4097 give quotient 0, remainder 0 and CF_ST_DIV_CAP,
    each on its own; the valid elements next to them are divided all the same; D = rows is valid"""
    rng = random.Random(k)
    rows = 100 if k > 8 else 50
    bad = DC.invalid_divisors(k) + [rows + 1] + ([4097] if k > 13 else [])
    divs = [3] + bad + [rows]
    nums = [(rng.getrandbits(k), 0) for _ in divs]
    want = [XC.divmod_centred(v, D, k, rows) for v, D in zip(nums, divs)]
    assert want[1:-1] == [(0, 0)] * len(bad)
    q, rem = run_divmod(sim, nums, divs, k, rows)
    DC.check_output(q, [w[0] for w in want], k)
    assert rem.tolist() == [w[1] for w in want]
    assert sim.sim_status() == DC.ST_DIV_CAP
    for D in bad:
        q, rem = run_divmod(sim, [(5, 0)], [D], k, rows if D != 4097 else XC.MAX_ROWS)
        DC.check_output(q, [0], k)
        assert rem.tolist() == [0] and sim.sim_status() == DC.ST_DIV_CAP
    q, rem = run_divmod(sim, [(5, 0)], [(1 << k) + 3], k, rows)               # a magnitude of 2^k and above enters as its residue
    DC.check_output(q, [1], k)
    assert rem.tolist() == [2] and sim.sim_status() == 0


def test_divmod_refusals(sim):
    """kbits = 0 and 640, rows = 0 and 4097, no divisor, an element count that is no multiple of the divisor count: refused,
    nothing written"""
    assert sim.divx_sim_max_rows() == 4096
    for k, divs, n, rows in ((0, [3], 2, 8), (640, [3], 2, 8), (128, [3], 2, 0), (128, [3], 2, 4097), (128, [], 2, 8), (128, [3, 5], 3, 8)):
        q, rem = run_divmod(sim, [(9, 0)] * n, divs, k, rows, rc_want=-1)
        assert (q == PREFILL).all() and (rem == PREFILL).all()
    q, rem = run_divmod(sim, [(9, 0)], [4], 639, 4096)
    DC.check_output(q, [2], 639)
    assert rem.tolist() == [1]


@pytest.mark.parametrize("width", (4, 1), ids=["pieces16", "dwords"])
@pytest.mark.parametrize("k", XC.ROWS_KBITS)
def test_rows_body_matches_python_integers(sim, k, width):
    """C2: D in {1, 2, 3, 8, 100} (and 4096 where k allows), rows in {D, D + 3}, masks with m(r) in {0, 1, D - 1} of either sign and
    random ones: every record against Python, zero records beyond D, every word written over the prefill, in both access widths"""
    rng = random.Random(70 + k)
    for D in (1, 2, 3, 8, 100, 4096):
        if D >= 1 << (k - 1):
            continue
        for rows in (D, D + 3):
            if rows > XC.MAX_ROWS:
                continue
            rs = XC.masks(k, D, rng, extra=1 if D == 4096 else 3)
            if D == 4096:
                rs = rs[:2] + rs[-1:]
            out = run_rows(sim, rs, [D], k, rows, width)
            assert not (out.reshape(-1, 32)[:, :] == PREFILL).all(axis=1).any()
            want = [t for r in rs for t in XC.row_values(r, D, k, rows)]
            DC.check_output(out, want, k)
    assert sim.sim_status() == 0


def test_rows_with_element_wise_and_invalid_divisors(sim):
    """element i reads divisor i mod n_div; an invalid divisor (0, a set sign word, one above rows) gives `rows` zero records and
    CF_ST_DIV_CAP, and the elements next to it keep their rows"""
    k, rows = 128, 11
    rng = random.Random(5)
    rs = [rng.getrandbits(k) for _ in range(6)]
    for divs, status in (([3, 11], 0), ([7, 0, 5, -3, 12, 11], DC.ST_DIV_CAP)):
        out = run_rows(sim, rs, divs, k, rows, 4)
        want = [t for i, r in enumerate(rs) for t in XC.row_values(r, divs[i % len(divs)], k, rows)]
        DC.check_output(out, want, k)
        assert sim.sim_status() == status
    for kk, rr, divs, n in ((0, 4, [3], 2), (640, 4, [3], 2), (128, 0, [3], 2), (128, 4097, [3], 2), (128, 4, [], 2), (128, 4, [3, 2], 3)):
        assert (run_rows(sim, [5] * n, divs, kk, rr, 4, rc_want=-1) == PREFILL).all()              # refused, nothing written


def test_select_entry_is_64_bit_and_never_beyond_the_tuple(sim):
    """the entry k_divx_select reads: i rows + index in 64 bits, and entry i rows with the flag for an index of rows or more"""
    bad = C.c_int()
    for i, rows, index in ((0, 1, 0), (5, 3, 2), ((1 << 24) - 1, 4096, 4095), (1 << 40, 4096, 17)):
        assert sim.divx_entry_sim(C.c_uint64(i), C.c_uint32(rows), C.c_uint32(index), C.byref(bad)) == i * rows + index and bad.value == 0
    for i, rows, index in ((0, 1, 1), (5, 3, 3), (7, 4096, 0xFFFFFFFF), (1 << 40, 100, 100)):
        assert sim.divx_entry_sim(C.c_uint64(i), C.c_uint32(rows), C.c_uint32(index), C.byref(bad)) == i * rows and bad.value == 1


@pytest.mark.parametrize("D", XC.PROTOCOL_DIVISORS)
def test_the_protocol_is_exact_on_every_pair_without_a_wrap_at_8_bits(D):
    """C3: all 2^16 pairs (x, r) at k = 8: on every pair with s(x) = s(r) + s(e) the result is the floor quotient and x - D y is
    (m(r) + m(e)) mod D; no pair is left out; the other pairs are exactly the wrapping ones, and there the result differs"""
    k, M = 8, 256
    exact = wrapped = 0
    for x in range(M):
        sx = DC.centred(x, k)
        for r in range(M):
            e = (x - r) % M
            y = XC.protocol_result(x, r, D, k)
            if DC.centred(r, k) + DC.centred(e, k) == sx:
                assert DC.centred(y, k) == sx // D, (x, r)
                assert sx - D * DC.centred(y, k) == (DC.centred(r, k) % D + DC.centred(e, k) % D) % D == sx % D, (x, r)
                exact += 1
            else:
                assert abs(DC.centred(r, k) + DC.centred(e, k) - sx) == M
                wrapped += 1
    # the wrapping pairs of x are the |s(x)| masks of the division row's contract: sum over x of |s(x)|
    assert wrapped == sum(abs(DC.centred(x, k)) for x in range(M)) and exact + wrapped == M * M


@pytest.mark.parametrize("t", (1, 3, 7))
def test_power_of_two_rows_are_a_lookup_rotation(sim, t):
    """C4: for D = 2^t, T_j = g[(j + r) mod 2^t] with g[v] = q(r) + [v < m(r)], in Python and on the rows body"""
    rng = random.Random(t)
    for k in (8, 128):
        if t >= k - 1:
            continue
        D = 1 << t
        rs = XC.masks(k, D, rng)
        out = XC.u32_values(run_rows(sim, rs, [D], k, D, 4))
        for i, r in enumerate(rs):
            g = XC.pow2_table(r, t, k)
            rot = [g[(j + r) % D] for j in range(D)]
            assert rot == XC.row_values(r, D, k, D) == out[i * D:(i + 1) * D], (k, r)
