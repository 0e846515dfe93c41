"""GPU: exact floor division of ciphertext tensors by small public divisors from one opened value
(cofhe_amd/csrc/divide_exact.hip): k_plain_divmod and the rows of k_divx_prep / k_divx_rows against Python integers and against
the lookup rotation, the tuples against the fresh encryption of the rows, the closing step against the index gather and the
plaintext addend byte for byte and through decryption, the whole protocol next to the inexact division pair, the refusals and
the guards, and the protocol through the C++ host layer."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import div_cases as DC
import divx_cases as XC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL, ESHAPE = -1, -2
REC = 168
CT_WORDS = 2 * REC
WG_ELEMENTS = 32                             # elements of a k_plain_divmod workgroup (plain_div.hpp: PDV_GROUPS)
PREFILL = 0xA5A5A5A5 - (1 << 32)             # as int32: every word must be written


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def divmod_gpu(E, torch, nums, divs, k, rows):
    """(the quotients' records, the remainders) of nums (pairs (magnitude, sign word)) by divs, one launch"""
    n = len(nums)
    q = torch.full((n * 32,), PREFILL, dtype=torch.int32, device="cuda")
    rem = torch.full((n,), PREFILL, dtype=torch.int32, device="cuda")
    dv, dd = dev(torch, DC.records(nums)), dev(torch, DC.int_records(divs))
    E.divmod_plain_records(dv.data_ptr(), dd.data_ptr(), len(divs), q.data_ptr(), rem.data_ptr(), n, rows, k)
    torch.cuda.synchronize()
    return host(q), host(rem).tolist()


def check_divmod(E, torch, nums, divs, k, rows):
    q, rem = divmod_gpu(E, torch, nums, divs, k, rows)
    want = [XC.divmod_centred(nums[e], divs[e % len(divs)], k, rows) for e in range(len(nums))]
    DC.check_output(q, [w[0] for w in want], k)
    assert rem == [w[1] for w in want]


def rows_gpu(E, torch, rs, divs, k, rows, offset_words=0):
    """the rows' records of the masks rs; offset_words = 1 puts the output 4 bytes off a 16-byte boundary (the dword route)"""
    n = len(rs)
    buf = torch.full((n * rows * 32 + 4,), PREFILL, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    dr, dd = dev(torch, DC.int_records(rs)), dev(torch, DC.int_records(divs))
    E.divx_rows_records(dr.data_ptr(), dd.data_ptr(), len(divs), buf.data_ptr() + 4 * offset_words, n, rows, k)
    torch.cuda.synchronize()
    h = host(buf)
    keep = np.ones(len(h), dtype=bool)
    keep[offset_words:offset_words + n * rows * 32] = False
    assert (h[keep] == 0xA5A5A5A5).all(), "a word outside the output was written"
    return h[offset_words:offset_words + n * rows * 32]


# ---- G1: k_plain_divmod ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", DC.KBITS_GPU)
def test_divmod_matches_python_integers(tiny, k):
    """every case of div_cases with D <= 4096 (set sign words, -0, magnitudes of 2^k and above, multiples of D and their
    neighbours of either sign) element-wise in one launch: quotient and remainder exact, every word of the output written"""
    import torch
    E = engine(setup(tiny)[0])
    cs = XC.cases(k)
    check_divmod(E, torch, [c[0] for c in cs], [c[1] for c in cs], k, XC.MAX_ROWS)
    assert E.device_status(clear=True) == 0


@pytest.mark.parametrize("n", [1, 7, 8, 9, WG_ELEMENTS - 1, WG_ELEMENTS, WG_ELEMENTS + 1])
def test_divmod_sizes_and_broadcast(tiny, n):
    """one wavefront's 8 groups and one workgroup's elements, each with one below and one above, at k = 128 with a scalar, a
    per-channel (where 3 divides n) and an element-wise divisor; one launch each, under its own profile name"""
    import torch
    E = engine(setup(tiny)[0])
    k = 128
    rng = random.Random(n)
    nums = [(rng.getrandbits(k), rng.randrange(2)) for _ in range(n)]
    E.profile_read("k_plain_divmod", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        launches = 0
        for n_div in (1, 3, n):
            if n % n_div:
                continue
            divs = [rng.randrange(1, 1 << rng.choice((1, 3, 8, 12))) for _ in range(n_div)]
            check_divmod(E, torch, nums, divs, k, XC.MAX_ROWS)
            launches += 1
        assert E.profile_read("k_plain_divmod", clear=True)[1] == launches
    finally:
        E.set_option("profile_kernels", 0)
        E.profile_read("k_plain_divmod", clear=True)
    assert E.device_status(clear=True) == 0


# ---- G2: k_divx_prep and k_divx_rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (8, 128))
@pytest.mark.parametrize("n", (1, 9, 33))
def test_rows_match_python_integers_in_both_access_widths(tiny, k, n):
    """D in {1, 3, 8, 100}, rows in {D, D + 3}: every record against Python, zero records beyond D, every word written and none
    outside, on a 16-byte-aligned output and on one offset by 4 bytes; masks with m(r) in {0, 1, D - 1} of either sign first"""
    import torch
    E = engine(setup(tiny)[0])
    rng = random.Random(100 * k + n)
    for D in (1, 3, 8, 100):
        rs = (XC.masks(k, D, rng, extra=n) * 2)[:n]
        for rows in (D, D + 3):
            want = [t for r in rs for t in XC.row_values(r, D, k, rows)]
            for off in (0, 1):
                DC.check_output(rows_gpu(E, torch, rs, [D], k, rows, off), want, k)
    assert E.device_status(clear=True) == 0


def test_rows_at_the_largest_divisor(tiny):
    """n = 3, D = rows = 4096 at k = 128: 12 288 records against Python"""
    import torch
    E = engine(setup(tiny)[0])
    k, D = 128, 4096
    rng = random.Random(4096)
    rs = [(5 * D) % (1 << k), (-3 * D + D - 1) % (1 << k), rng.getrandbits(k)]
    got = rows_gpu(E, torch, rs, [D], k, D).reshape(-1, 32)
    assert not got[:, 4:].any()
    vals = [int.from_bytes(row[:4].tobytes(), "little") for row in got]
    assert vals == [t for r in rs for t in XC.row_values(r, D, k, D)]


@pytest.mark.parametrize("t", (1, 3, 7))
def test_power_of_two_rows_equal_the_lookup_rotation(tiny, t):
    """for D = 2^t the rows are byte-equal to cofhe_hip_lut_rotate_records on the per-element table g[v] = q(r) + [v < m(r)]: an
    existing kernel as an independent oracle, element-wise tables, at k = 8 (t < 7) and k = 128"""
    import torch
    E = engine(setup(tiny)[0])
    rng = random.Random(t)
    for k in (8, 128):
        if t >= k - 1:
            continue
        D = 1 << t
        rs = XC.masks(k, D, rng, extra=3)
        n = len(rs)
        table = dev(torch, DC.int_records([g for r in rs for g in XC.pow2_table(r, t, k)]))
        want = torch.zeros(n * D * 32, dtype=torch.int32, device="cuda")
        E.lut_rotate_records(table.data_ptr(), n, dev(torch, DC.int_records(rs)).data_ptr(), want.data_ptr(), n, t)
        torch.cuda.synchronize()
        assert np.array_equal(rows_gpu(E, torch, rs, [D], k, D), host(want))


def test_rows_element_wise_divisors(tiny):
    """element i reads divisor i mod n_div: per-channel and element-wise divisors of different sizes under one `rows`"""
    import torch
    E = engine(setup(tiny)[0])
    k, rows, n = 128, 12, 6
    rng = random.Random(12)
    rs = [rng.getrandbits(k) for _ in range(n)]
    for divs in ([5, 12, 1], [2, 3, 4, 7, 11, 12]):
        want = [t for i, r in enumerate(rs) for t in XC.row_values(r, divs[i % len(divs)], k, rows)]
        DC.check_output(rows_gpu(E, torch, rs, divs, k, rows), want, k)


# ---- G3: the tuples ------------------------------------------------------------------------------------------------------------
def test_tuples_are_the_fresh_encryption_of_the_rows(params128):
    """divx_tuples_records at n = 9, D = 8 equals encrypt_fresh_records over the rows of divx_rows_records byte for byte"""
    import torch
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    n, D = 9, 8
    rng = random.Random(98)
    rs = [rng.getrandbits(k) for _ in range(n)]
    rhos = [rng.randrange(bound) for _ in range(n * D)]
    dr, dd, drho = dev(torch, DC.int_records(rs)), dev(torch, DC.int_records([D])), dev(torch, DC.int_records(rhos))
    rows = torch.zeros(n * D * 32, dtype=torch.int32, device="cuda")
    E.divx_rows_records(dr.data_ptr(), dd.data_ptr(), 1, rows.data_ptr(), n, D, k)
    want = torch.zeros(n * D * CT_WORDS, dtype=torch.int32, device="cuda")
    E.encrypt_fresh_records(rows.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], want.data_ptr(), n * D, k)
    out = torch.zeros_like(want)
    E.divx_tuples_records(dr.data_ptr(), dd.data_ptr(), 1, drho.data_ptr(), recs["h"], recs["pk"], recs["f"], out.data_ptr(), n, D, k)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert decrypt(E, torch, prm, out, n * D, k) == [t for r in rs for t in XC.row_values(r, D, k, D)]


# ---- G4: the closing step ------------------------------------------------------------------------------------------------------
def closing_inputs(E, torch, prm, n, D, seed, shared_c1):
    """values xs of up to 64 bits and both signs, uniform masks rs, the opened values es = xs - rs, and the tuples: the rows of
    Python freshly encrypted"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    M = 1 << k
    xs = ([0, M - 1, (1 << 64) - 1, M - (1 << 64)] + [rng.choice((1, -1)) * rng.getrandbits(64) % M for _ in range(n)])[-n:]
    rs = [rng.getrandbits(k) for _ in range(n)]
    es = [(x - r) % M for x, r in zip(xs, rs)]
    assert all(DC.centred(x, k) == DC.centred(r, k) + DC.centred(e, k) for x, r, e in zip(xs, rs, es))
    r0 = rng.randrange(bound)
    plain = [t for r in rs for t in XC.row_values(r, D, k, D)]
    tuples = fresh(E, torch, recs, plain, [r0 if shared_c1 else rng.randrange(bound) for _ in plain], k)
    return xs, rs, es, tuples


@pytest.mark.parametrize("shared_c1", [True, False], ids=["shared_c1", "distinct_c1"])
@pytest.mark.parametrize("D", (3, 8))
@pytest.mark.parametrize("n", (1, 8, 33))
def test_close_is_the_gather_and_the_plaintext_addend_and_decrypts(params128, n, D, shared_c1):
    """divx_close_records equals gather_records by the Python-computed entries followed by add_plain_records (mode 0) with the
    Python quotients, byte for byte; it decrypts to floor(s(x) / D); the tuples stay as they were"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    xs, rs, es, tuples = closing_inputs(E, torch, prm, n, D, 1000 * n + 10 * D + shared_c1, shared_c1)
    keep = tuples.clone()
    qm = [XC.divmod_centred((e, 0), D, k) for e in es]
    index = dev(torch, np.array([i * D + m for i, (_, m) in enumerate(qm)], dtype=np.uint32))
    picked = torch.zeros(n * CT_WORDS, dtype=torch.int32, device="cuda")
    E.gather_records(tuples.data_ptr(), n * D, index.data_ptr(), 0, picked.data_ptr(), n, CT_WORDS)
    want = torch.zeros_like(picked)
    E.add_plain_records(picked.data_ptr(), dev(torch, DC.int_records([q for q, _ in qm])).data_ptr(), recs["f"], want.data_ptr(), n, k, mode=0)
    out = torch.zeros_like(picked)
    de, dd = dev(torch, DC.int_records(es)), dev(torch, DC.int_records([D]))
    E.divx_close_records(de.data_ptr(), dd.data_ptr(), 1, tuples.data_ptr(), D, recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(tuples, keep)
    assert decrypt(E, torch, prm, out, n, k) == [(DC.centred(x, k) // D) % (1 << k) for x in xs]
    assert E.device_status(clear=True) == 0


def test_close_tensors_bytes_round_trips_and_refuses_a_wrong_tuple_shape(params128):
    """divx_close_tensors_bytes on a [2, 3] tensor with a scalar and a per-channel divisor returns the serialised result of
    divx_close_records, a tensor that passes the oracle's validation; tuples of another shape and divisors of another shape are
    COFHE_HIP_ESHAPE"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    n, D = 6, 5
    xs, rs, es, tuples = closing_inputs(E, torch, prm, n, D, 65, False)
    out = torch.zeros(n * CT_WORDS, dtype=torch.int32, device="cuda")
    de, dd = dev(torch, DC.int_records(es)), dev(torch, DC.int_records([D]))
    E.divx_close_records(de.data_ptr(), dd.data_ptr(), 1, tuples.data_ptr(), D, recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    tb = E.records_to_bytes(host(tuples), [2, 3, D])
    for shape, ds in (([1], [D]), ([3], [D] * 3), ([2, 3], [D] * 6)):
        got = E.divx_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes(shape, ds), tb, recs["f"], k)
        assert got == E.records_to_bytes(host(out), [2, 3])
    assert O.check_tensor(delta, got) == 1
    shp, r2 = E.bytes_to_records(got)
    assert list(shp) == [2, 3]
    assert decrypt(E, torch, prm, dev(torch, r2), n, k) == [(DC.centred(x, k) // D) % (1 << k) for x in xs]
    for call in (lambda: E.divx_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([1], [D]), E.records_to_bytes(host(tuples), [3, 2, D]), recs["f"], k),
                 lambda: E.divx_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([1], [D]), E.records_to_bytes(host(tuples), [6, D]), recs["f"], k),
                 lambda: E.divx_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([1], [D]), E.records_to_bytes(host(tuples), [2, 3 * D]), recs["f"], k),
                 lambda: E.divx_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([2], [D, D]), tb, recs["f"], k)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == ESHAPE
    assert E.divx_shape([2, 3], [2, 3, 4096]) == 4096
    for st in ([2, 3, 4097], [2, 3, 0], [2, 3], [3, 2, 5]):
        with pytest.raises(CofheHipError) as ei:
            E.divx_shape([2, 3], st)
        assert ei.value.code == ESHAPE


# ---- G5: the whole protocol ----------------------------------------------------------------------------------------------------
def protocol(E, torch, prm, xs, rs, D, inexact=False):
    """[x] and the tuples ([r], [T]) made by divx_tuples_records, e = Dec([x] - [r]) opened, [y] closed and decrypted; with
    inexact also what the division pair ([r], [r_q]) and div_close_records give on the same x and r"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(len(xs) + k + D)
    n = len(xs)
    enc = lambda ms: fresh(E, torch, recs, ms, [rng.randrange(bound) for _ in ms], k)      # noqa: E731
    dd, dr = dev(torch, DC.int_records([D])), dev(torch, DC.int_records(rs))
    drho = dev(torch, DC.int_records([rng.randrange(bound) for _ in range(n * D)]))
    tuples = torch.zeros(n * D * CT_WORDS, dtype=torch.int32, device="cuda")
    E.divx_tuples_records(dr.data_ptr(), dd.data_ptr(), 1, drho.data_ptr(), recs["h"], recs["pk"], recs["f"], tuples.data_ptr(), n, D, k)
    cx, cr = enc(xs), enc(rs)
    diff = torch.zeros_like(cx)
    E.sub_ciphertext_records(cx.data_ptr(), cr.data_ptr(), diff.data_ptr(), n)
    torch.cuda.synchronize()
    es = decrypt(E, torch, prm, diff, n, k)
    assert es == [(x - r) % (1 << k) for x, r in zip(xs, rs)]
    de = dev(torch, DC.int_records(es))
    out = torch.zeros_like(cx)
    E.divx_close_records(de.data_ptr(), dd.data_ptr(), 1, tuples.data_ptr(), D, recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    ys = decrypt(E, torch, prm, out, n, k)
    if not inexact:
        return ys
    crq = enc([DC.divfloor((r, 0), D, k) for r in rs])
    old = torch.zeros_like(cx)
    E.div_close_records(de.data_ptr(), dd.data_ptr(), 1, crq.data_ptr(), recs["f"], old.data_ptr(), n, k)
    torch.cuda.synchronize()
    return ys, decrypt(E, torch, prm, old, n, k)


def test_the_whole_protocol_at_8_bits_is_exact_where_the_pair_is_not(tiny):
    """k = 8, every x with |x| <= 2^(k-2), D in {2, 3, 7, 8, 127}, masks without a wrap: every decrypted result equals the floor
    quotient; the existing division pair on the same (x, r) gives one less for at least one element of every divisor and is
    never otherwise wrong -- the capability this protocol adds"""
    import torch
    prm = tiny
    delta, k, forms, recs, _ = setup(prm)
    assert k == 8
    E = engine(delta)
    rng = random.Random(85)
    M = 1 << k
    xs = [x % M for x in range(-(1 << (k - 2)), (1 << (k - 2)) + 1)]
    for D in (2, 3, 7, 8, 127):
        rs = DC.no_wrap_masks(xs, k, rng)
        ys, old = protocol(E, torch, prm, xs, rs, D, inexact=True)
        want = [(DC.centred(x, k) // D) % M for x in xs]
        assert ys == want, D
        off = [(w - o) % M for w, o in zip(want, old)]
        assert set(off) <= {0, 1} and 1 in off, D
    assert E.device_status(clear=True) == 0


def test_the_whole_protocol_at_128_bits_is_exact(params128):
    """64 elements of up to 64 bits and both signs, uniform masks (a wrap has probability 2^-64 per element: no allowance is
    made), D in {3, 256, 1000}: all exact"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    rng = random.Random(1285)
    n, M = 64, 1 << k
    xs = [0, 1, M - 1, (1 << 64) - 1, M - ((1 << 64) - 1)] + [rng.choice((1, -1)) * rng.getrandbits(64) % M for _ in range(n - 5)]
    for D in (3, 256, 1000):
        rs = [rng.getrandbits(k) for _ in range(n)]
        assert protocol(E, torch, prm, xs, rs, D) == [(DC.centred(x, k) // D) % M for x in xs], D
    assert E.device_status(clear=True) == 0


# ---- G6: refusals and guards ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_intact(params128):
    """kbits out of 1..639, rows out of 1..4096, n_div = 0, n no multiple of n_div and an output overlapping an input:
    COFHE_HIP_EINVAL at every entry point, with the prefill of every output intact; n = 0 does nothing"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    n, rows, w = 4, 3, 4
    ins = torch.zeros((2 * n) * 32, dtype=torch.int32, device="cuda")            # [values | divisors]
    ins[:n * 32] = dev(torch, DC.int_records([100, 200, 300, 400]))
    ins[n * 32:] = dev(torch, DC.int_records([3, 2, 3, 1]))
    pv, pd = ins.data_ptr(), ins.data_ptr() + n * 32 * w
    rho = dev(torch, DC.int_records([7] * (n * rows)))
    tuples = torch.full((n * rows * CT_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    outs = torch.full((n * rows * CT_WORDS,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    po, pr = outs.data_ptr(), outs.data_ptr() + n * 32 * w
    h, pk, f = recs["h"], recs["pk"], recs["f"]
    bad_shapes = ((n, 0, rows, n), (n, 640, rows, n), (n, k, 0, n), (n, k, 4097, n), (n, k, rows, 0), (n, k, rows, 3))
    calls = []
    for nn, kk, rr, nd in bad_shapes:
        calls += [lambda nn=nn, kk=kk, rr=rr, nd=nd: E.divmod_plain_records(pv, pd, nd, po, pr, nn, rr, kk),
                  lambda nn=nn, kk=kk, rr=rr, nd=nd: E.divx_rows_records(pv, pd, nd, po, nn, rr, kk),
                  lambda nn=nn, kk=kk, rr=rr, nd=nd: E.divx_tuples_records(pv, pd, nd, rho.data_ptr(), h, pk, f, po, nn, rr, kk),
                  lambda nn=nn, kk=kk, rr=rr, nd=nd: E.divx_close_records(pv, pd, nd, tuples.data_ptr(), rr, f, po, nn, kk)]
    calls += [lambda: E.divmod_plain_records(pv, pd, n, pv, pr, n, rows, k),                      # the quotients onto the values
              lambda: E.divmod_plain_records(pv, pd, n, po, pd, n, rows, k),                      # the remainders onto the divisors
              lambda: E.divmod_plain_records(pv, pd, n, po, po + w, n, rows, k),                  # the remainders onto the quotients
              lambda: E.divx_rows_records(pv, pd, n, pd - w, n, rows, k),                         # one word of the masks
              lambda: E.divx_rows_records(pv, pd, n, pd, n, rows, k),
              lambda: E.divx_tuples_records(pv, pd, n, rho.data_ptr(), h, pk, f, rho.data_ptr(), n, rows, k),
              lambda: E.divx_tuples_records(pv, pd, n, rho.data_ptr(), h, pk, f, pv, n, rows, k),
              lambda: E.divx_close_records(pv, pd, n, tuples.data_ptr(), rows, f, tuples.data_ptr(), n, k),
              lambda: E.divx_close_records(pv, pd, n, tuples.data_ptr(), rows, f, pv, n, k)]
    before = [t.clone() for t in (ins, rho, tuples, outs)]
    for call in calls:
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    E.divmod_plain_records(0, 0, 1, 0, 0, 0, rows, k)                                # nothing to do
    E.divx_rows_records(0, 0, 1, 0, 0, rows, k)
    E.divx_tuples_records(0, 0, 1, 0, h, pk, f, 0, 0, rows, k)
    E.divx_close_records(0, 0, 1, 0, rows, f, 0, 0, k)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((ins, rho, tuples, outs), before))
    assert E.device_status(clear=True) == 0


def test_invalid_divisors_give_zero_results_and_read_nothing_out_of_range(params128):
    """a divisor above rows, a negative and a zero divisor record: quotient 0, remainder 0, zero rows and the division bit of the
    status word, which this test reads with clear=True; the closing step then copies entry 0 of the element's tuple, whose
    buffer ends exactly at the end of its allocation (marked entries show which one), and adds nothing; the valid elements next to them are exact"""
    import torch
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    assert E.device_status(clear=True) == 0
    rng = random.Random(66)
    rows, M = 4, 1 << k
    divs = [3, rows + 1, -2, 0, rows]
    n = len(divs)
    nums = [(rng.getrandbits(64), 0) for _ in divs]
    check_divmod(E, torch, nums, divs, k, rows)
    assert E.device_status(clear=True) == DC.ST_DIV_CAP
    rs = [rng.getrandbits(k) for _ in divs]
    want = [t for r, D in zip(rs, divs) for t in XC.row_values(r, D, k, rows)]
    assert want[rows:4 * rows] == [0] * (3 * rows)
    DC.check_output(rows_gpu(E, torch, rs, divs, k, rows), want, k)
    assert E.device_status(clear=True) == DC.ST_DIV_CAP
    # the tuples at the very end of an allocation: n rows ciphertexts and not a word more
    pool = torch.zeros(3 * n * rows * CT_WORDS, dtype=torch.int32, device="cuda")
    tuples = pool[2 * n * rows * CT_WORDS:]
    plain = [t if XC.valid_divisor(divs[j // rows], k, rows) else 10 * (j // rows) + j % rows + 1 for j, t in enumerate(want)]
    tuples.copy_(fresh(E, torch, recs, plain, [rng.randrange(bound) for _ in plain], k))
    xs = [v for v, _ in nums]
    es = [(x - r) % M for x, r in zip(xs, rs)]
    out = torch.zeros(n * CT_WORDS, dtype=torch.int32, device="cuda")
    de, dd = dev(torch, DC.int_records(es)), dev(torch, DC.int_records(divs))
    E.divx_close_records(de.data_ptr(), dd.data_ptr(), n, tuples.data_ptr(), rows, recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    assert E.device_status(clear=True) == DC.ST_DIV_CAP
    ys = decrypt(E, torch, prm, out, n, k)
    assert ys == [xs[0] // 3, 11, 21, 31, xs[4] // rows]             # entry 0 of the element's own tuple, nothing added
    assert E.device_status(clear=True) == 0


# ---- G7: the host layer --------------------------------------------------------------------------------------------------------
def test_exact_division_through_the_host_layer(tmp_path):
    """local_bench divide_exact 64: a scalar divisor, per-channel divisors, Nearest rounding, truncate_exact at t = 8 and t = 16
    (two rounds), the remainder, decompose (3 digits of 8 bits of 20-bit values, recombined) and the exact 2 x 2 average pool
    through the single-key and the 2-of-3 threshold client EQUAL the plaintext integers, with ONE opened value per element and
    round, and the tensor it serialises is valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "divide_exact", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    assert r.stdout.count("opened_values 64,") == 10, r.stdout                  # five one-round calls per client
    assert r.stdout.count("truncate_exact by 2^16 over 64 elements, opened_values 128,") == 2, r.stdout
    assert r.stdout.count("decompose into 3 digits of 8 bits over 64 elements, opened_values 128:") == 2, r.stdout
    assert "avg_pool2d_exact: ok" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_divide_exact.bin", "rb").read()) == 1


def test_exact_division_timed_leg_through_the_host_layer(tmp_path):
    """local_bench divide_exact 8 1: the timed scalar division, at the smallest size that keeps the per-channel divisors and the
    2 x 2 average pool (a multiple of 4)"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "divide_exact", "8", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("divide_exact_json: ")]
    j = json.loads(line[len("divide_exact_json: "):])
    assert list(j) == ["E", "runs", "divide_exact_ms", "divide_exact_ms_min_max"]
