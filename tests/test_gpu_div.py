"""GPU: division of ciphertext tensors by public divisors from one opened value (cofhe_amd/csrc/divide.hip): k_plain_divfloor
against Python integers, the closing step and its bytes entry point against the plaintext addend byte for byte and through
decryption, the whole protocol at the ABI, the refusals, and the protocol through the C++ host layer."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import div_cases as DC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL = -1
REC = 168
WG_ELEMENTS = 32                             # elements of a k_plain_divfloor workgroup (plain_div.hpp: PDV_GROUPS)


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def divfloor(E, torch, nums, divs, k):
    """the quotients' records of nums (pairs (magnitude, sign word)) by divs (integers; element e reads divisor e mod len(divs))"""
    n = len(nums)
    q = torch.full((n * 32,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")        # every word must be written
    dv, dd = dev(torch, DC.records(nums)), dev(torch, DC.int_records(divs))
    E.divfloor_plain_records(dv.data_ptr(), dd.data_ptr(), len(divs), q.data_ptr(), n, k)
    torch.cuda.synchronize()
    return host(q)


@pytest.mark.parametrize("k", DC.KBITS_GPU)
def test_divfloor_matches_python_integers(tiny, k):
    """every family of div_cases (the divisors 1, 2, 3, 2^t, 2^(k-1) - 1, one limb, two limbs, full width; 0, 1, -1, the ends of
    the range, multiples of D and their neighbours of either sign, |v| < D, set sign words, magnitudes of 2^k and above, -0; the
    add-back family of mp_divrem_norm) element-wise in one launch, exact, every word of the output written"""
    import torch
    E = engine(setup(tiny)[0])
    cs = DC.cases(k)
    got = divfloor(E, torch, [c[0] for c in cs], [c[1] for c in cs], k)
    DC.check_output(got, [DC.divfloor(v, D, k) for v, D in cs], k)


@pytest.mark.parametrize("n", [1, 7, 8, 9, WG_ELEMENTS - 1, WG_ELEMENTS, WG_ELEMENTS + 1])
def test_divfloor_sizes_and_broadcast(tiny, n):
    """one wavefront's 8 groups and one workgroup's elements, each with one below and one above, at k = 128 with a scalar, a
    per-channel (where 3 divides n) and an element-wise divisor; one launch each, under its own profile name"""
    import torch
    E = engine(setup(tiny)[0])
    k = 128
    rng = random.Random(n)
    nums = [(rng.getrandbits(k), rng.randrange(2)) for _ in range(n)]
    E.profile_read("k_plain_divfloor", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        launches = 0
        for n_div in (1, 3, n):
            if n % n_div:
                continue
            divs = [rng.randrange(1, 1 << rng.choice((3, 31, 64, k - 1))) for _ in range(n_div)]
            DC.check_output(divfloor(E, torch, nums, divs, k), [DC.divfloor(nums[e], divs[e % n_div], k) for e in range(n)], k)
            launches += 1
        assert E.profile_read("k_plain_divfloor", clear=True)[1] == launches
    finally:
        E.set_option("profile_kernels", 0)
        E.profile_read("k_plain_divfloor", clear=True)


def test_invalid_divisors_set_the_status_bit(tiny):
    """0, 2^(k-1), 2^k - 1, a residue of 0 and a set sign word give quotient 0 and the division bit of the status word, which
    this test reads with clear=True; the valid elements of the same launch are divided"""
    import torch
    E = engine(setup(tiny)[0])
    assert E.device_status(clear=True) == 0
    for k in (8, 128):
        divs = [3] + DC.invalid_divisors(k) + [1]
        nums = [((1 << k) - 2 - i, 0) for i in range(len(divs))]
        DC.check_output(divfloor(E, torch, nums, divs, k), [DC.divfloor(v, D, k) for v, D in zip(nums, divs)], k)
        assert E.device_status(clear=True) == DC.ST_DIV_CAP
    DC.check_output(divfloor(E, torch, [(9, 0)], [3], 8), [3], 8)
    assert E.device_status(clear=True) == 0


def test_divfloor_refusals(tiny):
    """n no multiple of n_div, n_div = 0, an output that overlaps the numerators or the divisors, kbits = 0 and 640:
    COFHE_HIP_EINVAL and nothing written; n = 0 does nothing; kbits = 639 runs"""
    import torch
    from cofhe_amd import CofheHipError
    E = engine(setup(tiny)[0])
    n, w = 4, 4
    buf = torch.empty((3 * n) * 32, dtype=torch.int32, device="cuda")          # [numerators | divisors | output]
    buf[:n * 32] = dev(torch, DC.int_records([100, 200, 300, 400]))
    buf[n * 32:2 * n * 32] = dev(torch, DC.int_records([3, 5, 7, 9]))
    buf[2 * n * 32:].fill_(0x5A5A5A5A)
    before = buf.clone()
    pv, pd, pq = buf.data_ptr(), buf.data_ptr() + n * 32 * w, buf.data_ptr() + 2 * n * 32 * w
    for call in (lambda: E.divfloor_plain_records(pv, pd, 3, pq, n, 128), lambda: E.divfloor_plain_records(pv, pd, 0, pq, n, 128),
                 lambda: E.divfloor_plain_records(pv, pd, n, pv, n, 128),                     # onto the numerators
                 lambda: E.divfloor_plain_records(pv, pd, n, pd - w, n, 128),                 # one word of the numerators
                 lambda: E.divfloor_plain_records(pv, pd, n, pq - w, n, 128),                 # one word of the divisors
                 lambda: E.divfloor_plain_records(pv, pd, n, pq, n, 0), lambda: E.divfloor_plain_records(pv, pd, n, pq, n, 640)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    E.divfloor_plain_records(0, 0, 1, 0, 0, 128)                     # nothing to do
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    E.divfloor_plain_records(pv, pd, n, pq, n, 639)
    torch.cuda.synchronize()
    DC.check_output(host(buf[2 * n * 32:]), [33, 40, 42, 44], 639)


def closing_inputs(E, torch, prm, n, seed, shared_c1):
    """opened values e, divisors (one per element), the masks' quotients r_q in Python and [r_q] freshly encrypted"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    es = [0, 1, (1 << k) - 1, 1 << (k - 1), (1 << (k - 1)) - 1] + [rng.getrandbits(k) for _ in range(n - 5)]
    ds = DC.divisors(k, rng)
    divs = [ds[i % len(ds)] for i in range(n)]
    rq = [DC.divfloor((rng.getrandbits(k), 0), D, k) for D in divs]
    r0 = rng.randrange(bound)
    rqc = fresh(E, torch, recs, rq, [r0 if shared_c1 else rng.randrange(bound) for _ in range(n)], k)
    return es, divs, rq, rqc


@pytest.mark.parametrize("shared_c1", [True, False], ids=["shared_c1", "distinct_c1"])
def test_div_close_is_the_plaintext_addend_and_decrypts(params128, shared_c1):
    """div_close_records at 17 elements equals add_plain_records (mode 0) on [r_q] with the quotients of Python byte for byte,
    decrypts to r_q + e_q mod 2^k, leaves [r_q] as it was, and div_close_tensors_bytes returns the same tensor serialised: a
    tensor that passes the oracle's validation"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    n, M = 17, 1 << k
    es, divs, rq, rqc = closing_inputs(E, torch, prm, n, 1700 + shared_c1, shared_c1)
    keep = rqc.clone()
    eq = [DC.divfloor((e, 0), D, k) for e, D in zip(es, divs)]
    want = torch.zeros_like(rqc)
    dq = dev(torch, DC.int_records(eq))
    E.add_plain_records(rqc.data_ptr(), dq.data_ptr(), recs["f"], want.data_ptr(), n, k, mode=0)
    out = torch.zeros_like(rqc)
    de, dd = dev(torch, DC.int_records(es)), dev(torch, DC.int_records(divs))
    E.div_close_records(de.data_ptr(), dd.data_ptr(), n, rqc.data_ptr(), recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(rqc, keep)
    assert decrypt(E, torch, prm, out, n, k) == [(a + b) % M for a, b in zip(rq, eq)]
    got = E.div_close_tensors_bytes(_pt_bytes([n], es), _pt_bytes([n], divs), E.records_to_bytes(host(rqc), [n]), recs["f"], k)
    assert got == E.records_to_bytes(host(out), [n])
    assert O.check_tensor(delta, got) == 1


def test_div_close_bytes_broadcast_shapes_and_refusals(params128):
    """a [2, 3] tensor keeps its shape under a scalar, a per-channel [3] and an element-wise [2, 3] divisor tensor; a divisor
    tensor of another shape and an [r_q] of another shape are COFHE_HIP_ESHAPE; the divisors 0, 2^(k-1) and -3 are
    COFHE_HIP_EINVAL; an output that overlaps [r_q] or the opened values, n no multiple of n_div and kbits = 640 are
    COFHE_HIP_EINVAL at the records entry point"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    n = 6
    es, divs, rq, rqc = closing_inputs(E, torch, prm, n, 66, False)
    rqb, rqb2 = E.records_to_bytes(host(rqc), [n]), E.records_to_bytes(host(rqc), [2, 3])
    eq = lambda ds: [(a + DC.divfloor((e, 0), ds[i % len(ds)], k)) % (1 << k) for i, (a, e) in enumerate(zip(rq, es))]      # noqa: E731
    for shape, ds in (([1], divs[:1]), ([3], divs[:3]), ([2, 3], divs)):
        got = E.div_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes(shape, ds), rqb2, recs["f"], k)
        shp, r2 = E.bytes_to_records(got)
        assert list(shp) == [2, 3]
        assert decrypt(E, torch, prm, dev(torch, r2), n, k) == eq(ds)
    for call in (lambda: E.div_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([2], divs[:2]), rqb2, recs["f"], k),
                 lambda: E.div_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([3, 2], divs), rqb2, recs["f"], k),
                 lambda: E.div_close_tensors_bytes(_pt_bytes([2, 3], es), _pt_bytes([1], divs[:1]), rqb, recs["f"], k)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == -2
    for bad in (0, 1 << (k - 1), -3):
        with pytest.raises(CofheHipError) as ei:
            E.div_close_tensors_bytes(_pt_bytes([n], es), _pt_bytes([n], divs[:n - 1] + [bad]), rqb, recs["f"], k)
        assert ei.value.code == EINVAL
    de, dd = dev(torch, DC.int_records(es)), dev(torch, DC.int_records(divs))
    out = torch.zeros_like(rqc)
    for call in (lambda: E.div_close_records(de.data_ptr(), dd.data_ptr(), n, rqc.data_ptr(), recs["f"], rqc.data_ptr(), n, k),
                 lambda: E.div_close_records(de.data_ptr(), dd.data_ptr(), n, rqc.data_ptr(), recs["f"], de.data_ptr(), n, k),
                 lambda: E.div_close_records(de.data_ptr(), dd.data_ptr(), 4, rqc.data_ptr(), recs["f"], out.data_ptr(), n, k),
                 lambda: E.div_close_records(de.data_ptr(), dd.data_ptr(), n, rqc.data_ptr(), recs["f"], out.data_ptr(), n, 640)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL


def protocol(E, torch, prm, xs, rs, divs):
    """[x] and the division pairs ([r], [r_q]) freshly encrypted, e = Dec([x] - [r]) opened, [y] closed and decrypted"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(len(xs) + k)
    n = len(xs)
    enc = lambda ms: fresh(E, torch, recs, ms, [rng.randrange(bound) for _ in range(n)], k)      # noqa: E731
    dd = dev(torch, DC.int_records(divs))
    q = torch.zeros(n * 32, dtype=torch.int32, device="cuda")
    E.divfloor_plain_records(dev(torch, DC.int_records(rs)).data_ptr(), dd.data_ptr(), len(divs), q.data_ptr(), n, k)
    torch.cuda.synchronize()
    rq = [int.from_bytes(row[:31].tobytes(), "little") for row in host(q).reshape(n, 32)]
    cx, cr, crq = enc(xs), enc(rs), enc(rq)
    diff = torch.zeros_like(cx)
    E.sub_ciphertext_records(cx.data_ptr(), cr.data_ptr(), diff.data_ptr(), n)
    torch.cuda.synchronize()
    es = decrypt(E, torch, prm, diff, n, k)
    assert es == [(x - r) % (1 << k) for x, r in zip(xs, rs)]
    out = torch.zeros_like(cx)
    E.div_close_records(dev(torch, DC.int_records(es)).data_ptr(), dd.data_ptr(), len(divs), crq.data_ptr(), recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    return decrypt(E, torch, prm, out, n, k)


def check_protocol(xs, ys, divs, k):
    for i, (x, y) in enumerate(zip(xs, ys)):
        c = (DC.divfloor((x, 0), divs[i % len(divs)], k) - y) % (1 << k)
        assert c in (0, 1), "element %d: x = %x, D = %x, off by %x" % (i, x, divs[i % len(divs)], c)


def test_the_whole_protocol_at_128_bits(params128):
    """17 elements of up to 64 bits and both signs, r uniform in Z/2^k drawn here (a wrap has probability below 2^-64 per
    element), a scalar, a per-channel (n_div = 17 has no proper divisor: 1 and 17) and an element-wise divisor: every element
    decrypts to floor(x / D) - c with c in {0, 1}"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    rng = random.Random(128)
    n, M = 17, 1 << k
    xs = [0, 1, M - 1, (1 << 64) - 1, M - ((1 << 64) - 1)] + [rng.choice((1, -1)) * rng.getrandbits(64) % M for _ in range(n - 5)]
    rs = [rng.getrandbits(k) for _ in range(n)]
    assert all(DC.centred(x, k) == DC.centred(r, k) + DC.centred((x - r) % M, k) for x, r in zip(xs, rs))
    for divs in ([1 << 16], [7], [rng.randrange(1, 1 << rng.choice((2, 33, 70))) for _ in range(n)]):
        check_protocol(xs, protocol(E, torch, prm, xs, rs, divs), divs, k)


def test_the_whole_protocol_at_8_bits_without_a_wrap(tiny):
    """k = 8: x over the whole range, the most negative and the most positive value included; r drawn uniformly among the
    masks with -2^(k-1) <= s(x) - s(r) < 2^(k-1), so that no element is left out; every divisor from 1 to 2^(k-1) - 1 in turn"""
    import torch
    prm = tiny
    delta, k, forms, recs, _ = setup(prm)
    assert k == 8
    E = engine(delta)
    rng = random.Random(8)
    n, M = 17, 1 << k
    xs = [0, 1, M - 1, 1 << (k - 1), (1 << (k - 1)) - 1] + [rng.getrandbits(k) for _ in range(n - 5)]
    for divs in ([1], [2], [3], [127], [rng.randrange(1, 128) for _ in range(n)]):
        rs = DC.no_wrap_masks(xs, k, rng)
        ys = protocol(E, torch, prm, xs, rs, divs)
        check_protocol(xs, ys, divs, k)
        if divs == [1]:
            assert ys == xs


def test_division_through_the_host_layer(tmp_path):
    """local_bench divide: a scalar divisor, per-channel divisors and truncate over 64 elements through the single-key and the
    2-of-3 threshold client decrypt to floor(x / D) or one less with ONE opened value per element, and the tensor it serialises
    is valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "divide", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert r.stdout.count("opened_values 64,") == 6, r.stdout
    assert "avg_pool2d: ok" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_divide.bin", "rb").read()) == 1


def test_division_timed_leg_through_the_host_layer(tmp_path):
    """local_bench divide 8 1: the timed scalar division that tools/bench_ops.py reads, at the smallest size that keeps the
    per-channel divisors and the 2 x 2 average pool (a multiple of 4)"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "divide", "8", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("divide_json: ")]
    j = json.loads(line[len("divide_json: "):])
    assert list(j) == ["E", "runs", "divide_ms", "divide_ms_min_max"]
