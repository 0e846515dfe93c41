"""GPU: polynomial evaluation on ciphertext tensors from one opened value (cofhe_amd/csrc/pow_dot.hip): k_pow_dot against
the C++/GMP oracle byte for byte (a sum of the oracle's scal_1d results), its refusals, k_poly_shift against Python integers,
the closing step and its bytes entry point against the oracle and through decryption, and the protocol through the C++ host
layer."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import poly_cases as PC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records  # noqa: F401
import oracle_lib as O
from plain_mm_cases import check_output
from test_gpu_affine import NPOOL, REC, pool, tensor
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def pow_dot(E, torch, bases, exps, n):
    """bases: d device tensors of n ciphertexts; exps: d lists of n integers"""
    d = len(bases)
    db = torch.cat(bases).contiguous()
    de = dev(torch, exp_records([v for row in exps for v in row]))
    out = torch.zeros(n * 2 * REC, dtype=torch.int32, device="cuda")
    E.pow_dot_records(db.data_ptr(), de.data_ptr(), out.data_ptr(), n, d)
    torch.cuda.synchronize()
    return out


def oracle_pow_dot(E, delta, bases, exps, n):
    """add over the d results of scal_1d"""
    to_b = lambda t: E.records_to_bytes(host(t), [n])       # noqa: E731
    acc = None
    for b, row in zip(bases, exps):
        term = O.scal_1d(delta, _pt_bytes([n], row), to_b(b))
        acc = term if acc is None else O.add(delta, acc, term)
    return acc


def family_rows(d, k, n, rng, skip=()):
    """d rows of n exponents: element e takes the exponents of family e mod (number of families)"""
    fams = [f for f in PC.exponent_families(d, k, rng) if f[0] not in skip]
    cols = [fams[e % len(fams)][1] for e in range(n)]
    return [[cols[e][i] for e in range(n)] for i in range(d)]


def check_pow_dot(E, torch, delta, k, fw, n, d, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda hi=NPOOL - 2: torch.randint(0, hi, (n,), device="cuda", generator=g)      # noqa: E731
    one = lambda i: torch.full((n,), i, dtype=torch.int64, device="cuda")                   # noqa: E731
    rng = random.Random(seed)
    to_b = lambda t: E.records_to_bytes(host(t), [n])       # noqa: E731
    # every exponent family over bases with distinct c1
    bases = [tensor(torch, fw, rnd(), rnd()) for _ in range(d)]
    exps = family_rows(d, k, n, rng)
    assert to_b(pow_dot(E, torch, bases, exps, n)) == oracle_pow_dot(E, delta, bases, exps, n), (n, d, "families, distinct c1")
    # shared c1, and the principal form and (4, 4, c) among the c2 (pool indices NPOOL - 2, NPOOL - 1)
    edge = rnd(NPOOL)
    edge[::3] = NPOOL - 2
    edge[1::3] = NPOOL - 1
    bases = [tensor(torch, fw, one(5 + i), edge if i % 2 == 0 else rnd(NPOOL)) for i in range(d)]
    exps = family_rows(d, k, n, rng, skip=("lengths 3, 128 and 992 mixed",))
    assert to_b(pow_dot(E, torch, bases, exps, n)) == oracle_pow_dot(E, delta, bases, exps, n), (n, d, "shared c1, boundary forms")
    if d >= 2:              # the same base tensor given twice
        bases[1] = bases[0]
        assert to_b(pow_dot(E, torch, bases, exps, n)) == oracle_pow_dot(E, delta, bases, exps, n), (n, d, "one tensor twice")
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("d", [1, 2, 3, 8])
@pytest.mark.parametrize("n_ct", [1, 15, 16, 17, 33])
def test_pow_dot_matches_the_oracle(tiny, n_ct, d):
    """pow_dot_records equals add over scal_1d of the GMP oracle byte for byte on either side of a workgroup's 16 ciphertexts:
    every exponent family (all zero, a zero among non-zero, 1, 2^k - 1, negative, lengths 3 / 128 / 992 mixed, a shared top
    digit, equal exponents), distinct and shared c1, the principal form and (4, 4, c) among the bases, one tensor twice"""
    import torch
    delta, k, forms, recs, _ = setup(tiny)
    fw, _ = pool(torch, delta, k, forms["f"])
    check_pow_dot(engine(delta), torch, delta, k, fw, n_ct, d, 100 * n_ct + d)


@pytest.mark.parametrize("d", [2, 4])
def test_pow_dot_at_128_bits(params128, d):
    import torch
    delta, k, forms, recs, _ = setup(params128)
    fw, _ = pool(torch, delta, k, forms["f"])
    check_pow_dot(engine(delta), torch, delta, k, fw, 17, d, 1700 + d)


def test_pow_dot_with_one_base_is_pow_records(tiny):
    """d = 1 gives pow_records' bytes for every exponent family, in one launch that "profile_kernels" names k_pow_dot"""
    import torch
    delta, k, forms, recs, _ = setup(tiny)
    E = engine(delta)
    fw, _ = pool(torch, delta, k, forms["f"])
    n = 33
    g = torch.Generator(device="cuda").manual_seed(33)
    base = tensor(torch, fw, torch.randint(0, NPOOL, (n,), device="cuda", generator=g), torch.randint(0, NPOOL, (n,), device="cuda", generator=g))
    exps = family_rows(1, k, n, random.Random(33))
    want, de = torch.zeros_like(base), dev(torch, exp_records(exps[0]))
    E.pow_records(base.data_ptr(), de.data_ptr(), want.data_ptr(), n)
    torch.cuda.synchronize()
    E.profile_read("k_pow_dot", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        assert torch.equal(pow_dot(E, torch, [base], exps, n), want)
        assert E.profile_read("k_pow_dot", clear=True)[1] == 1             # one launch, under its own name
    finally:
        E.set_option("profile_kernels", 0)
        E.profile_read("k_pow_dot", clear=True)


def test_pow_dot_refusals(tiny):
    """d = 0, d = 9 and an output that overlaps the bases or the exponents: COFHE_HIP_EINVAL, and the output keeps its bytes"""
    import torch
    from cofhe_amd import CofheHipError
    delta, k, forms, recs, _ = setup(tiny)
    E = engine(delta)
    fw, _ = pool(torch, delta, k, forms["f"])
    n, d = 4, 2
    ct_words, exp_words = n * 2 * REC, n * 32
    idx = torch.arange(n, device="cuda")
    # one allocation: [bases (d tensors) | exponents (d tensors) | output]
    buf = torch.empty(d * ct_words + d * exp_words + ct_words, dtype=torch.int32, device="cuda")
    for i in range(d):
        buf[i * ct_words:(i + 1) * ct_words] = tensor(torch, fw, idx + i, idx + 7)
    buf[d * ct_words:d * ct_words + d * exp_words] = dev(torch, exp_records([3, 5, 7, 9, 2, 4, 6, 8]))
    out = buf[d * ct_words + d * exp_words:]
    out.fill_(0x5A5A5A5A)
    before = buf.clone()
    w = buf.element_size()
    p_bases, p_exps, p_out = buf.data_ptr(), buf.data_ptr() + d * ct_words * w, out.data_ptr()
    for call in (lambda: E.pow_dot_records(p_bases, p_exps, p_out, n, 0), lambda: E.pow_dot_records(p_bases, p_exps, p_out, n, 9),
                 lambda: E.pow_dot_records(p_bases, p_exps, p_bases + ct_words * w, n, d),              # the second base tensor
                 lambda: E.pow_dot_records(p_bases, p_exps, p_exps - (ct_words - 1) * w, n, d),         # one word into the exponents
                 lambda: E.pow_dot_records(p_bases, p_out - exp_words * w, p_out - w, n, 1)):           # one word of the exponents
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    E.pow_dot_records(p_bases, p_exps, p_out, n, d)                  # and the well-formed call next to them runs
    E.pow_dot_records(0, 0, 0, 0, 3)                                 # nothing to do
    torch.cuda.synchronize()
    assert torch.equal(buf[:d * ct_words + d * exp_words], before[:d * ct_words + d * exp_words]) and not torch.equal(out, before[-ct_words:])


@pytest.mark.parametrize("k", [8, 128, 256, 300])
def test_poly_shift_on_the_device(tiny, k):
    """poly_shift_records at 33 elements, degree 3 (k = 300: the runtime limb count, whose working array is the output) and the
    copy of degree 0, against Python integers; every word of the output is written; k = 0 and k = 641 are refused"""
    import torch
    from cofhe_amd import CofheHipError
    E = engine(setup(tiny)[0])
    rng = random.Random(300 + k)
    n = 33
    xs = PC.shift_points(k, n - 2, rng) + [-rng.getrandbits(k), (1 << k) + 3]
    for coef in ([rng.getrandbits(k), -rng.getrandbits(k + 9), (1 << k) - 1, rng.getrandbits(k)], [-5]):
        d = len(coef) - 1
        q = torch.full(((d + 1) * n * 32,), 0xA5A5A5A5 - (1 << 32), dtype=torch.int32, device="cuda")
        dc, dx = dev(torch, exp_records(coef)), dev(torch, exp_records(xs))
        E.poly_shift_records(dc.data_ptr(), dx.data_ptr(), q.data_ptr(), n, d, k)
        torch.cuda.synchronize()
        per = [PC.taylor_shift(coef, x, k) for x in xs]
        check_output(host(q), [per[e][i] for i in range(d + 1) for e in range(n)], k)
    for bad in (0, 641):
        with pytest.raises(CofheHipError) as ei:
            E.poly_shift_records(q.data_ptr(), q.data_ptr(), q.data_ptr(), 1, 0, bad)
        assert ei.value.code == EINVAL


def closing_inputs(E, torch, prm, coef, n, seed):
    """x, the power tuples as d freshly encrypted tensors, the opened values x - a"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    M, d = 1 << k, len(coef) - 1
    xs = PC.shift_points(k, n, rng)
    a = [rng.getrandbits(k) for _ in range(n)]
    powers = [fresh(E, torch, recs, [pow(v, i, M) for v in a], [rng.randrange(bound) for _ in range(n)], k) for i in range(1, d + 1)]
    return xs, powers, [(x - v) % M for x, v in zip(xs, a)]


@pytest.mark.parametrize("coef", [(0, 0, 1), (7, -3, 11), (5, -3, 7, 11)], ids=["square", "degree2", "degree3"])
def test_poly_close_matches_the_oracle_and_decrypts(params128, coef):
    """poly_close_records at 17 elements equals the oracle's sum of scal_1d(q_i, [a^i]) plus f^(q_0) byte for byte, decrypts to
    p(x) mod 2^k for x in {0, 1, 2^k - 1, 2^(k-1), random}, and poly_close_tensors returns the same tensor serialised"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    n, d, M = 17, len(coef) - 1, 1 << k
    coef = [c % M for c in coef]
    xs, powers, es = closing_inputs(E, torch, prm, coef, n, 17 * d + coef[0])
    dp = torch.cat(powers).contiguous()
    out = torch.zeros(n * 2 * REC, dtype=torch.int32, device="cuda")
    dc, de = dev(torch, exp_records(coef)), dev(torch, exp_records(es))
    E.poly_close_records(dc.data_ptr(), de.data_ptr(), dp.data_ptr(), recs["f"], out.data_ptr(), n, d, k)
    torch.cuda.synchronize()
    q = [PC.taylor_shift(coef, e, k) for e in es]
    want = oracle_pow_dot(E, delta, powers, [[q[e][i] for e in range(n)] for i in range(1, d + 1)], n)
    fq0 = O.scal_1d(delta, _pt_bytes([n], [q[e][0] for e in range(n)]), P.serialize_ciphertext_tensor([n], [(P.identity(delta), forms["f"])] * n))
    want = O.add(delta, want, fq0)
    got = E.records_to_bytes(host(out), [n])
    assert got == want
    assert decrypt(E, torch, prm, out, n, k) == [PC.poly(coef, x, k) for x in xs]
    assert E.poly_close_tensors(_pt_bytes([d + 1], coef), _pt_bytes([n], es), E.records_to_bytes(host(dp), [d, n]), recs["f"], k) == got


def test_poly_close_bytes_shapes_and_refusals(params128):
    """a 2-D tensor keeps its shape; powers of another shape are COFHE_HIP_ESHAPE; an output that overlaps the powers, d = 0 and
    d = 9 are COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    coef, n = [1, 2, 3], 6
    xs, powers, es = closing_inputs(E, torch, prm, coef, n, 66)
    dp = torch.cat(powers).contiguous()
    cb, pb = _pt_bytes([3], coef), E.records_to_bytes(host(dp), [2, 2, 3])
    flat = E.poly_close_tensors(cb, _pt_bytes([n], es), E.records_to_bytes(host(dp), [2, n]), recs["f"], k)
    _, r2 = E.bytes_to_records(E.poly_close_tensors(cb, _pt_bytes([2, 3], es), pb, recs["f"], k))
    assert E.records_to_bytes(r2, [n]) == flat
    for call in (lambda: E.poly_close_tensors(cb, _pt_bytes([3, 2], es), pb, recs["f"], k),
                 lambda: E.poly_close_tensors(_pt_bytes([4], coef + [1]), _pt_bytes([2, 3], es), pb, recs["f"], k)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == -2
    de, dc = dev(torch, exp_records(es)), dev(torch, exp_records(coef))
    for call in (lambda: E.poly_close_records(dc.data_ptr(), de.data_ptr(), dp.data_ptr(), recs["f"], dp.data_ptr(), n, 2, k),
                 lambda: E.poly_close_records(dc.data_ptr(), de.data_ptr(), dp.data_ptr(), recs["f"], de.data_ptr(), n, 0, k),
                 lambda: E.poly_close_records(dc.data_ptr(), de.data_ptr(), dp.data_ptr(), recs["f"], de.data_ptr(), n, 9, k)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL


def test_polynomial_activation_through_the_host_layer(tmp_path):
    """local_bench poly_activation: degree 3 over 64 elements through the single-key and the 2-of-3 threshold client decrypts
    to p(x) mod 2^k with ONE opened value per element, and the tensor it serialises is valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "poly_activation", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert r.stdout.count("decrypted_elements 64,") == 2, r.stdout
    assert "pow_dot_ciphertext_tensors: ok" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_poly_activation.bin", "rb").read()) == 1


def test_polynomial_activation_timed_leg_through_the_host_layer(tmp_path):
    """local_bench poly_activation 8 1: the timed comparison that tools/bench_ops.py reads, at the smallest size that still has
    all eight special inputs: x^3 by the polynomial opens one value per element, by two chained products four"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "poly_activation", "8", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("compare_json: ")]
    j = json.loads(line[len("compare_json: "):])
    assert list(j) == ["E", "degree", "runs", "poly_ms", "poly_ms_min_max", "chained_products_ms", "chained_ms_min_max",
                       "chained_over_poly", "opened_poly", "opened_chained", "agree"]
    assert j["E"] == 8 and j["opened_poly"] == 8 and j["opened_chained"] == 32 and j["agree"] is True
