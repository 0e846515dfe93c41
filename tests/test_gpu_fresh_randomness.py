"""GPU: fresh randomness per ciphertext through the fixed-base comb (cofhe_amd/csrc/comb.hpp, comb.hip):
cofhe_hip_pow_fixed_base_many_records against the k_pow ladder, cofhe_hip_encrypt_fresh_records and
cofhe_hip_rerandomize_records against the C++/GMP oracle, round trips through decryption, chunk boundaries and the
launch route."""
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records, form_record, hx  # noqa: F401
import oracle_lib as O

pytestmark = pytest.mark.gpu
REC = 168
WIDTHS = (2, 5, 8, 10)


def setup(prm):
    d, k = hx(prm["delta"]), prm["k"]
    F = lambda o: P.Form(hx(o["a"]), hx(o["b"]), hx(o["c"]))       # noqa: E731
    forms = {n: F(prm[n]) for n in ("h", "pk", "f")}
    recs = {n: form_record(f.a, f.b, f.c) for n, f in forms.items()}
    return d, k, forms, recs, hx(prm["exponent_bound"])


def dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


def ladder(E, torch, base_rec, exps):
    """base^e[i] by the k_pow ladder (cofhe_hip_pow_form_records) over n copies of the base"""
    n = len(exps)
    b = dev(torch, np.tile(base_rec, n))
    out = torch.empty_like(b)
    E.pow_form_records(b.data_ptr(), dev(torch, exp_records(exps)).data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    return host(out).reshape(n, REC)


def comb_many(E, torch, base_rec, exps):
    n = len(exps)
    out = torch.zeros(n * REC, dtype=torch.int32, device="cuda")
    de = dev(torch, exp_records(exps))
    E.pow_fixed_base_many_records(base_rec, de.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    return host(out).reshape(n, REC)


def fresh(E, torch, recs, ms, rs, k):
    n = len(ms)
    out = torch.zeros(n * 2 * REC, dtype=torch.int32, device="cuda")
    dm, dr = dev(torch, exp_records(ms)), dev(torch, exp_records(rs))
    E.encrypt_fresh_records(dm.data_ptr(), dr.data_ptr(), recs["h"], recs["pk"], recs["f"], out.data_ptr(), n, k)
    torch.cuda.synchronize()
    return out


def rerand(E, torch, recs, cts, rs, in_place=False):
    n = len(rs)
    src = cts.clone()
    out = src if in_place else torch.zeros_like(src)
    dr = dev(torch, exp_records(rs))
    E.rerandomize_records(src.data_ptr(), dr.data_ptr(), recs["h"], recs["pk"], out.data_ptr(), n)
    torch.cuda.synchronize()
    return out


def oracle_fresh(d, k, forms, ms, rs):
    """(h^r, pk^r o f^(m mod 2^k)) by the GMP oracle: scal_1d of (h, pk) by r, plus scal_1d of (1, f) by m mod 2^k"""
    n = len(ms)
    hr = O.scal_1d(d, _pt_bytes([n], rs), P.serialize_ciphertext_tensor([n], [(forms["h"], forms["pk"])] * n))
    fm = O.scal_1d(d, _pt_bytes([n], [m % (1 << k) for m in ms]), P.serialize_ciphertext_tensor([n], [(P.identity(d), forms["f"])] * n))
    return O.add(d, hr, fm)


def oracle_rerand(d, forms, cts_bytes, rs):
    n = len(rs)
    hr = O.scal_1d(d, _pt_bytes([n], rs), P.serialize_ciphertext_tensor([n], [(forms["h"], forms["pk"])] * n))
    return O.add(d, cts_bytes, hr)


def decrypt(E, torch, prm, cts, n, k):
    frec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    ow = (k + 31) // 32 + 1
    out = torch.zeros(n * ow, dtype=torch.int32, device="cuda")
    dsk = dev(torch, exp_records([hx(prm["sk"])]))
    E.decrypt_records(cts.data_ptr(), dsk.data_ptr(), frec, out.data_ptr(), n, k)
    torch.cuda.synchronize()
    o = host(out).reshape(n, ow)
    assert not o[:, -1].any()
    return [int.from_bytes(r[:-1].tobytes(), "little") for r in o]


def edge_exponents(bound, rng):
    vals = [0, 1, -1, (1 << 992) - 1, -((1 << 991) + 1), bound - 1, 2, -2]
    for t in (7, 8, 9, 15, 16, 17, 479, 480, 481, 959, 960, 961, 989, 990, 991):
        vals += [1 << t, (1 << t) - 1]
    return vals + [rng.randrange(bound) * (1 if i % 5 else -1) for i in range(300 - len(vals))]


def test_many_powers_match_the_ladder(golden):
    """pow_fixed_base_many_records equals the k_pow ladder byte for byte for the edge exponents, at every pinned width,
    n in {1, 31, 32, 33, 300}, five bases (h, pk, f, two ciphertext components): more (base, w) pairs than the context
    keeps tables, more bases than it keeps chains"""
    import torch
    prm, _ = golden
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(k)
    exps = edge_exponents(bound, rng)
    ct = P.random_form(d, P.SplitMix64(k + 1)), P.random_form(d, P.SplitMix64(k + 2))
    bases = [recs["h"], recs["pk"], recs["f"]] + [form_record(f.a, f.b, f.c) for f in ct]
    try:
        for b in bases:
            want = ladder(E, torch, b, exps)
            for w in WIDTHS:
                E.set_option("comb_width", w)
                for n in (1, 31, 32, 33, 300):
                    got = comb_many(E, torch, b, exps[:n] if n < 300 else exps)
                    assert np.array_equal(got, want[:n]), (w, n)
        # a second pass hits the tables that survived and rebuilds the evicted ones
        E.set_option("comb_width", 8)
        assert np.array_equal(comb_many(E, torch, bases[0], exps[:40]), ladder(E, torch, bases[0], exps[:40]))
    finally:
        E.set_option("comb_width", 0)


def test_fresh_encryption_matches_the_oracle(golden):
    """encrypt_fresh_records equals the GMP oracle for 64 elements with m in {0, 2^k - 1, -1, wider than k} and r in {0, 1,
    bound - 1}; with one r for all elements it equals the shared-r encrypt_records byte for byte"""
    import torch
    prm, _ = golden
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(3 * k)
    M = 1 << k
    ms = [0, M - 1, -1, M + 5, (M << 40) + 3, -(M + 9), 1, 2] + [rng.getrandbits(k) - (M >> 1) for _ in range(56)]
    rs = [0, 1, bound - 1, 2] + [rng.randrange(bound) for _ in range(60)]
    got = fresh(E, torch, recs, ms, rs, k)
    assert E.records_to_bytes(host(got), [64]) == oracle_fresh(d, k, forms, ms, rs)
    # shared r: the existing route
    r = rng.randrange(bound)
    hp = torch.zeros(2 * REC, dtype=torch.int32, device="cuda")
    base = dev(torch, np.concatenate([recs["h"], recs["pk"]]))
    E.pow_form_records(base.data_ptr(), dev(torch, exp_records([r, r])).data_ptr(), hp.data_ptr(), 2)
    shared = torch.zeros(64 * 2 * REC, dtype=torch.int32, device="cuda")
    E.encrypt_records(dev(torch, exp_records(ms)).data_ptr(), hp.data_ptr(), recs["f"], shared.data_ptr(), 64, k)
    torch.cuda.synchronize()
    assert torch.equal(fresh(E, torch, recs, ms, [r] * 64, k), shared)


def test_rerandomize_matches_the_oracle(golden):
    """rerandomize_records equals the oracle in place and out of place; r = 0 is the identity; decryption is unchanged"""
    import torch
    prm, _ = golden
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(5 * k)
    n = 64
    ms = [rng.getrandbits(k) for _ in range(n)]
    cts = fresh(E, torch, recs, ms, [rng.randrange(bound) for _ in range(n)], k)
    rs = [0, 1, bound - 1] + [rng.randrange(bound) for _ in range(n - 3)]
    want = oracle_rerand(d, forms, E.records_to_bytes(host(cts), [n]), rs)
    out = rerand(E, torch, recs, cts, rs)
    assert E.records_to_bytes(host(out), [n]) == want
    inp = rerand(E, torch, recs, cts, rs, in_place=True)
    assert torch.equal(inp, out)
    assert torch.equal(rerand(E, torch, recs, cts, [0] * n), cts)
    assert decrypt(E, torch, prm, out, n, k) == decrypt(E, torch, prm, cts, n, k) == ms


def test_round_trip_and_distinct_c1(params128):
    """1024 fresh encryptions decrypt to m mod 2^k, and no two share a c1"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(11)
    n = 1024
    ms = [rng.getrandbits(k + 8) - (1 << (k + 7)) for _ in range(n)]
    cts = fresh(E, torch, recs, ms, [rng.randrange(bound) for _ in range(n)], k)
    c1 = host(cts).reshape(n, 2, REC)[:, 0, :]
    assert len({hashlib.sha256(r.tobytes()).digest() for r in c1}) == n
    assert decrypt(E, torch, prm, cts, n, k) == [m % (1 << k) for m in ms]


def test_chunk_boundaries_match_the_ladder(params128):
    """"comb_chunk" pinned small: n = chunk - 1, chunk, chunk + 1, 2 chunk + 1 equal the ladder route for fresh encryption
    (h^r, pk^r o f^m by k_pow and compose), re-randomisation and plain powers"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(13)
    chunk = 16
    n_max = 2 * chunk + 1
    ms = [rng.getrandbits(k) for _ in range(n_max)]
    rs = [rng.randrange(bound) for _ in range(n_max)]
    hr, pkr, fm = ladder(E, torch, recs["h"], rs), ladder(E, torch, recs["pk"], rs), ladder(E, torch, recs["f"], ms)
    a, b = dev(torch, pkr), dev(torch, fm)
    c2 = torch.empty_like(a)
    E.compose_records(a.data_ptr(), b.data_ptr(), c2.data_ptr(), n_max)
    torch.cuda.synchronize()
    want = np.stack([hr, host(c2).reshape(n_max, REC)], axis=1).reshape(-1)
    # re-randomising those ciphertexts with fresh r': ct o (h^r', pk^r') by the ladder and compose
    rs2 = [rng.randrange(bound) for _ in range(n_max)]
    hr2 = np.stack([ladder(E, torch, recs["h"], rs2), ladder(E, torch, recs["pk"], rs2)], axis=1).reshape(-1)
    a, b = dev(torch, want), dev(torch, hr2)
    rr_want = torch.empty_like(a)
    E.compose_records(a.data_ptr(), b.data_ptr(), rr_want.data_ptr(), 2 * n_max)
    torch.cuda.synchronize()
    rr_want = host(rr_want)
    try:
        E.set_option("comb_chunk", chunk)
        for n in (chunk - 1, chunk, chunk + 1, n_max):
            got = fresh(E, torch, recs, ms[:n], rs[:n], k)
            assert np.array_equal(host(got), want[: n * 2 * REC]), n
            assert np.array_equal(comb_many(E, torch, recs["h"], rs[:n]), hr[:n]), n
            rr = rerand(E, torch, recs, got, rs2[:n], in_place=(n % 2 == 1))
            assert np.array_equal(host(rr), rr_want[: n * 2 * REC]), n
    finally:
        E.set_option("comb_chunk", 0)


def test_route_builds_a_table_once(params128):
    """with "profile_kernels" on: a new base builds its table in w - 1 k_comb_table launches on first use only, and each
    chunk runs k_comb_first once"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(17)
    f = P.random_form(d, P.SplitMix64(99))
    base = form_record(f.a, f.b, f.c)
    rs = [rng.randrange(bound) for _ in range(100)]
    E.profile_read("k_comb_table", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        E.set_option("comb_width", 6)
        E.set_option("comb_chunk", 40)
        first = comb_many(E, torch, base, rs)
        assert E.profile_read("k_comb_table")[1] == 5
        assert E.profile_read("k_comb_first")[1] == 3
        levels = E.profile_read("k_compose_pairs", clear=True)[1]
        assert levels == 3 * ((966 // 6 + 2) // 2 - 1).bit_length()
        again = comb_many(E, torch, base, rs)
        assert E.profile_read("k_comb_table")[1] == 0
        assert E.profile_read("k_comb_first", clear=True)[1] == 3
        assert np.array_equal(first, again)
        assert np.array_equal(first, ladder(E, torch, base, rs))
    finally:
        E.set_option("profile_kernels", 0)
        E.set_option("comb_width", 0)
        E.set_option("comb_chunk", 0)
        E.profile_read("k_comb_table", clear=True)


def test_zero_count_and_bad_arguments(params128):
    """n = 0 is a no-op; widths outside 2..10 and a k out of range are refused"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    E.encrypt_fresh_records(0, 0, recs["h"], recs["pk"], recs["f"], 0, 0, k)
    E.pow_fixed_base_many_records(recs["h"], 0, 0, 0)
    for bad in (1, 11):
        with pytest.raises(CofheHipError):
            E.set_option("comb_width", bad)
    out = torch.zeros(2 * REC, dtype=torch.int32, device="cuda")
    de = dev(torch, exp_records([1]))
    with pytest.raises(CofheHipError):
        E.encrypt_fresh_records(de.data_ptr(), de.data_ptr(), recs["h"], recs["pk"], recs["f"], out.data_ptr(), 1, 0)


def test_cpp_per_element_mode(tmp_path):
    """HIPCryptoSystem in TensorRandomness::PerElement mode (local_bench fresh_randomness): encrypt_tensor, add, 1-D scal,
    negate and rerandomize_ciphertext_tensor give every ciphertext its own c1 and decrypt as before, while the default mode
    still shares one r per tensor; the serialised tensors are valid for the oracle"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "fresh_randomness", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    for name in ("local_bench_fresh_ct.bin", "local_bench_fresh_rerand.bin"):
        t = open(tmp_path / name, "rb").read()
        assert O.check_tensor(delta, t) == 1
        shape, cts = P.deserialize_ciphertext_tensor(t)
        assert shape == [64] and len({(c1.a, c1.b) for c1, _ in cts}) == 64
