"""GPU: ciphertext differences, record inverses and the plaintext addend (cofhe_amd/csrc/affine.hip, the comb's kinds 3 and
4): cofhe_hip_sub_ciphertext_records, cofhe_hip_invert_records and cofhe_hip_add_plain_records against the C++/GMP oracle
byte for byte, their launch routes, round trips through decryption, the two bytes entry points and the C++ host layer."""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records, form_record, hx  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, oracle_rerand, setup

pytestmark = pytest.mark.gpu
REC = 168
WIDTHS = (2, 5, 8, 10)
NPOOL = 40


def rec_of(f):
    return form_record(f.a, f.b, f.c)


def boundary(d, k, f):
    """the principal form and f^(2^(k-1)) = (4, 4, c), which is its own inverse"""
    half_f = P.power(f, 1 << (k - 1), d)
    assert (half_f.a, half_f.b) == (4, 4)
    return P.identity(d), half_f


_pools = {}


def pool(torch, d, k, f):
    """NPOOL forms of the discriminant -- random ones, then (index NPOOL - 2, NPOOL - 1) the principal form and (4, 4, c) --
    as device records [NPOOL, 168], and the same for their inverses (inverted on the host by the model)"""
    if d not in _pools:
        rng = P.SplitMix64(515 + k)
        small = (-d).bit_length() < 256
        forms = [P.random_form(d, rng, 12, 10) if small else P.random_form(d, rng) for _ in range(NPOOL - 2)] + list(boundary(d, k, f))
        fw = dev(torch, np.concatenate([rec_of(x) for x in forms])).view(NPOOL, REC)
        inv = dev(torch, np.concatenate([rec_of(P.inverse(x)) for x in forms])).view(NPOOL, REC)
        _pools[d] = (fw, inv)
    return _pools[d]


def tensor(torch, recs, c1_idx, c2_idx):
    return torch.stack([recs[c1_idx], recs[c2_idx]], 1).reshape(-1).contiguous()


def sub_cases(torch, n, seed):
    """(name, c1 and c2 pool indices of a, of b) for the input cases of the subtraction"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda hi=NPOOL - 2: torch.randint(0, hi, (n,), device="cuda", generator=g)      # noqa: E731
    one = lambda i: torch.full((n,), i, dtype=torch.int64, device="cuda")                   # noqa: E731
    last = one(5)
    last[n - 1] = 7
    same = (rnd(), rnd())
    edge = rnd()
    edge[::2] = NPOOL - 2                     # b.c2: the principal form and (4, 4, c) in turn, a random form now and then
    edge[1::2] = NPOOL - 1
    edge[2::7] = 3
    return [("shared c1", one(5), rnd(), one(11), rnd()), ("distinct c1", rnd(), rnd(), rnd(), rnd()),
            ("one differing c1 in the last ciphertext", last, rnd(), one(11), rnd()), ("a - a", same[0], same[1], same[0], same[1]),
            ("b with boundary forms", one(5), rnd(NPOOL), one(NPOOL - 1), edge)]


def sub(E, torch, a, b, n, out=None):
    out = torch.zeros_like(a) if out is None else out
    E.sub_ciphertext_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
    torch.cuda.synchronize()
    return out


def check_sub(E, torch, d, fw, inv, n, seed):
    to_b = lambda t: E.records_to_bytes(host(t), [n])       # noqa: E731
    one_b = None
    for name, a1, a2, b1, b2 in sub_cases(torch, n, seed):
        a, b, b_inv = tensor(torch, fw, a1, a2), tensor(torch, fw, b1, b2), tensor(torch, inv, b1, b2)
        want = O.add(d, to_b(a), to_b(b_inv))
        got = sub(E, torch, a, b, n)
        assert to_b(got) == want, (n, name)
        a2_, b2_ = a.clone(), b.clone()
        assert torch.equal(sub(E, torch, a2_, b, n, out=a2_), got), (n, name, "out = a")
        assert torch.equal(sub(E, torch, a, b2_, n, out=b2_), got), (n, name, "out = b")
        if name == "a - a":
            one_b = one_b or P.serialize_ciphertext_tensor([n], [(P.identity(d), P.identity(d))] * n)
            assert want == one_b
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("n_ct", [1, 15, 16, 17, 31, 32, 300])
def test_sub_matches_the_oracle(params128, n_ct):
    """sub_ciphertext_records equals add(a, inverse of b) of the GMP oracle byte for byte on both sides of a workgroup's 32
    compositions (16 ciphertexts plain, 31 + 1 folded): shared c1, distinct c1, one differing c1 at the end, a - a (all
    principal), b with the principal form and (4, 4, c) as c2; out of place, out = a and out = b"""
    import torch
    d, k, forms, recs, _ = setup(params128)
    fw, inv = pool(torch, d, k, forms["f"])
    check_sub(engine(d), torch, d, fw, inv, n_ct, 900 + n_ct)


def test_sub_on_every_parameter_set(golden):
    """the same at n_ct = 33 for tiny_k8 and k = 256 (and k = 128)"""
    import torch
    d, k, forms, recs, _ = setup(golden[0])
    fw, inv = pool(torch, d, k, forms["f"])
    check_sub(engine(d), torch, d, fw, inv, 33, 33 + k)


def test_sub_in_the_paired_launch_window(params128):
    """n_ct = 12 289: 769 workgroups for 2 n compositions, 385 folded -- the pair of launches, one built three per CU ("k_sub_ct3")
    and one four ("k_sub_ct"); shared and distinct c1 equal compose_records over records whose second operand the host inverted"""
    import torch
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    n = 12289
    E.profile_read("k_sub_ct", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        for name, a1, a2, b1, b2 in sub_cases(torch, n, 12289)[:2]:
            a, b, b_inv = tensor(torch, fw, a1, a2), tensor(torch, fw, b1, b2), tensor(torch, inv, b1, b2)
            want = torch.empty_like(a)
            E.compose_records(a.data_ptr(), b_inv.data_ptr(), want.data_ptr(), 2 * n)
            E.profile_read("k_sub_ct", clear=True)
            got = sub(E, torch, a, b, n)
            assert torch.equal(got, want), name
            assert (E.profile_read("k_sub_ct3")[1], E.profile_read("k_sub_ct", clear=True)[1]) == (1, 1), name
    finally:
        E.set_option("profile_kernels", 0)
        E.profile_read("k_sub_ct", clear=True)


def test_invert_records(params128):
    """invert_records equals the model's inverse on 64 records, the boundary forms among them; in place too; twice is the input"""
    import torch
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    idx = torch.arange(64, device="cuda") % NPOOL
    idx[:4] = torch.tensor([NPOOL - 2, NPOOL - 1, NPOOL - 2, NPOOL - 1], device="cuda")
    x, want = fw[idx].reshape(-1).contiguous(), inv[idx].reshape(-1).contiguous()
    out = torch.zeros_like(x)
    E.invert_records(x.data_ptr(), out.data_ptr(), 64)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    E.invert_records(out.data_ptr(), out.data_ptr(), 64)
    torch.cuda.synchronize()
    assert torch.equal(out, x)
    E.invert_records(0, 0, 0)


# ---- the plaintext addend ----------------------------------------------------------------------------------------------------

def plain_values(k, n, rng):
    M = 1 << k
    vals = [0, 1, -1, M - 1, M, M + 5, -(M + 9), (M << 40) + 3]
    vals += [rng.getrandbits(k) - (M >> 1) for _ in range(max(0, n - len(vals)))]
    rng.shuffle(vals)
    return vals[:n]


def add_plain(E, torch, recs, cts, ms, k, mode, in_place=False, rs=None):
    src = cts.clone()
    out = src if in_place else torch.zeros_like(src)
    dm = dev(torch, exp_records(ms))
    dr = dev(torch, exp_records(rs)) if rs is not None else None
    E.add_plain_records(src.data_ptr(), dm.data_ptr(), recs["f"], out.data_ptr(), len(ms), k, mode,
                        d_r=dr.data_ptr() if rs is not None else None, h_record=recs["h"], pk_record=recs["pk"])
    torch.cuda.synchronize()
    if not in_place:
        assert torch.equal(src, cts)
    return out


def oracle_add_plain(E, d, k, forms, cts, cts_inv, ms, mode):
    """(c1, c2 o f^(+-m mod 2^k)), the leaf inverted for m - ct: scal_1d of (1, f) by the exponent, plus add"""
    n = len(ms)
    M = 1 << k
    to_b = lambda t: E.records_to_bytes(host(t), [n])       # noqa: E731
    es = [(-m if mode == 1 else m) % M for m in ms]
    fm = O.scal_1d(d, _pt_bytes([n], es), P.serialize_ciphertext_tensor([n], [(P.identity(d), forms["f"])] * n))
    return O.add(d, to_b(cts_inv if mode == 2 else cts), fm)


def ct_pair(torch, fw, inv, n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    i1, i2 = (torch.randint(0, NPOOL, (n,), device="cuda", generator=g) for _ in range(2))
    return tensor(torch, fw, i1, i2), tensor(torch, inv, i1, i2)


@pytest.mark.parametrize("w", WIDTHS)
def test_add_plain_matches_the_oracle(params128, w):
    """add_plain_records without randomness equals the oracle for m in {0, 1, -1, 2^k - 1, 2^k, 2^k + 5, -(2^k + 9), wider than
    k} and random values, at a pinned width, n in {1, 31, 32, 33, 300}, modes 0, 1, 2, in place and out of place; c1 is
    byte-identical to the input (its inverse in mode 2)"""
    import torch
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    rng = random.Random(17 * w)
    try:
        E.set_option("comb_width", w)
        for n in (1, 31, 32, 33, 300):
            cts, cts_inv = ct_pair(torch, fw, inv, n, 100 * w + n)
            ms = plain_values(k, n, rng)
            for mode in (0, 1, 2):
                got = add_plain(E, torch, recs, cts, ms, k, mode, in_place=(n + mode) % 2 == 1)
                assert E.records_to_bytes(host(got), [n]) == oracle_add_plain(E, d, k, forms, cts, cts_inv, ms, mode), (w, n, mode)
                c1_in = (cts_inv if mode == 2 else cts).view(n, 2, REC)[:, 0]
                assert torch.equal(got.view(n, 2, REC)[:, 0], c1_in), (w, n, mode)
    finally:
        E.set_option("comb_width", 0)


def test_add_plain_chunks_and_zero(params128):
    """"comb_chunk" pinned to 16: n = 15, 16, 17, 33 equal the unchunked call; m = 0 (mod 2^k) returns the input, inverted in mode 2"""
    import torch
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    rng = random.Random(23)
    cts, cts_inv = ct_pair(torch, fw, inv, 33, 2323)
    ms = plain_values(k, 33, rng)
    whole = {mode: add_plain(E, torch, recs, cts, ms, k, mode) for mode in (0, 1, 2)}
    assert E.records_to_bytes(host(whole[1]), [33]) == oracle_add_plain(E, d, k, forms, cts, cts_inv, ms, 1)
    try:
        E.set_option("comb_chunk", 16)
        for n in (15, 16, 17, 33):
            for mode in (0, 1, 2):
                got = add_plain(E, torch, recs, cts[: n * 2 * REC], ms[:n], k, mode, in_place=n % 2 == 0)
                assert torch.equal(got, whole[mode][: n * 2 * REC]), (n, mode)
    finally:
        E.set_option("comb_chunk", 0)
    zeros = [0, 1 << k, -(1 << k), 3 << k] * 4
    for mode in (0, 1, 2):
        got = add_plain(E, torch, recs, cts[: 16 * 2 * REC], zeros, k, mode)
        assert torch.equal(got, (cts_inv if mode == 2 else cts)[: 16 * 2 * REC]), mode


def test_add_plain_with_fresh_randomness(golden):
    """with d_r the result is the oracle's re-randomisation of the call without; r = 0 equals the call without"""
    import torch
    prm, _ = golden
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    rng = random.Random(29 + k)
    n = 33
    cts, _ = ct_pair(torch, fw, inv, n, 2929)
    ms = plain_values(k, n, rng)
    rs = [0, 1, bound - 1] + [rng.randrange(bound) for _ in range(n - 3)]
    for mode in (0, 1, 2):
        bare = add_plain(E, torch, recs, cts, ms, k, mode)
        got = add_plain(E, torch, recs, cts, ms, k, mode, in_place=mode == 1, rs=rs)
        assert E.records_to_bytes(host(got), [n]) == oracle_rerand(d, forms, E.records_to_bytes(host(bare), [n]), rs), mode
        assert torch.equal(add_plain(E, torch, recs, cts, ms, k, mode, rs=[0] * n), bare), mode


def test_add_plain_route(params128):
    """with "profile_kernels": a call without randomness runs one k_comb_first per chunk and (slots / 2 - 1).bit_length()
    k_compose_pairs levels per chunk, with slots = k // w + 2 rounded up to even -- one column per ciphertext -- and builds the
    table of f on first use only"""
    import torch
    from cofhe_amd import engine as eng_mod
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    cts, _ = ct_pair(torch, fw, inv, 100, 3131)
    ms = plain_values(k, 100, random.Random(31))
    E.profile_read("k_comb_table", clear=True)
    try:
        E.set_option("profile_kernels", 1)
        E.set_option("comb_width", 7)                   # a width no other test pins for f: the table is new
        E.set_option("comb_chunk", 40)
        w, slots, chunk = eng_mod.comb_shape(3, 100, 0, k, 7, 40)
        assert (w, slots, chunk) == (7, (k // 7 + 2 + 1) // 2 * 2, 40)
        first = add_plain(E, torch, recs, cts, ms, k, 0)
        assert E.profile_read("k_comb_table")[1] == 6
        assert E.profile_read("k_comb_first")[1] == 3
        assert E.profile_read("k_compose_pairs", clear=True)[1] == 3 * (slots // 2 - 1).bit_length()
        again = add_plain(E, torch, recs, cts, ms, k, 0)
        assert E.profile_read("k_comb_table")[1] == 0
        assert E.profile_read("k_comb_first", clear=True)[1] == 3
        assert torch.equal(first, again)
    finally:
        E.set_option("profile_kernels", 0)
        E.set_option("comb_width", 0)
        E.set_option("comb_chunk", 0)
        E.profile_read("k_comb_table", clear=True)


def test_round_trips_through_decryption(params128):
    """64 elements: a - b, ct + m, ct - m, m - ct and invert(ct) decrypt to the expected values mod 2^k"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(37)
    n, M = 64, 1 << k
    xs, ys = [rng.getrandbits(k) for _ in range(n)], [rng.getrandbits(k) for _ in range(n)]
    ms = plain_values(k, n, rng)
    a = fresh(E, torch, recs, xs, [rng.randrange(bound) for _ in range(n)], k)
    b = fresh(E, torch, recs, ys, [rng.randrange(bound) for _ in range(n)], k)
    assert decrypt(E, torch, prm, sub(E, torch, a, b, n), n, k) == [(x - y) % M for x, y in zip(xs, ys)]
    for mode, want in ((0, lambda x, m: x + m), (1, lambda x, m: x - m), (2, lambda x, m: m - x)):
        assert decrypt(E, torch, prm, add_plain(E, torch, recs, a, ms, k, mode), n, k) == [want(x, m) % M for x, m in zip(xs, ms)], mode
    rs = [rng.randrange(bound) for _ in range(n)]
    assert decrypt(E, torch, prm, add_plain(E, torch, recs, a, ms, k, 2, rs=rs), n, k) == [(m - x) % M for x, m in zip(xs, ms)]
    neg = torch.zeros_like(a)
    E.invert_records(a.data_ptr(), neg.data_ptr(), 2 * n)
    torch.cuda.synchronize()
    assert decrypt(E, torch, prm, neg, n, k) == [-x % M for x in xs]


def test_bytes_entry_points(params128):
    """sub_ciphertext_tensors and add_plaintext_tensor on serialised tensors equal the records path packed with
    records_to_bytes (2-D shape kept); a shape mismatch is COFHE_HIP_ESHAPE, a mode outside 0..2 COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    d, k, forms, recs, _ = setup(params128)
    E = engine(d)
    fw, inv = pool(torch, d, k, forms["f"])
    n, shape = 12, [3, 4]
    a, _ = ct_pair(torch, fw, inv, n, 4141)
    b, _ = ct_pair(torch, fw, inv, n, 4242)
    ms = plain_values(k, n, random.Random(41))
    ab, bb, pb = E.records_to_bytes(host(a), shape), E.records_to_bytes(host(b), shape), _pt_bytes(shape, ms)
    assert E.sub_ciphertext_tensors(ab, bb) == E.records_to_bytes(host(sub(E, torch, a, b, n)), shape)
    for mode in (0, 1, 2):
        assert E.add_plaintext_tensor(ab, pb, recs["f"], k, mode) == E.records_to_bytes(host(add_plain(E, torch, recs, a, ms, k, mode)), shape)
    for call in (lambda: E.sub_ciphertext_tensors(ab, E.records_to_bytes(host(b), [4, 3])),
                 lambda: E.sub_ciphertext_tensors(ab, E.records_to_bytes(host(b)[: 6 * 2 * REC], [6])),
                 lambda: E.add_plaintext_tensor(ab, _pt_bytes([12], ms), recs["f"], k, 0)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == -2 and "Tensor shapes must be equal" in str(ei.value)
    for call in (lambda: E.add_plaintext_tensor(ab, pb, recs["f"], k, 3), lambda: E.add_plaintext_tensor(ab, pb, recs["f"], 0, 0)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == -1


@pytest.mark.parametrize("mode,n,files", [("affine", "64", ("local_bench_affine_sub.bin", "local_bench_affine_plain.bin")),
                                          ("beaver_direct", "8", ("local_bench_beaver_direct.bin",))])
def test_cpp_host_layer(tmp_path, mode, n, files):
    """HIPCryptoSystem's sub / invert / plaintext-addend members against decryption (local_bench affine) and the Beaver
    product with direct differences (local_bench beaver_direct): both agree, and the tensors they serialise are valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, mode, n], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    for name in files:
        assert O.check_tensor(delta, open(tmp_path / name, "rb").read()) == 1
