"""GPU: table lookups on ciphertext tensors from one opened value (cofhe_amd/csrc/lut.hip): k_lut_rotate and k_lut_select
against Python integers, the tuples entry point against the fresh encryption byte for byte, the whole protocol at the ABI
through decryption, the bytes entry point, the refusals, and the protocol through the C++ host layer."""
import json
import os
import random
import subprocess

import numpy as np
import pytest

import lut_cases as LC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL, ESHAPE = -1, -2
REC = 168
CT = 2 * REC                                 # words of a ciphertext
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def filled(torch, words):
    return torch.full((words,), FILL - (1 << 32), dtype=torch.int32, device="cuda")


def random_tuples(torch, n_ct, seed):
    """n_ct ciphertext records of random words, none of them the fill word: the closing step moves bytes and composes nothing"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    t = torch.randint(-(1 << 31), (1 << 31) - 1, (n_ct * CT,), dtype=torch.int32, device="cuda", generator=g)
    t[t == FILL - (1 << 32)] = 0
    return t


def rotate(E, torch, tab, n_tab, rs, b, shift=0):
    """the rotated rows' records; shift: every pointer that many words beyond a 16-byte boundary"""
    n = len(rs)
    dt, dr = dev(torch, np.concatenate([np.zeros(shift, np.uint32), LC.records(tab)])), dev(torch, np.concatenate([np.zeros(shift, np.uint32), LC.records(rs)]))
    out = filled(torch, (n << b) * 32 + shift)
    E.lut_rotate_records(dt.data_ptr() + 4 * shift, n_tab, dr.data_ptr() + 4 * shift, out.data_ptr() + 4 * shift, n, b)
    torch.cuda.synchronize()
    return host(out)[shift:]


def select(E, torch, es, tuples, b, shift=0):
    """the selected ciphertexts' records; tuples: a device tensor that starts `shift` words beyond a 16-byte boundary"""
    n = len(es)
    de = dev(torch, np.concatenate([np.zeros(shift, np.uint32), LC.records(es)]))
    out = filled(torch, n * CT + shift)
    E.lut_select_records(de.data_ptr() + 4 * shift, tuples.data_ptr(), out.data_ptr() + 4 * shift, n, b)
    torch.cuda.synchronize()
    return host(out)[shift:]


@pytest.mark.parametrize("n,b", [(n, b) for b in LC.BITS_GPU for n in LC.SIZES_GPU] + [(2, 12)])
def test_rotate_and_select_match_python_integers(tiny, n, b):
    """rotate word for word with one table, three (where 3 divides n) and one per element; select byte for byte against the
    tuple buffer with every output word pre-filled and written; masks and opened values from every family of lut_cases; one
    launch per call, under the kernels' own profile names"""
    import torch
    E = engine(setup(tiny)[0])
    rng = random.Random(100 * n + b)
    rs, es = LC.values(b, 128, n, rng), LC.values(b, 128, n, rng)
    for name in ("k_lut_rotate", "k_lut_select"):
        E.profile_read(name, clear=True)
    try:
        E.set_option("profile_kernels", 1)
        launches = 0
        for n_tab in sorted({1, 3, n}):
            if n % n_tab:
                continue
            tab = LC.table(b, n_tab, rng)
            got = rotate(E, torch, tab, n_tab, rs, b)
            assert np.array_equal(got, LC.records(LC.rotate(tab, n_tab, rs, b))), n_tab
            launches += 1
        tuples = random_tuples(torch, n << b, n + b)
        got = select(E, torch, es, tuples, b).reshape(n, CT)
        want = host(tuples).reshape(n << b, CT)[LC.selected(es, b)]
        assert np.array_equal(got, want)
        assert launches >= 1
        assert E.profile_read("k_lut_rotate")[1] == launches               # clear=True drops the spans of every name
        assert E.profile_read("k_lut_select", clear=True)[1] == 1
    finally:
        E.set_option("profile_kernels", 0)
        for name in ("k_lut_rotate", "k_lut_select"):
            E.profile_read(name, clear=True)


def test_pointers_with_only_4_byte_alignment_give_the_same_bytes(tiny):
    """every pointer one word beyond a 16-byte boundary (the dword path of both kernels) against the aligned call, n = 9, b = 3,
    three tables; nothing before the shifted output is touched"""
    import torch
    E = engine(setup(tiny)[0])
    rng = random.Random(49)
    n, b, n_tab = 9, 3, 3
    rs, es, tab = LC.values(b, 128, n, rng), LC.values(b, 128, n, rng), LC.table(b, n_tab, rng)
    want = rotate(E, torch, tab, n_tab, rs, b)
    assert np.array_equal(want, LC.records(LC.rotate(tab, n_tab, rs, b)))
    assert np.array_equal(rotate(E, torch, tab, n_tab, rs, b, shift=1), want)
    tuples = random_tuples(torch, (n << b) + 1, 7)
    aligned = tuples[CT:].clone()                                   # a fresh allocation: 16-byte aligned
    assert aligned.data_ptr() % 16 == 0 and tuples[1:].data_ptr() % 16 == 4
    shifted = tuples[1:1 + (n << b) * CT]
    want = select(E, torch, es, aligned, b)
    assert np.array_equal(want.reshape(n, CT), host(aligned).reshape(n << b, CT)[LC.selected(es, b)])
    aligned[:] = shifted
    assert np.array_equal(select(E, torch, es, shifted, b, shift=1), select(E, torch, es, aligned, b))


def test_tuples_are_the_fresh_encryption_of_the_rotated_rows(params128):
    """lut_tuples_records at n = 5, b = 3 equals encrypt_fresh_records over the output of lut_rotate_records byte for byte, and
    the c1 of its 40 ciphertexts are pairwise distinct"""
    import torch
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    rng = random.Random(53)
    n, b = 5, 3
    tab = [(rng.getrandbits(k), 0) for _ in range(1 << b)]
    rs = LC.values(b, k, n, rng)
    rho = [rng.randrange(bound) for _ in range(n << b)]
    dt, dr, drho = dev(torch, LC.records(tab)), dev(torch, LC.records(rs)), dev(torch, exp_records(rho))
    rows = torch.zeros((n << b) * 32, dtype=torch.int32, device="cuda")
    E.lut_rotate_records(dt.data_ptr(), 1, dr.data_ptr(), rows.data_ptr(), n, b)
    want = torch.zeros((n << b) * CT, dtype=torch.int32, device="cuda")
    E.encrypt_fresh_records(rows.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], want.data_ptr(), n << b, k)
    got = filled(torch, (n << b) * CT)
    E.lut_tuples_records(dt.data_ptr(), 1, dr.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], got.data_ptr(), n, b, k)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    c1 = host(got).reshape(n << b, 2, REC)[:, 0]
    assert len({r.tobytes() for r in c1}) == n << b


def protocol(E, torch, prm, xs, tab, b, seed):
    """fresh [x] and [r], the tuples of the table `tab` (2^b plaintexts), e = Dec([x] - [r]) opened, the entries selected and
    decrypted; returns (opened values, tuple buffer, selected ciphertexts, their plaintexts)"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    n, M = len(xs), 1 << k
    rand = lambda m: [rng.randrange(bound) for _ in range(m)]       # noqa: E731
    rs = [rng.getrandbits(k) for _ in range(n)]
    cx, cr = fresh(E, torch, recs, xs, rand(n), k), fresh(E, torch, recs, rs, rand(n), k)
    dt, dr, drho = dev(torch, exp_records(tab)), dev(torch, exp_records(rs)), dev(torch, exp_records(rand(n << b)))
    tuples = torch.zeros((n << b) * CT, dtype=torch.int32, device="cuda")
    E.lut_tuples_records(dt.data_ptr(), 1, dr.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], tuples.data_ptr(), n, b, k)
    diff = torch.zeros_like(cx)
    E.sub_ciphertext_records(cx.data_ptr(), cr.data_ptr(), diff.data_ptr(), n)
    torch.cuda.synchronize()
    es = decrypt(E, torch, prm, diff, n, k)
    assert es == [(x - r) % M for x, r in zip(xs, rs)]
    out = filled(torch, n * CT)
    E.lut_select_records(dev(torch, exp_records(es)).data_ptr(), tuples.data_ptr(), out.data_ptr(), n, b)
    torch.cuda.synchronize()
    return es, tuples, out, decrypt(E, torch, prm, out, n, k)


@pytest.mark.parametrize("b", [3, 8])
def test_the_whole_protocol_at_8_bits(tiny, b):
    """k = 8, b = 3 and b = 8 = k: x over the whole range of Z/2^k, both signs, and (b = 3) far outside the b-bit range, where
    it wraps; the table a permutation of distinct values, so a wrong index cannot pass, and then the ReLU of a b-bit signed
    value; every element decrypts to exactly table[x mod 2^b]"""
    import torch
    prm = tiny
    delta, k, forms, recs, _ = setup(prm)
    assert k == 8
    E = engine(delta)
    rng = random.Random(80 + b)
    xs = list(range(1 << k))
    rng.shuffle(xs)
    perm = rng.sample(range(1 << k), 1 << b)
    for tab in (perm, LC.relu_table(b)):
        ys = protocol(E, torch, prm, xs, tab, b, 800 + b)[3]
        assert ys == [tab[x % (1 << b)] for x in xs]
    assert [max(LC.signed(x, b), 0) for x in xs] == [LC.relu_table(b)[x % (1 << b)] for x in xs]


def test_the_whole_protocol_at_128_bits_and_the_bytes_entry_point(params128):
    """n = 17, b = 4: x of both signs inside the 4-bit signed range, and outside it (64-bit and k-bit values of both signs),
    where it wraps as x mod 2^b; table entries up to 2^k - 1; every element decrypts to exactly table[x mod 2^b];
    lut_select_tensors_bytes returns the same tensor serialised, for a [17] and a [17, 1] tensor, and the oracle accepts it; a
    tuple tensor of another shape is COFHE_HIP_ESHAPE"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    rng = random.Random(128)
    n, b, M = 17, 4, 1 << k
    xs = [0, 1, 7, M - 1, M - 8, 8, M - 9, (1 << 64) - 1, M - (1 << 64) + 3, M >> 1] + [rng.getrandbits(k) for _ in range(n - 10)]
    tab = [M - 1, 0, 1] + [rng.getrandbits(k) for _ in range(13)]
    assert len(set(tab)) == 16
    es, tuples, out, ys = protocol(E, torch, prm, xs, tab, b, 1280)
    assert ys == [tab[x % 16] for x in xs]
    assert np.array_equal(host(out).reshape(n, CT), host(tuples).reshape(n << b, CT)[LC.selected([(e, 0) for e in es], b)])
    want = E.records_to_bytes(host(out), [n])
    got = E.lut_select_tensors_bytes(_pt_bytes([n], es), E.records_to_bytes(host(tuples), [n, 16]))
    assert got == want
    assert O.check_tensor(delta, got) == 1
    got2 = E.lut_select_tensors_bytes(_pt_bytes([n, 1], es), E.records_to_bytes(host(tuples), [n, 1, 16]))
    assert got2 == E.records_to_bytes(host(out), [n, 1])
    tb = host(tuples)
    for eb, tbytes in ((_pt_bytes([n], es), E.records_to_bytes(tb, [n * 16])),                       # no entry dimension
                       (_pt_bytes([n], es), E.records_to_bytes(tb, [16, n])),                        # transposed
                       (_pt_bytes([n], es), E.records_to_bytes(tb[:n * 12 * CT], [n, 12])),          # 12 is no power of two
                       (_pt_bytes([n], es), E.records_to_bytes(tb[:n * CT], [n, 1])),                # bits = 0
                       (_pt_bytes([n - 1], es[:-1]), E.records_to_bytes(tb, [n, 16])),
                       (_pt_bytes([n, 1], es), E.records_to_bytes(tb, [n, 16]))):
        with pytest.raises(CofheHipError) as ei:
            E.lut_select_tensors_bytes(eb, tbytes)
        assert ei.value.code == ESHAPE


def test_the_bytes_entry_point_refuses_a_forged_tuple():
    """lut_select_tensors_bytes is composed from unpack_tensor_device, so it stands behind the form gate like the library's own
    *_tensors_bytes entry points: one equation forgery (c + 1) and one non-primitive forgery as c1 of the first entry and as c2
    of the last of a [2, 2] tuple tensor are refused, and the same call with valid forms goes through"""
    import form_gate_cases as G
    from cofhe_amd import CofheHipError
    d = G.discriminants()[1]
    E = engine(d.delta)
    ok = [G.as_form(cs.rec) for cs in G.passes(d)]
    by = {cs.label: cs.rec for cs in d.cases}
    e = _pt_bytes([2], [7, 9])

    def tuples(forged=None, at=None):
        cts = [(ok[2 * i % len(ok)], ok[(2 * i + 1) % len(ok)]) for i in range(4)]
        if at == "first_c1":
            cts[0] = (forged, cts[0][1])
        if at == "last_c2":
            cts[-1] = (cts[-1][0], forged)
        return cts, P.serialize_ciphertext_tensor([2, 2], cts)

    cts, valid = tuples()
    assert E.lut_select_tensors_bytes(e, valid) == P.serialize_ciphertext_tensor([2], [cts[1], cts[3]])      # 7 and 9 are odd
    for label in ("c_plus_1", "content2_random"):
        for at in ("first_c1", "last_c2"):
            with pytest.raises(CofheHipError, match="not a reduced form"):
                E.lut_select_tensors_bytes(e, tuples(G.as_form(by[label]), at)[1])
    assert E.device_status(clear=False) == 0


def test_refusals_leave_the_buffers_unchanged(params128):
    """bits = 0 and 13, n_tab = 0, n no multiple of n_tab and an output that overlaps an input, at each of the three records
    entry points; bits > k at the tuples: COFHE_HIP_EINVAL, nothing written, the status word clear; n = 0 does nothing;
    bits = 12 runs"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    rng = random.Random(9)
    n, b, w = 4, 2, 4
    size = 1 << b
    # exponent records: [table (2 tables) | r | e | rho | rows]
    o_tab, o_r, o_e, o_rho, o_rows = 0, 2 * size * 32, (2 * size + n) * 32, (2 * size + 2 * n) * 32, (2 * size + 2 * n + n * size) * 32
    ex = filled(torch, o_rows + n * size * 32)
    ex[:o_r] = dev(torch, LC.records(LC.table(b, 2, rng)))
    ex[o_r:o_e] = dev(torch, LC.records(LC.values(b, k, n, rng)))
    ex[o_e:o_rho] = dev(torch, LC.records(LC.values(b, k, n, rng)))
    ex[o_rho:o_rows] = dev(torch, exp_records([rng.randrange(bound) for _ in range(n * size)]))
    # ciphertext records: [tuples | out]
    ct = filled(torch, (n * size + n) * CT)
    ct[:n * size * CT] = random_tuples(torch, n * size, 3)
    before_ex, before_ct = ex.clone(), ct.clone()
    pe, pc = ex.data_ptr(), ct.data_ptr()
    p_tab, p_r, p_e, p_rho, p_rows = (pe + w * o for o in (o_tab, o_r, o_e, o_rho, o_rows))
    p_tup, p_out = pc, pc + w * n * size * CT
    rot = lambda tab=p_tab, n_tab=2, r=p_r, out=p_rows, n=n, bits=b: E.lut_rotate_records(tab, n_tab, r, out, n, bits)      # noqa: E731
    sel = lambda e=p_e, tup=p_tup, out=p_out, n=n, bits=b: E.lut_select_records(e, tup, out, n, bits)      # noqa: E731
    tup = lambda tab=p_tab, n_tab=2, out=p_tup, n=n, bits=b, kk=k: E.lut_tuples_records(      # noqa: E731
        tab, n_tab, p_r, p_rho, recs["h"], recs["pk"], recs["f"], out, n, bits, kk)
    calls = [lambda: rot(bits=0), lambda: rot(bits=13), lambda: rot(n_tab=0), lambda: rot(n_tab=3),
             lambda: rot(out=p_tab), lambda: rot(out=p_r - w), lambda: rot(out=p_r), lambda: rot(out=p_r + w * n * 32 - w),
             lambda: sel(bits=0), lambda: sel(bits=13), lambda: sel(out=p_tup), lambda: sel(out=p_out - w), lambda: sel(out=p_e),
             lambda: tup(bits=0), lambda: tup(bits=13), lambda: tup(n_tab=0), lambda: tup(n_tab=3), lambda: tup(bits=9, kk=8),
             lambda: tup(out=p_tab), lambda: tup(out=p_r), lambda: tup(out=p_rho), lambda: tup(out=p_rows - w)]
    for i, call in enumerate(calls):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL, i
    rot(tab=0, r=0, out=0, n=0)                                      # nothing to do
    sel(e=0, tup=0, out=0, n=0)
    tup(tab=0, out=0, n=0)
    torch.cuda.synchronize()
    assert torch.equal(ex, before_ex) and torch.equal(ct, before_ct)
    assert E.device_status(clear=False) == 0
    # the bound itself runs: one element, 4096 entries
    tab12, r12 = LC.table(12, 1, rng), [(4095, 1)]
    assert np.array_equal(rotate(E, torch, tab12, 1, r12, 12), LC.records(LC.rotate(tab12, 1, r12, 12)))
    assert E.device_status(clear=False) == 0


def test_lookups_through_the_host_layer(tmp_path):
    """local_bench lookup 64: a random 8-bit table, relu, max and a 2 x 2 max pool over 64 elements through the single-key and
    the 2-of-3 threshold client agree with the plaintext computation with ONE opened value per element per lookup (three per
    output of the 2 x 2 max pool), the c1 of a tuple tensor are pairwise distinct in the default randomness mode, and the tensor
    it serialises is valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "lookup", "64"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert r.stdout.count("opened_values 64,") == 6, r.stdout                  # table, relu, max: one per element, two clients
    assert r.stdout.count("opened_values 48 for 16 outputs,") == 2, r.stdout     # the 2 x 2 max pool: three per output
    assert "FAILED" not in r.stdout, r.stdout
    assert "distinct c1: yes" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_lookup.bin", "rb").read()) == 1


def test_lookups_timed_leg_through_the_host_layer(tmp_path):
    """local_bench lookup 8 1: the timed relu that tools/bench_ops.py reads, at the smallest size that keeps the five fixed
    values and the 2 x 2 max pool (a multiple of 4)"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "lookup", "8", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("lookup_json: ")]
    j = json.loads(line[len("lookup_json: "):])
    assert list(j) == ["E", "bits", "runs", "relu_ms", "relu_ms_min_max"]
    assert j["bits"] == 8
