"""GPU: piecewise-polynomial activations on ciphertext tensors from one opened value (cofhe_amd/csrc/spline.hip): k_spline_rows
and k_spline_powers against Python integers, k_spline_close against the C++/GMP oracle byte for byte, the tuples entry point
against the fresh encryption byte for byte, the whole protocol at the ABI through decryption, the bytes entry point, the
refusals, and the protocol through the C++ host layer."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import spline_cases as SC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records  # noqa: F401
import oracle_lib as O
from plain_mm_cases import check_output
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL, ESHAPE = -1, -2
REC = 168
CT = 2 * REC                                 # words of a ciphertext
FILL = 0xA5A5A5A5
KERNELS = ("k_spline_rows", "k_spline_powers", "k_spline_close")


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def filled(torch, words):
    return torch.full((words,), FILL - (1 << 32), dtype=torch.int32, device="cuda")


def shifted(torch, arr, shift):
    """the array on the device, starting `shift` words beyond a 16-byte boundary; returns (the tensor that owns it, its pointer)"""
    t = dev(torch, np.concatenate([np.zeros(shift, np.uint32), arr]))
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * shift


def rows(E, torch, pieces, n_tab, rs, b, t, d, k, shift=0):
    """the rows' records; every word of the output pre-filled; shift: every pointer that many words beyond a 16-byte boundary"""
    n = len(rs)
    (keep_t, pt), (keep_r, pr) = shifted(torch, SC.piece_records(pieces), shift), shifted(torch, SC.records(rs), shift)
    out = filled(torch, (n << b) * (d + 1) * 32 + shift)
    E.spline_rows_records(pt, n_tab, pr, out.data_ptr() + 4 * shift, n, b, t, d, k)
    torch.cuda.synchronize()
    got = host(out)
    assert (got[:shift] == FILL).all()
    return got[shift:]


def powers(E, torch, es, d, k, shift=0):
    n = len(es)
    keep_e, pe = shifted(torch, SC.records(es), shift)
    out = filled(torch, n * d * 32 + shift)
    E.spline_powers_records(pe, out.data_ptr() + 4 * shift, n, d, k)
    torch.cuda.synchronize()
    got = host(out)
    assert (got[:shift] == FILL).all()
    return got[shift:]


@pytest.mark.parametrize("n", [1, 63, 65])
@pytest.mark.parametrize("b,t,d", [(2, 3, 2), (3, 0, 1)])
def test_rows_and_powers_match_python_integers(tiny, b, t, d, n):
    """k = 8: the rows word for word with one table, three (where 3 divides n) and one per element, the powers word for word;
    masks and opened values from every family of spline_cases, coefficients with set sign words and of 992 bits; every output word
    pre-filled and written; one launch per call, under the kernels' own profile names"""
    import torch
    delta, k, *_ = setup(tiny)
    E = engine(delta)
    rng = random.Random(1000 * n + 10 * b + d)
    rs, es = SC.values(t, b, k, n, rng), SC.values(t, b, k, n, rng)
    for name in KERNELS:
        E.profile_read(name, clear=True)
    try:
        E.set_option("profile_kernels", 1)
        launches = 0
        for n_tab in sorted({1, 3, n}):
            if n % n_tab:
                continue
            pieces = SC.table(b, d, k, n_tab, rng)
            check_output(rows(E, torch, pieces, n_tab, rs, b, t, d, k), SC.rows(pieces, n_tab, rs, b, t, d, k), k)
            launches += 1
        check_output(powers(E, torch, es, d, k), SC.powers(es, d, k), k)
        assert E.profile_read("k_spline_rows")[1] == launches
        assert E.profile_read("k_spline_powers")[1] == 1
        assert E.profile_read("k_spline_close", clear=True)[1] == 0          # clear=True drops the spans of every name
    finally:
        E.set_option("profile_kernels", 0)
        for name in KERNELS:
            E.profile_read(name, clear=True)


@pytest.mark.parametrize("shift", [4, 1])
def test_rows_and_powers_at_shifted_pointers(tiny, shift):
    """every pointer 4 words past a 16-byte boundary, and 1 word past one (4-byte alignment only): the same records, and nothing
    before the shifted outputs is touched; n = 9 with three tables; also a degree of 8 at k = 8"""
    import torch
    delta, k, *_ = setup(tiny)
    E = engine(delta)
    rng = random.Random(90 + shift)
    for b, t, d in ((2, 3, 2), (3, 0, 1), (2, 6, 8)):
        n, n_tab = 9, 3
        rs, es, pieces = SC.values(t, b, k, n, rng), SC.values(t, b, k, n, rng), SC.table(b, d, k, n_tab, rng)
        want = SC.rows(pieces, n_tab, rs, b, t, d, k)
        check_output(rows(E, torch, pieces, n_tab, rs, b, t, d, k, shift=shift), want, k)
        check_output(powers(E, torch, es, d, k, shift=shift), SC.powers(es, d, k), k)


@pytest.mark.parametrize("k,d", [(128, 2), (300, 3)])
def test_rows_and_powers_beyond_one_limb(tiny, k, d):
    """the same kernels at k = 128 (the register array of 8 limbs) and k = 300 (the runtime limb count, whose working array is
    the rows' own output records), with the segment field straddling a word (t = 30, b = 4) and at the top of k"""
    import torch
    E = engine(setup(tiny)[0])
    rng = random.Random(k + d)
    for t, b in ((30, 4), (k - 3, 3)):
        n, n_tab = 7, 1
        rs, es, pieces = SC.values(t, b, k, n, rng), SC.values(t, b, k, n, rng), SC.table(b, d, k, n_tab, rng)
        check_output(rows(E, torch, pieces, n_tab, rs, b, t, d, k), SC.rows(pieces, n_tab, rs, b, t, d, k), k)
        check_output(powers(E, torch, es, d, k), SC.powers(es, d, k), k)


def close_case(E, torch, prm, n, b, t, d, es, seed):
    """tuples of real ciphertexts (fresh encryptions of random plaintexts), closed at the opened values es; returns (tuples as
    [n 2^b (d + 1), CT] host words, the closed ciphertexts as a device tensor)"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    m = (n << b) * (d + 1)
    tuples = fresh(E, torch, recs, [rng.getrandbits(k) for _ in range(m)], [rng.randrange(bound) for _ in range(m)], k)
    out = filled(torch, n * CT)
    de = dev(torch, SC.records(es))
    E.spline_close_records(de.data_ptr(), tuples.data_ptr(), out.data_ptr(), n, b, t, d, k)
    torch.cuda.synchronize()
    return tuples, out


def oracle_close(E, delta, tuples, es, n, b, t, d, k):
    """[q_0] o prod_c [q_c]^(e^c mod 2^k) over the selected row, by compose and pow of the GMP oracle"""
    tw = host(tuples).reshape(n << b, d + 1, CT)
    sel = [(i << b) + SC.index(e, t, b, k) for i, e in enumerate(es)]
    to_b = lambda c: E.records_to_bytes(np.ascontiguousarray(tw[sel, c]).reshape(-1), [n])       # noqa: E731
    acc = to_b(0)
    pw = SC.powers(es, d, k)
    for c in range(1, d + 1):
        acc = O.add(delta, acc, O.scal_1d(delta, _pt_bytes([n], pw[(c - 1) * n:c * n]), to_b(c)))
    return acc, sel


def opened_values(t, b, k, n, rng):
    """e = 0, e with the top bit set, e = 2^(k-1) whose higher powers vanish, -1, then values of spline_cases' families"""
    fixed = [(0, 0), ((1 << (k - 1)) | 5, 0), (1 << (k - 1), 0), (1, 1), (0, 1)]
    return (fixed + SC.values(t, b, k, max(n, 1), rng))[:n] if n > 1 else [fixed[rng.randrange(3)]]


@pytest.mark.parametrize("d", [1, 3])
@pytest.mark.parametrize("n", [1, 16, 17])
def test_close_matches_the_oracle(tiny, n, d):
    """k_spline_close on either side of a workgroup's 16 ciphertexts equals compose and pow of the GMP oracle over the selected row
    byte for byte: opened values 0 (the result is [q_0] itself), with the top bit set, 2^(k-1) (d = 3: its powers vanish), set
    sign words; one launch of each of the two kernels of the closing step"""
    import torch
    delta, k, *_ = setup(tiny)
    E = engine(delta)
    b, t = 2, 3
    rng = random.Random(100 * n + d)
    runs = [opened_values(t, b, k, n, rng)] if n > 1 else [[(0, 0)], [((1 << (k - 1)) | 5, 0)], [(1 << (k - 1), 0)]]
    for name in KERNELS:
        E.profile_read(name, clear=True)
    try:
        E.set_option("profile_kernels", 1)
        for es in runs:
            tuples, out = close_case(E, torch, tiny, n, b, t, d, es, 7 * n + d)
            want, sel = oracle_close(E, delta, tuples, es, n, b, t, d, k)
            assert E.records_to_bytes(host(out), [n]) == want
            for i, e in enumerate(es):
                if SC.residue(e, k) == 0:
                    assert np.array_equal(host(out).reshape(n, CT)[i], host(tuples).reshape(n << b, d + 1, CT)[sel[i], 0])
        assert E.profile_read("k_spline_powers")[1] == len(runs)
        assert E.profile_read("k_spline_close", clear=True)[1] == len(runs)
    finally:
        E.set_option("profile_kernels", 0)
        for name in KERNELS:
            E.profile_read(name, clear=True)
    assert E.device_status(clear=False) == 0


def test_close_at_128_bits_is_pow_dot_and_a_composition(params128):
    """n = 3, d = 2 at k = 128, b = 3, t = 30 (the segment field straddles a word): the oracle's bytes, and the bytes of
    pow_dot_records on the gathered bases composed with the constant term by compose_records"""
    import torch
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    n, b, t, d = 3, 3, 30, 2
    es = [((1 << (k - 1)) | (5 << 30) | 77, 0), (0, 0), ((3 << 30) + 12345, 1)]
    tuples, out = close_case(E, torch, prm, n, b, t, d, es, 128)
    want, sel = oracle_close(E, delta, tuples, es, n, b, t, d, k)
    assert E.records_to_bytes(host(out), [n]) == want
    tw = host(tuples).reshape(n << b, d + 1, CT)
    bases = dev(torch, np.ascontiguousarray(np.stack([tw[sel, c] for c in range(1, d + 1)])).reshape(-1))        # power-major
    q0 = dev(torch, np.ascontiguousarray(tw[sel, 0]).reshape(-1))
    pw = dev(torch, SC.int_records(SC.powers(es, d, k)))
    prod, got = torch.zeros(n * CT, dtype=torch.int32, device="cuda"), torch.zeros(n * CT, dtype=torch.int32, device="cuda")
    E.pow_dot_records(bases.data_ptr(), pw.data_ptr(), prod.data_ptr(), n, d)
    E.compose_records(prod.data_ptr(), q0.data_ptr(), got.data_ptr(), 2 * n)
    torch.cuda.synchronize()
    assert torch.equal(got, out)


def test_tuples_are_the_fresh_encryption_of_the_rows(params128):
    """spline_tuples_records at n = 3, b = 2, d = 2 equals encrypt_fresh_records over the output of spline_rows_records byte for
    byte, and the c1 of its 36 ciphertexts are pairwise distinct"""
    import torch
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    rng = random.Random(53)
    n, b, t, d = 3, 2, 30, 2
    m = (n << b) * (d + 1)
    pieces, rs = SC.table(b, d, k, 1, rng), SC.values(t, b, k, n, rng)
    rho = [rng.randrange(bound) for _ in range(m)]
    dt, dr, drho = dev(torch, SC.piece_records(pieces)), dev(torch, SC.records(rs)), dev(torch, exp_records(rho))
    rws = torch.zeros(m * 32, dtype=torch.int32, device="cuda")
    E.spline_rows_records(dt.data_ptr(), 1, dr.data_ptr(), rws.data_ptr(), n, b, t, d, k)
    want = torch.zeros(m * CT, dtype=torch.int32, device="cuda")
    E.encrypt_fresh_records(rws.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], want.data_ptr(), m, k)
    got = filled(torch, m * CT)
    E.spline_tuples_records(dt.data_ptr(), 1, dr.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], got.data_ptr(), n, b, t, d, k)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    c1 = host(got).reshape(m, 2, REC)[:, 0]
    assert len({r.tobytes() for r in c1}) == m


def protocol(E, torch, prm, xs, table, b, t, seed):
    """fresh [x] and [r], the tuples of the table (2^b pieces of d + 1 integers), e = Dec([x] - [r]) opened, the closing step,
    decryption; returns (masks, opened values, tuple buffer, closed ciphertexts, their plaintexts)"""
    delta, k, forms, recs, bound = setup(prm)
    rng = random.Random(seed)
    n, M, d = len(xs), 1 << k, len(table[0]) - 1
    m = (n << b) * (d + 1)
    rand = lambda cnt: [rng.randrange(bound) for _ in range(cnt)]       # noqa: E731
    rs = [rng.getrandbits(k) for _ in range(n)]
    cx, cr = fresh(E, torch, recs, xs, rand(n), k), fresh(E, torch, recs, rs, rand(n), k)
    dt, dr, drho = dev(torch, exp_records([c for p in table for c in p])), dev(torch, exp_records(rs)), dev(torch, exp_records(rand(m)))
    tuples = torch.zeros(m * CT, dtype=torch.int32, device="cuda")
    E.spline_tuples_records(dt.data_ptr(), 1, dr.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], tuples.data_ptr(), n, b, t, d, k)
    diff = torch.zeros_like(cx)
    E.sub_ciphertext_records(cx.data_ptr(), cr.data_ptr(), diff.data_ptr(), n)
    torch.cuda.synchronize()
    es = decrypt(E, torch, prm, diff, n, k)
    assert es == [(x - r) % M for x, r in zip(xs, rs)]
    out = filled(torch, n * CT)
    E.spline_close_records(dev(torch, exp_records(es)).data_ptr(), tuples.data_ptr(), out.data_ptr(), n, b, t, d, k)
    torch.cuda.synchronize()
    return rs, es, tuples, out, decrypt(E, torch, prm, out, n, k)


@pytest.mark.parametrize("b,t,d", [(2, 3, 2), (3, 0, 1)])
def test_the_whole_protocol_at_8_bits(tiny, b, t, d):
    """k = 8: every x of Z/2^k (so every x of the window, and every x outside it, where it wraps) against a table of random
    coefficients, so that a wrong piece cannot pass; every element decrypts to exactly S_{seg(x) - c}(x) with c from the known r,
    and to its own piece when t = 0"""
    import torch
    prm = tiny
    delta, k, *_ = setup(prm)
    assert k == 8
    E = engine(delta)
    rng = random.Random(80 + b)
    xs = list(range(1 << k))
    rng.shuffle(xs)
    table = [[rng.randrange(1 << k) for _ in range(d + 1)] for _ in range(1 << b)]
    rs, es, _, _, ys = protocol(E, torch, prm, xs, table, b, t, 800 + b)
    want = [SC.expected(table, x, r, b, t, k) for x, r in zip(xs, rs)]
    assert ys == [v for v, _ in want]
    if t == 0:
        assert [p for _, p in want] == [SC.segment(x, t, b) for x in xs]
    else:
        assert {(SC.segment(x, t, b) - p) % (1 << b) for x, (_, p) in zip(xs, want)} == {0, 1}        # both cases were seen


def test_the_whole_protocol_at_128_bits_and_the_bytes_entry_point(params128):
    """n = 4, b = 3, t = 30, d = 2 at k = 128: x of both signs inside the 33-bit window and outside it; coefficients up to 2^k - 1;
    every element decrypts to S_{seg(x) - c}(x); spline_close_tensors_bytes returns the same tensor serialised, for a [4] and a
    [2, 2] tensor, and the oracle accepts it; a tuple tensor of another shape is COFHE_HIP_ESHAPE"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, _ = setup(prm)
    E = engine(delta)
    rng = random.Random(128)
    n, b, t, d, M = 4, 3, 30, 2, 1 << k
    xs = [(1 << 31) + 12345, M - (3 << 30) - 7, (1 << 100) + (5 << 30), rng.getrandbits(k)]
    table = [[M - 1, rng.getrandbits(k), rng.getrandbits(64)] for _ in range(1 << b)]
    rs, es, tuples, out, ys = protocol(E, torch, prm, xs, table, b, t, 1280)
    assert ys == [SC.expected(table, x, r, b, t, k)[0] for x, r in zip(xs, rs)]
    want = E.records_to_bytes(host(out), [n])
    tb = host(tuples)
    got = E.spline_close_tensors_bytes(_pt_bytes([n], es), E.records_to_bytes(tb, [n, 8, 3]), t, k)
    assert got == want
    assert O.check_tensor(delta, got) == 1
    got2 = E.spline_close_tensors_bytes(_pt_bytes([2, 2], es), E.records_to_bytes(tb, [2, 2, 8, 3]), t, k)
    assert got2 == E.records_to_bytes(host(out), [2, 2])
    for eb, tbytes in ((_pt_bytes([n], es), E.records_to_bytes(tb, [n * 8, 3])),                      # no piece dimension
                       (_pt_bytes([n], es), E.records_to_bytes(tb, [n, 3, 8])),                       # transposed: 3 is no power of two
                       (_pt_bytes([n], es), E.records_to_bytes(tb, [n, 24, 1])),                      # 24 pieces of degree 0
                       (_pt_bytes([n - 1], es[:-1]), E.records_to_bytes(tb, [n, 8, 3])),
                       (_pt_bytes([n, 1], es), E.records_to_bytes(tb, [n, 8, 3]))):
        with pytest.raises(CofheHipError) as ei:
            E.spline_close_tensors_bytes(eb, tbytes, t, k)
        assert ei.value.code == ESHAPE


def test_the_bytes_entry_point_refuses_a_forged_tuple():
    """spline_close_tensors_bytes is composed from unpack_tensor_device, so it stands behind the form gate like the library's own
    *_tensors_bytes entry points: one equation forgery (c + 1) and one non-primitive forgery as c1 of the first entry and as c2
    of the last of a [2, 2, 2] tuple tensor are refused, and the same call with valid forms goes through"""
    import form_gate_cases as G
    from cofhe_amd import CofheHipError
    dsc = G.discriminants()[1]
    E = engine(dsc.delta)
    ok = [G.as_form(cs.rec) for cs in G.passes(dsc)]
    by = {cs.label: cs.rec for cs in dsc.cases}
    e = _pt_bytes([2], [0, 0])                                  # e = 0: the result is the constant term of row 0, a copy

    def tuples(forged=None, at=None):
        cts = [(ok[2 * i % len(ok)], ok[(2 * i + 1) % len(ok)]) for i in range(8)]
        if at == "first_c1":
            cts[0] = (forged, cts[0][1])
        if at == "last_c2":
            cts[-1] = (cts[-1][0], forged)
        return cts, P.serialize_ciphertext_tensor([2, 2, 2], cts)

    cts, valid = tuples()
    assert E.spline_close_tensors_bytes(e, valid, 0, 8) == P.serialize_ciphertext_tensor([2], [cts[0], cts[4]])
    for label in ("c_plus_1", "content2_random"):
        for at in ("first_c1", "last_c2"):
            with pytest.raises(CofheHipError, match="not a reduced form"):
                E.spline_close_tensors_bytes(e, tuples(G.as_form(by[label]), at)[1], 0, 8)
    assert E.device_status(clear=False) == 0


def test_refusals_leave_the_buffers_unchanged(params128):
    """bits = 0, d = 0 and 9, 2^bits (d + 1) > 4096, shift + bits > kbits, kbits = 0 and 640, n_tab = 0, n no multiple of n_tab
    and an output that overlaps an input, at each records entry point: COFHE_HIP_EINVAL, nothing written, the status word clear;
    n = 0 does nothing; shift = 0 runs"""
    import torch
    from cofhe_amd import CofheHipError
    prm = params128
    delta, k, forms, recs, bound = setup(prm)
    E = engine(delta)
    rng = random.Random(9)
    n, b, t, d, w = 4, 2, 5, 2, 4
    per = (1 << b) * (d + 1)
    # exponent records: [pieces (2 tables) | r | e | rho | rows | powers]
    o_tab, o_r = 0, 2 * per * 32
    o_e, o_rho = o_r + n * 32, o_r + 2 * n * 32
    o_rows = o_rho + n * per * 32
    o_pw = o_rows + n * per * 32
    ex = filled(torch, o_pw + n * d * 32)
    ex[:o_r] = dev(torch, SC.piece_records(SC.table(b, d, k, 2, rng)))
    ex[o_r:o_e] = dev(torch, SC.records(SC.values(t, b, k, n, rng)))
    ex[o_e:o_rho] = dev(torch, SC.records(SC.values(t, b, k, n, rng)))
    ex[o_rho:o_rows] = dev(torch, exp_records([rng.randrange(bound) for _ in range(n * per)]))
    # ciphertext records: [tuples | out]
    ct = filled(torch, (n * per + n) * CT)
    before_ex, before_ct = ex.clone(), ct.clone()
    pe, pc = ex.data_ptr(), ct.data_ptr()
    p_tab, p_r, p_e, p_rho, p_rows, p_pw = (pe + w * o for o in (o_tab, o_r, o_e, o_rho, o_rows, o_pw))
    p_tup, p_out = pc, pc + w * n * per * CT

    def row(tab=p_tab, n_tab=2, r=p_r, out=p_rows, n=n, bits=b, shift=t, d=d, kk=k):
        E.spline_rows_records(tab, n_tab, r, out, n, bits, shift, d, kk)

    def tup(tab=p_tab, n_tab=2, out=p_tup, n=n, bits=b, shift=t, d=d, kk=k):
        E.spline_tuples_records(tab, n_tab, p_r, p_rho, recs["h"], recs["pk"], recs["f"], out, n, bits, shift, d, kk)

    def pw(e=p_e, out=p_pw, n=n, d=d, kk=k):
        E.spline_powers_records(e, out, n, d, kk)

    def cls(e=p_e, tu=p_tup, out=p_out, n=n, bits=b, shift=t, d=d, kk=k):
        E.spline_close_records(e, tu, out, n, bits, shift, d, kk)

    shapes = [dict(bits=0), dict(d=0), dict(d=9), dict(bits=11, d=2), dict(bits=12, d=1), dict(shift=k - b + 1), dict(bits=3, shift=6, kk=8),
              dict(kk=0), dict(kk=640)]
    calls = [lambda kw=kw, f=f: f(**kw) for kw in shapes for f in (row, tup, cls)]
    calls += [lambda: row(n_tab=0), lambda: row(n_tab=3), lambda: tup(n_tab=0), lambda: tup(n_tab=3),
              lambda: row(out=p_tab), lambda: row(out=p_r - w), lambda: row(out=p_r), lambda: row(out=p_r + w * n * 32 - w),
              lambda: tup(out=p_tab), lambda: tup(out=p_r), lambda: tup(out=p_rho), lambda: tup(out=p_rows - w),
              lambda: pw(d=0), lambda: pw(d=9), lambda: pw(kk=0), lambda: pw(kk=640), lambda: pw(out=p_e), lambda: pw(out=p_e - w * n * d * 32 + w),
              lambda: cls(out=p_tup), lambda: cls(out=p_out - w), lambda: cls(out=p_e)]
    for i, call in enumerate(calls):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL, i
    row(tab=0, r=0, out=0, n=0)                                      # nothing to do
    tup(tab=0, out=0, n=0)
    pw(e=0, out=0, n=0)
    cls(e=0, tu=0, out=0, n=0)
    torch.cuda.synchronize()
    assert torch.equal(ex, before_ex) and torch.equal(ct, before_ct)
    assert E.device_status(clear=False) == 0
    # shift = 0 is allowed, and so is the largest tuple: 4096 ciphertexts' worth of rows for one element
    pieces, r1 = SC.table(9, 7, k, 1, rng), [(12345, 1)]
    check_output(rows(E, torch, pieces, 1, r1, 9, 0, 7, k), SC.rows(pieces, 1, r1, 9, 0, 7, k), k)
    assert E.device_status(clear=False) == 0


def test_sigmoid_through_the_host_layer(tmp_path):
    """local_bench spline 8: the sigmoid spline at the bench defaults (32 pieces of degree 2 over a 16-bit window) over 8 elements
    through the single-key and the 2-of-3 threshold client decrypts to the table's own value on the element's piece or the one
    below, within the builder's reported error of the sigmoid, with ONE opened value per element; the c1 of the tuple tensor are
    pairwise distinct in the default randomness mode, and the tensor it serialises is valid"""
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "spline", "8"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    assert r.stdout.count("opened_values 8,") == 2, r.stdout
    assert "distinct c1: yes" in r.stdout, r.stdout
    (line,) = [ln for ln in r.stdout.splitlines() if ln.startswith("spline_error: ")]
    worst, reported = (float(v) for v in re.fullmatch(r"spline_error: worst (\S+) reported (\S+)", line).groups())
    assert worst <= reported
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_spline.bin", "rb").read()) == 1
