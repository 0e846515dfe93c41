"""GPU: the exact sign, ReLU and max on windows of up to 64 bits from digit comparisons (cofhe_amd/csrc/compare.hip): k_cmp_rows
against Python integers, k_cmp_close byte for byte against compositions of the same entries by compose_records, the tuples entry
point against the fresh encryption, the whole protocol at the ABI through decryption, the bytes route, the refusals, and the
protocol through the C++ host layer."""
import os
import random
import subprocess

import numpy as np
import pytest

import compare_cases as CC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL, ESHAPE = -1, -2
REC = 168
CT = 2 * REC                                 # words of a ciphertext
FILL = 0xA5A5A5A5
KERNELS = ("k_cmp_rows", "k_cmp_close")


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


def filled(torch, words):
    return torch.full((words,), FILL - (1 << 32), dtype=torch.int32, device="cuda")


def shifted(torch, arr, shift):
    """a device copy of arr that starts `shift` words beyond a 16-byte boundary"""
    t = dev(torch, np.concatenate([np.zeros(shift, np.uint32), np.ascontiguousarray(arr, dtype=np.uint32)]))
    assert t.data_ptr() % 16 == 0
    return t[shift:]


class Spans:
    """the launches of the two kernels under "profile_kernels", cleared on the way in and out"""

    def __init__(self, E):
        self.E = E

    def __enter__(self):
        for name in KERNELS:
            self.E.profile_read(name, clear=True)
        self.E.set_option("profile_kernels", 1)
        return self

    def launches(self, name):
        return self.E.profile_read(name)[1]

    def __exit__(self, *exc):
        self.E.set_option("profile_kernels", 0)
        for name in KERNELS:
            self.E.profile_read(name, clear=True)


def rows(E, torch, rs, k, bits, d, shift=0):
    entries = CC.digits_of(bits, d) << d
    dr = shifted(torch, CC.records(rs), shift)
    out = filled(torch, len(rs) * entries * 32 + shift + 4)
    E.cmp_rows_records(dr.data_ptr(), out.data_ptr() + 4 * shift, len(rs), bits, d, k)
    torch.cuda.synchronize()
    got = host(out)
    assert (got[:shift] == FILL).all() and (got[shift + len(rs) * entries * 32:] == FILL).all()
    return got[shift:shift + len(rs) * entries * 32]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("k,bits,d", CC.PARAMS)
def test_rows_match_python_integers(tiny, k, bits, d, shift):
    """k_cmp_rows word for word at the parameter sets of the CPU tier, by 16-byte pieces and (pointers one word beyond a 16-byte
    boundary) by dwords; masks from every family of compare_cases; one launch under the kernel's own profile name"""
    import torch
    E = engine(setup(tiny)[0])
    rs = CC.values(bits, k, 3 if d >= 7 else 23, random.Random(k + bits + d))
    with Spans(E) as sp:
        got = rows(E, torch, rs, k, bits, d, shift)
        assert sp.launches("k_cmp_rows") == 1
    assert np.array_equal(got, CC.records(CC.rows(rs, bits, d)))


@pytest.fixture(scope="module")
def pool(params128):
    """64 valid ciphertexts at s128_k128 (fresh encryptions of random plaintexts) as [64, CT] host words"""
    import torch
    delta, k, forms, recs, bound = setup(params128)
    E = engine(delta)
    rng = random.Random(64)
    cts = fresh(E, torch, recs, [rng.getrandbits(k) for _ in range(64)], [rng.randrange(bound) for _ in range(64)], k)
    return host(cts).reshape(64, CT).copy()


def close(E, torch, es, tuples, k, bits, d, shift=0):
    """(pairs as [n, 2, CT] host words, wrap as [n, 32]); tuples: a device tensor; shift: e, out and wrap start that many words
    beyond a 16-byte boundary; the words around both outputs must stay as they were"""
    n = len(es)
    de = shifted(torch, CC.records(es), shift)
    out, wrap = filled(torch, 2 * n * CT + shift + 4), filled(torch, n * 32 + shift + 4)
    E.cmp_close_records(de.data_ptr(), tuples.data_ptr(), out.data_ptr() + 4 * shift, wrap.data_ptr() + 4 * shift, n, bits, d, k)
    torch.cuda.synchronize()
    o, w = host(out), host(wrap)
    assert (o[:shift] == FILL).all() and (o[shift + 2 * n * CT:] == FILL).all()
    assert (w[:shift] == FILL).all() and (w[shift + n * 32:] == FILL).all()
    return o[shift:shift + 2 * n * CT].reshape(n, 2, CT), w[shift:shift + n * 32].reshape(n, 32)


def composed(E, torch, tuples_host, es, bits, d):
    """[n, 2, CT]: for both thresholds of every opened value the left fold of the selected entries by compose_records"""
    n, nd = len(es), CC.digits_of(bits, d)
    sel = np.zeros((n, 2, nd), dtype=np.int64)
    for i, e in enumerate(es):
        a, b, _ = CC.thresholds(CC.low(e, bits), bits)
        sel[i, 0], sel[i, 1] = CC.entries(i, a, bits, d), CC.entries(i, b, bits, d)
    acc = dev(torch, np.ascontiguousarray(tuples_host[sel[:, :, 0].reshape(-1)]).reshape(-1))
    for j in range(1, nd):
        rhs = dev(torch, np.ascontiguousarray(tuples_host[sel[:, :, j].reshape(-1)]).reshape(-1))
        nxt = torch.zeros_like(acc)
        E.compose_records(acc.data_ptr(), rhs.data_ptr(), nxt.data_ptr(), 2 * n * 2)
        acc = nxt
    torch.cuda.synchronize()
    return host(acc).reshape(n, 2, CT), sel


# n = 1 (copies), n = 2 (no prefix composition), a middle case at the flagship parameters, n = 11 (the cap of the rounds)
CLOSE_SHAPES = ((8, 8), (2, 2), (16, 8), (2, 1), (32, 6), (11, 1), (64, 6))


@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("bits,d", CLOSE_SHAPES)
def test_close_matches_compositions_of_the_selected_entries(params128, pool, n, bits, d):
    """k_cmp_close byte for byte against compose_records over the same entries in the same order, for one element and for 33 (66
    limb groups: the last workgroup of 32 is partly filled), with 1, 2, 6 and 11 digits; the tuples are gathered from a pool of
    64 valid ciphertexts, so entries repeat (squarings among the compositions); wrap against Python integers; one launch; the
    status word clear"""
    import torch
    delta, k, *_ = setup(params128)
    E = engine(delta)
    nd = CC.digits_of(bits, d)
    assert nd == {(8, 8): 1, (2, 2): 1, (16, 8): 2, (2, 1): 2, (32, 6): 6, (11, 1): 11, (64, 6): 11}[(bits, d)]
    rng = random.Random(1000 * n + 10 * bits + d)
    es = CC.values(bits, k, 40, rng)[:n] if n > 1 else [rng.choice(CC.values(bits, k, 40, rng))]
    idx = np.array([rng.randrange(64) for _ in range(n * (nd << d))])
    tuples_host = pool[idx]
    tuples = dev(torch, tuples_host.reshape(-1))
    want, sel = composed(E, torch, tuples_host, es, bits, d)
    with Spans(E) as sp:
        got, wrap = close(E, torch, es, tuples, k, bits, d)
        assert sp.launches("k_cmp_close") == 1
    assert np.array_equal(got, want)
    if nd == 1:
        assert np.array_equal(got, tuples_host[sel[:, :, 0]])
    assert np.array_equal(wrap.reshape(-1), CC.records([(CC.thresholds(CC.low(e, bits), bits)[2], 0) for e in es]))
    assert E.device_status(clear=False) == 0
    assert O.check_tensor(delta, E.records_to_bytes(got.reshape(-1), [n, 2])) == 1


def test_close_at_shifted_pointers(params128, pool):
    """e, the tuples, out and wrap one word beyond a 16-byte boundary: the same bytes as the aligned call, nothing around the
    outputs touched"""
    import torch
    delta, k, *_ = setup(params128)
    E = engine(delta)
    n, bits, d = 5, 17, 5
    rng = random.Random(175)
    es = CC.values(bits, k, 40, rng)[:n]
    idx = np.array([rng.randrange(64) for _ in range(n * (CC.digits_of(bits, d) << d))])
    flat = pool[idx].reshape(-1)
    aligned, off = dev(torch, flat), shifted(torch, flat, 1)
    assert aligned.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    want, wrap = close(E, torch, es, aligned, k, bits, d)
    got, wrap1 = close(E, torch, es, off, k, bits, d, shift=1)
    assert np.array_equal(got, want) and np.array_equal(wrap1, wrap)
    assert np.array_equal(want, composed(E, torch, pool[idx], es, bits, d)[0])
    assert E.device_status(clear=False) == 0


def test_tuples_are_the_fresh_encryption_of_the_rows(params128):
    """cmp_tuples_records at n = 3, (bits, d) = (17, 5) equals encrypt_fresh_records over the output of cmp_rows_records byte for
    byte, and the c1 of its 384 ciphertexts are pairwise distinct"""
    import torch
    delta, k, forms, recs, bound = setup(params128)
    E = engine(delta)
    rng = random.Random(53)
    n, bits, d = 3, 17, 5
    m = n * (CC.digits_of(bits, d) << d)
    rs = CC.values(bits, k, n, rng)
    dr, drho = dev(torch, CC.records(rs)), dev(torch, exp_records([rng.randrange(bound) for _ in range(m)]))
    rws = torch.zeros(m * 32, dtype=torch.int32, device="cuda")
    E.cmp_rows_records(dr.data_ptr(), rws.data_ptr(), n, bits, d, k)
    want = torch.zeros(m * CT, dtype=torch.int32, device="cuda")
    E.encrypt_fresh_records(rws.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], want.data_ptr(), m, k)
    got = filled(torch, m * CT)
    E.cmp_tuples_records(dr.data_ptr(), drho.data_ptr(), recs["h"], recs["pk"], recs["f"], got.data_ptr(), n, bits, d, k)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    c1 = host(got).reshape(m, 2, REC)[:, 0]
    assert len({r.tobytes() for r in c1}) == m
    # the entries decrypt to 2^j sgn(r_j - c) mod 2^k
    M = 1 << k
    assert decrypt(E, torch, params128, got, m, k) == [(-mag if neg else mag) % M for mag, neg in CC.rows(rs, bits, d)]


class Party:
    """the protocol at the ABI: fresh encryptions, the opening (a decryption that counts what it opens), lookups and Beaver
    products from the records entry points"""

    def __init__(self, E, torch, prm, seed):
        self.E, self.torch, self.prm = E, torch, prm
        self.delta, self.k, self.forms, self.recs, self.bound = setup(prm)
        self.M = 1 << self.k
        self.rng = random.Random(seed)
        self.opened = 0

    def rand(self, m):
        return [self.rng.randrange(self.bound) for _ in range(m)]

    def enc(self, ms):
        return fresh(self.E, self.torch, self.recs, [m % self.M for m in ms], self.rand(len(ms)), self.k)

    def peek(self, cts, n):
        return decrypt(self.E, self.torch, self.prm, cts, n, self.k)

    def open(self, cts, n):
        self.opened += n
        return self.peek(cts, n)

    def zeros(self, n_ct):
        return self.torch.zeros(n_ct * CT, dtype=self.torch.int32, device="cuda")

    def sub(self, a, b, n):
        out = self.zeros(n)
        self.E.sub_ciphertext_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
        return out

    def add(self, a, b, n):
        out = self.zeros(n)
        self.E.add_ciphertext_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), n)
        return out

    def add_plain(self, a, ms, n):
        out = self.zeros(n)
        dm = dev(self.torch, exp_records([m % self.M for m in ms]))
        self.E.add_plain_records(a.data_ptr(), dm.data_ptr(), self.recs["f"], out.data_ptr(), n, self.k)
        return out

    def scal(self, a, ms, n):
        out = self.zeros(n)
        dm = dev(self.torch, exp_records(ms))
        self.E.pow_records(a.data_ptr(), dm.data_ptr(), out.data_ptr(), n)
        return out

    def masked(self, cx, n):
        """([r], r, the opened x - r)"""
        rs = [self.rng.getrandbits(self.k) for _ in range(n)]
        cr = self.enc(rs)
        return cr, rs, self.open(self.sub(cx, cr, n), n)

    def lookup(self, cx, n, table, b):
        _, rs, es = self.masked(cx, n)
        dt, dr, drho = (dev(self.torch, exp_records(v)) for v in (table, rs, self.rand(n << b)))
        tuples = self.zeros(n << b)
        self.E.lut_tuples_records(dt.data_ptr(), 1, dr.data_ptr(), drho.data_ptr(), self.recs["h"], self.recs["pk"], self.recs["f"], tuples.data_ptr(), n, b,
                                  self.k)
        out = self.zeros(n)
        de = dev(self.torch, exp_records(es))
        self.E.lut_select_records(de.data_ptr(), tuples.data_ptr(), out.data_ptr(), n, b)
        return out

    def product(self, cx, cy, n):
        """one Beaver product per element: two opened values each"""
        a, b = [self.rng.getrandbits(self.k) for _ in range(n)], [self.rng.getrandbits(self.k) for _ in range(n)]
        ca, cb, cc = self.enc(a), self.enc(b), self.enc([u * v for u, v in zip(a, b)])
        e, dd = self.open(self.sub(cx, ca, n), n), self.open(self.sub(cy, cb, n), n)
        s = self.add(self.add(self.scal(cb, e, n), self.scal(ca, dd, n), n), cc, n)
        return self.add_plain(s, [u * v for u, v in zip(e, dd)], n)

    def nonneg(self, cx, xs, bits, d):
        """[x >= 0] from a comparison tuple per element, cmp_close_records and one lookup of nd + 1 bits; the intermediate
        plaintexts are checked against the integers on the way"""
        E, torch, k, n, nd = self.E, self.torch, self.k, len(xs), CC.digits_of(bits, d)
        cr, rs, es = self.masked(cx, n)
        assert es == [(x - r) % self.M for x, r in zip(xs, rs)]
        m = n * (nd << d)
        tuples = self.zeros(m)
        dr, drho, de = (dev(torch, exp_records(v)) for v in (rs, self.rand(m), es))       # held: a dropped tensor's block is reused
        E.cmp_tuples_records(dr.data_ptr(), drho.data_ptr(), self.recs["h"], self.recs["pk"], self.recs["f"], tuples.data_ptr(), n, bits, d, k)
        pairs, wrap = self.zeros(2 * n), torch.zeros(n * 32, dtype=torch.int32, device="cuda")
        E.cmp_close_records(de.data_ptr(), tuples.data_ptr(), pairs.data_ptr(), wrap.data_ptr(), n, bits, d, k)
        torch.cuda.synchronize()
        th = [CC.thresholds(e % (1 << bits), bits) for e in es]
        wr = [int(w) for w in host(wrap).reshape(n, 32)[:, 0]]
        assert wr == [t[2] for t in th] and not host(wrap).reshape(n, 32)[:, 1:].any()
        s_want = [CC.s_value(r % (1 << bits), t[s], bits, d) % self.M for r, t in zip(rs, th) for s in (0, 1)]
        assert self.peek(pairs, 2 * n) == s_want                        # a look behind the curtain, not an opened value
        g = self.lookup(pairs, 2 * n, CC.sign_table(nd), nd + 1)
        gw = host(g).reshape(n, 2, CT)
        ga, gb = dev(torch, np.ascontiguousarray(gw[:, 0]).reshape(-1)), dev(torch, np.ascontiguousarray(gw[:, 1]).reshape(-1))
        return self.add_plain(self.sub(gb, ga, n), [1 - w for w in wr], n)

    def relu(self, cx, xs, bits, d):
        return self.product(cx, self.nonneg(cx, xs, bits, d), len(xs))

    def maximum(self, ca, cb, a, b, bits, d):
        """b + relu(a - b) on the (bits + 1)-bit window"""
        n = len(a)
        return self.add(cb, self.relu(self.sub(ca, cb, n), [u - v for u, v in zip(a, b)], bits + 1, d), n)


def run_protocol(party, xs, ys, bits, d):
    """sign and ReLU of xs on the window of `bits` bits, max of the halves of xs and ys (their difference stays in the window);
    every element against the integers, 3 opened values per element for the sign, 5 for ReLU and for max"""
    n, M = len(xs), party.M
    cx = party.enc(xs)
    before = party.opened
    s = party.nonneg(cx, xs, bits, d)
    assert party.opened - before == 3 * n
    assert party.peek(s, n) == [int(x >= 0) for x in xs]
    before = party.opened
    r = party.relu(cx, xs, bits, d)
    assert party.opened - before == 5 * n
    assert party.peek(r, n) == [max(x, 0) % M for x in xs]
    a, b = [x >> 1 for x in xs], [y >> 1 for y in ys]
    before = party.opened
    m = party.maximum(party.enc(a), party.enc(b), a, b, bits - 1, d)
    assert party.opened - before == 5 * n
    assert party.peek(m, n) == [max(u, v) % M for u, v in zip(a, b)]
    assert party.E.device_status(clear=False) == 0


@pytest.mark.parametrize("batch", [0, 1])
def test_the_whole_protocol_at_8_bits(tiny, batch):
    """tiny_k8, a window of 8 bits = k in 3 digits of 3 bits: all 256 values in two batches of 128, the edges -128, -1, 0, 1, 127
    among them; sign, ReLU and max decrypt to the integers"""
    import torch
    E = engine(setup(tiny)[0])
    xs = list(range(-128, 128))
    random.Random(8).shuffle(xs)
    xs = xs[128 * batch:128 * (batch + 1)]
    ys = xs[::-1]
    run_protocol(Party(E, torch, tiny, 80 + batch), xs, ys, 8, 3)


@pytest.mark.parametrize("bits,d", [(16, 4), (32, 6), (64, 8)])
def test_the_whole_protocol_at_128_bits(params128, bits, d):
    """s128_k128, 8 elements: the five edges of the window and three random values of it; sign, ReLU and max decrypt to the
    integers, with 3, 5 and 5 opened values per element"""
    import torch
    E = engine(setup(params128)[0])
    rng = random.Random(bits)
    xs = CC.edges(bits) + [rng.randrange(-(1 << (bits - 1)), 1 << (bits - 1)) for _ in range(3)]
    ys = xs[::-1][1:] + [rng.randrange(-(1 << (bits - 1)), 1 << (bits - 1))]
    run_protocol(Party(E, torch, params128, 1280 + bits), xs, ys, bits, d)


def plain(E, data):
    """(shape, values) of a serialised plaintext tensor of non-negative values"""
    shape, ex = E.bytes_to_exponents(data)
    ex = ex.reshape(-1, 32)
    assert not ex[:, 31].any()
    return shape, [int.from_bytes(row[:31].tobytes(), "little") for row in ex]


def test_the_bytes_route_equals_the_records_route(params128, pool):
    """Engine.cmp_close_tensors_bytes on serialised tensors returns the pairs [n, 2] and wrap [n] of cmp_close_records, for a [5]
    and a [5, 1] tensor, and the oracle accepts the pairs; a tuple tensor of another shape is COFHE_HIP_ESHAPE, parameters out
    of bounds COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    delta, k, *_ = setup(params128)
    E = engine(delta)
    n, bits, d = 5, 16, 4
    nd = CC.digits_of(bits, d)
    rng = random.Random(16)
    es = [rng.getrandbits(k) for _ in range(n - 1)] + [0]
    idx = np.array([rng.randrange(64) for _ in range(n * (nd << d))])
    flat = pool[idx].reshape(-1)
    pairs, wrap = close(E, torch, [(e, 0) for e in es], dev(torch, flat), k, bits, d)
    wr = [int(w) for w in wrap[:, 0]]
    got_p, got_w = E.cmp_close_tensors_bytes(_pt_bytes([n], es), E.records_to_bytes(flat, [n, nd, 1 << d]), bits, d, k)
    assert got_p == E.records_to_bytes(pairs.reshape(-1), [n, 2]) and plain(E, got_w) == ([n], wr)
    assert O.check_tensor(delta, got_p) == 1
    got_p, got_w = E.cmp_close_tensors_bytes(_pt_bytes([n, 1], es), E.records_to_bytes(flat, [n, 1, nd, 1 << d]), bits, d, k)
    assert got_p == E.records_to_bytes(pairs.reshape(-1), [n, 1, 2]) and plain(E, got_w) == ([n, 1], wr)
    eb = _pt_bytes([n], es)
    for e_bytes, t_bytes in ((eb, E.records_to_bytes(flat, [n, nd << d])), (eb, E.records_to_bytes(flat, [n, 1 << d, nd])),
                             (eb, E.records_to_bytes(flat, [nd, n, 1 << d])), (_pt_bytes([n - 1], es[:-1]), E.records_to_bytes(flat, [n, nd, 1 << d])),
                             (_pt_bytes([n, 1], es), E.records_to_bytes(flat, [n, nd, 1 << d]))):
        with pytest.raises(CofheHipError) as ei:
            E.cmp_close_tensors_bytes(e_bytes, t_bytes, bits, d, k)
        assert ei.value.code == ESHAPE
    for b2, d2, k2 in ((1, 1, k), (65, 8, k), (16, 0, k), (16, 9, k), (64, 5, k), (16, 4, 8)):
        with pytest.raises(CofheHipError) as ei:
            E.cmp_close_tensors_bytes(eb, E.records_to_bytes(flat, [n, nd, 1 << d]), b2, d2, k2)
        assert ei.value.code == EINVAL
    assert E.device_status(clear=False) == 0


def test_the_bytes_route_refuses_a_forged_tuple():
    """cmp_close_tensors_bytes is composed from unpack_tensor_device, so it stands behind the form gate like the library's own
    *_tensors_bytes entry points: one equation forgery (c + 1) and one non-primitive forgery as c1 of the first entry and as c2
    of the last of a [2, 1, 4] tuple tensor are refused, and the same call with valid forms goes through (one digit: copies)"""
    import form_gate_cases as G
    from cofhe_amd import CofheHipError
    dsc = G.discriminants()[1]
    E = engine(dsc.delta)
    ok = [G.as_form(cs.rec) for cs in G.passes(dsc)]
    by = {cs.label: cs.rec for cs in dsc.cases}
    e = _pt_bytes([2], [0, 3])          # bits = 2: u = 0 -> A = 2, B = 0, wrap; u = 3 -> A = 3, B = 1, wrap

    def tuples(forged=None, at=None):
        cts = [(ok[2 * i % len(ok)], ok[(2 * i + 1) % len(ok)]) for i in range(8)]
        if at == "first_c1":
            cts[0] = (forged, cts[0][1])
        if at == "last_c2":
            cts[-1] = (cts[-1][0], forged)
        return cts, P.serialize_ciphertext_tensor([2, 1, 4], cts)

    cts, valid = tuples()
    pairs, wrap = E.cmp_close_tensors_bytes(e, valid, 2, 2, 8)
    assert pairs == P.serialize_ciphertext_tensor([2, 2], [cts[2], cts[0], cts[4 + 3], cts[4 + 1]]) and plain(E, wrap) == ([2], [1, 1])
    for label in ("c_plus_1", "content2_random"):
        for at in ("first_c1", "last_c2"):
            with pytest.raises(CofheHipError, match="not a reduced form"):
                E.cmp_close_tensors_bytes(e, tuples(G.as_form(by[label]), at)[1], 2, 2, 8)
    assert E.device_status(clear=False) == 0


def test_refusals_leave_the_buffers_unchanged(params128, pool):
    """every parameter bound, bits > kbits, kbits = 0 and 640, and an output that overlaps an input or the other output, at each
    records entry point: COFHE_HIP_EINVAL, nothing written, the status word clear; n = 0 does nothing"""
    import torch
    from cofhe_amd import CofheHipError
    delta, k, forms, recs, bound = setup(params128)
    E = engine(delta)
    rng = random.Random(9)
    n, bits, d, w = 3, 8, 2, 4
    per = CC.digits_of(bits, d) << d
    # exponent records: [r | e | rho | rows | wrap]
    o_r, o_e, o_rho = 0, n * 32, 2 * n * 32
    o_rows = o_rho + n * per * 32
    o_wrap = o_rows + n * per * 32
    ex = filled(torch, o_wrap + n * 32)
    ex[:o_e] = dev(torch, CC.records(CC.values(bits, k, n, rng)))
    ex[o_e:o_rho] = dev(torch, CC.records(CC.values(bits, k, n, rng)))
    ex[o_rho:o_rows] = dev(torch, exp_records([rng.randrange(bound) for _ in range(n * per)]))
    # ciphertext records: [tuples | out]
    ct = filled(torch, (n * per + 2 * n) * CT)
    ct[:n * per * CT] = dev(torch, pool[np.arange(n * per) % 64].reshape(-1))
    before_ex, before_ct = ex.clone(), ct.clone()
    pe, pc = ex.data_ptr(), ct.data_ptr()
    p_r, p_e, p_rho, p_rows, p_wrap = (pe + w * o for o in (o_r, o_e, o_rho, o_rows, o_wrap))
    p_tup, p_out = pc, pc + w * n * per * CT

    def row(r=p_r, out=p_rows, n=n, bits=bits, d=d, kk=k):
        E.cmp_rows_records(r, out, n, bits, d, kk)

    def tup(out=p_tup, n=n, bits=bits, d=d, kk=k):
        E.cmp_tuples_records(p_r, p_rho, recs["h"], recs["pk"], recs["f"], out, n, bits, d, kk)

    def cls(e=p_e, tu=p_tup, out=p_out, wrap=p_wrap, n=n, bits=bits, d=d, kk=k):
        E.cmp_close_records(e, tu, out, wrap, n, bits, d, kk)

    shapes = [dict(bits=1), dict(bits=0), dict(bits=65, d=8), dict(bits=9, d=3, kk=8), dict(d=0), dict(d=9), dict(bits=64, d=5), dict(bits=8, d=1, kk=8),
              dict(kk=0), dict(kk=640)]
    calls = [lambda kw=kw, f=f: f(**kw) for kw in shapes for f in (row, tup, cls)]
    calls += [lambda: row(out=p_r), lambda: row(out=p_r + w * n * 32 - w), lambda: row(out=p_r - w * n * per * 32 + w),
              lambda: tup(out=p_r), lambda: tup(out=p_rho), lambda: tup(out=p_rho + w * n * per * 32 - w),
              lambda: cls(out=p_tup), lambda: cls(out=p_out - w), lambda: cls(out=p_e), lambda: cls(wrap=p_e), lambda: cls(wrap=p_tup),
              lambda: cls(wrap=p_out), lambda: cls(wrap=p_out + w * 2 * n * CT - w)]
    for i, call in enumerate(calls):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL, i
    row(r=0, out=0, n=0)                                             # nothing to do
    tup(out=0, n=0)
    cls(e=0, tu=0, out=0, wrap=0, n=0)
    torch.cuda.synchronize()
    assert torch.equal(ex, before_ex) and torch.equal(ct, before_ct)
    assert E.device_status(clear=False) == 0


def test_compare_through_the_host_layer(tmp_path):
    """local_bench compare 8 64: sign, ReLU and max over 8 elements of the widest window (its five edges among them) through
    the single-key and the 2-of-3 threshold client agree with the integers, with 3, 5 and 5 opened values per element, the c1
    of a tuple tensor are pairwise distinct in the default randomness mode, and the tensor it serialises is valid.  No timed
    runs: the 26 openings of the six calls are most of its time already."""
    bits = 64
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "compare", "8", str(bits)], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert "FAILED" not in r.stdout, r.stdout
    assert r.stdout.count("sign over 8 elements, opened_values_per_element 3,") == 2, r.stdout
    assert r.stdout.count("relu over 8 elements, opened_values_per_element 5,") == 2, r.stdout
    assert r.stdout.count("max over 8 elements, opened_values_per_element 5,") == 2, r.stdout
    assert "distinct c1: yes" in r.stdout, r.stdout
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    assert O.check_tensor(delta, open(tmp_path / "local_bench_compare.bin", "rb").read()) == 1
    d = CC.pick_digit_bits(bits, 128)
    assert "window %d bits, %d digits of %d bits," % (bits, CC.digits_of(bits, d), d) in r.stdout, r.stdout
