"""CPU: the per-thread bodies of the wire-format kernels -- wire.hpp (cofhe_amd/csrc), which k_unpack, k_widths and k_pack
call, compiled for the host -- against the plain-Python model of wire_cases: every slot width of every plane, unwritten bytes
(all outputs start as 0xA5), encodings our writer never produces, and every refusal by its error bits.  Exact.  No kernel runs;
the scan kernels are replaced by a serial sum (tests/test_gpu_wire.py runs them)."""
import ctypes as C
import os
import random
import struct
import subprocess

import numpy as np
import pytest

import wire_cases as W
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libwiresim.so")
A5 = 0xA5A5A5A5
GUARD = 64                                   # bytes / words past the end of every output that must stay 0xA5


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "wire_sim.cpp")
    deps = [src] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in ("wire.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    lib = C.CDLL(_SO)
    lib.wire_sim_unpack.restype = C.c_uint32
    return lib


def sim_unpack(sim, kind, data):
    """(err word, records) of a buffer whose header is well formed; the guard words past the last record are checked here"""
    shape, offs, body = W.split(kind, data)
    n_rec = len(offs) // W.INTS[kind]
    words = n_rec * W.REC_WORDS[kind]
    rec = np.zeros(words + GUARD, dtype=np.uint32)
    off = np.array(offs, dtype=np.uint64)
    b = np.frombuffer(body + b"\xEE" * 8, dtype=np.uint8)        # bytes past the body are not the body's: never read as zero
    err = sim.wire_sim_unpack(b.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p), C.c_uint64(len(body)), C.c_uint64(n_rec),
                              C.c_int(kind), rec.ctypes.data_as(C.c_void_p), C.c_uint64(words + GUARD))
    assert (rec[words:] == A5).all(), "a word past the last record was written"
    return err, rec[:words]


def sim_pack(sim, kind, shape, recs, room=GUARD):
    """(bytes, body capacity) of records packed: header from the model, table and body from the simulator; the tail past the
    length must still be 0xA5"""
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n_rec = recs.size // W.REC_WORDS[kind]
    count = n_rec * W.INTS[kind]
    bound = n_rec * ((W.BOUND_EXP if kind == 0 else W.BOUND_FORM) - 8 * W.INTS[kind])
    off = np.zeros(max(count, 1), dtype=np.uint64)
    body = np.zeros(bound + room, dtype=np.uint8)
    ln = C.c_uint64()
    rc = sim.wire_sim_pack(recs.ctypes.data_as(C.c_void_p), C.c_uint64(n_rec), C.c_int(kind), off.ctypes.data_as(C.c_void_p),
                           body.ctypes.data_as(C.c_void_p), C.c_uint64(body.size), C.byref(ln))
    assert rc == 0 and ln.value <= bound, "a body above the bound of the width rule"
    assert (body[ln.value:] == 0xA5).all(), "a byte past the length was written"
    return W.header(shape) + off[:count].astype("<u8").tobytes() + body[:ln.value].tobytes()


def test_the_model_by_hand():
    """0 is one zero byte with the flag; 255 has 8 bits and so two bytes, 256 has 9 and two; -1 is the flag on 01; a form with
    b = 0 flags the b alone; decode negates what is flagged; the record of -5 is magnitude 5 and sign word 1"""
    q = lambda *o: b"".join(struct.pack("<Q", x) for x in o)
    h1 = b"\1\0\0\0" + b"\4\0\0\0"
    assert W.encode(0, [4], [0, 255, 256, -1]) == h1 + q(W.FLAG, 1, 3, W.FLAG | 5) + b"\0" + b"\xff\0" + b"\0\1" + b"\1"
    assert W.decode(0, W.encode(0, [4], [0, 255, 256, -1])) == ([4], [0, 255, 256, -1])
    assert W.encode(0, [], [7]) == b"\0\0\0\0" + q(0) + b"\7"
    f = (2, 0, 0x1FF)
    assert W.encode(1, [1], [f]) == b"\1\0\0\0\1\0\0\0" + q(0, W.FLAG | 1, 2) + b"\2" + b"\0" + b"\xff\1"
    assert W.decode(1, W.encode(1, [1], [f])) == ([1], [f])
    two = W.encode(2, [1], [(3, -1, 5), (1, 1, 1 << 16)])
    assert two == b"\1\0\0\0\1\0\0\0" + q(0, W.FLAG | 1, 2, 3, 4, 5) + b"\3\1\5\1\1" + b"\0\0\1"
    assert W.decode(2, two) == ([1], [(3, -1, 5), (1, 1, 1 << 16)])
    flagged_a = b"\1\0\0\0\1\0\0\0" + q(W.FLAG, 1, 2) + b"\2\1\3"
    assert W.decode(1, flagged_a) == ([1], [(-2, 1, 3)]), "the reference's reader negates a flagged a"
    assert [W.slot_width(x) for x in (0, 1, 127, 128, 255, 256, (1 << 992) - 1, (1 << 1280) - 1, (1 << 2560) - 1)] == [1, 1, 1, 2, 2, 2, 125, 161, 321]
    r = W.records(0, [-5, 0])
    assert r[0] == 5 and r[31] == 1 and not r[1:31].any() and not r[32:].any()
    fr = W.records(1, [(3, -1, 5)])
    assert (fr[0], fr[40], fr[80], fr[160]) == (3, 1, 5, 1) and fr.sum() == 10
    assert W.value_of(0, (0, 1)) == 0 and W.arrives_as(0, (0, 1)) == (0, 0) and W.arrives_as(1, (2, 0, 1, 3)) == (2, 0, 0, 3)
    assert W.arrives_as(0, (9, 1)) == (9, 1) and W.value_of(1, (2, 7, 1, 3)) == (2, -7, 3)


def test_the_vectorised_encoder_agrees_with_the_scalar_one():
    """a whole small tensor byte for byte, and 300 sampled elements of a larger one slot by slot"""
    mags, neg, bits = W.exponents_vec(700, 1)
    assert min(bits) < 8 and max(bits) > 984
    vals = W.ints_of_vec(mags, neg, range(700))
    assert [abs(v).bit_length() for v in vals] == bits.tolist()
    assert W.encode_vec([7, 100], mags, neg) == W.encode(0, [7, 100], vals)
    assert np.array_equal(W.records_vec(mags, neg), W.records(0, vals))
    n = 20000
    mags, neg, bits = W.exponents_vec(n, 2)
    data = W.encode_vec([n], mags, neg)
    shape, offs, body = W.split(0, data)
    idx = random.Random(3).sample(range(n - 1), 299) + [n - 1]
    for i, v in zip(idx, W.ints_of_vec(mags, neg, idx)):
        en = (offs[i + 1] & W.M63) if i + 1 < n else len(body)
        one = W.split(0, W.encode(0, [1], [v]))
        assert body[offs[i] & W.M63:en] == one[2] and offs[i] >> 63 == one[1][0] >> 63, i
    assert np.array_equal(W.records_vec(mags, neg).reshape(n, 32)[idx], W.records(0, W.ints_of_vec(mags, neg, idx)).reshape(-1, 32))


@pytest.fixture(scope="module")
def exp_table():
    raws = W.exponent_widths()
    return raws, W.encode(0, [len(raws)], [W.value_of(0, r) for r in raws])


@pytest.fixture(scope="module")
def form_table():
    raws = W.form_widths()
    return raws, W.encode(1, [len(raws)], [W.value_of(1, r) for r in raws])


def test_the_width_tables_hold_every_length(exp_table, form_table):
    raws, data = exp_table
    assert len(raws) == 993 * 3 * 2
    assert {(m.bit_length(), s) for m, s in raws} == {(n, s) for n in range(993) for s in (0, 1)}
    assert W.decode(0, data)[1] == [W.value_of(0, r) for r in raws]
    raws, data = form_table
    assert {r[0].bit_length() for r in raws} == set(range(1, 1281))
    assert {(r[1].bit_length(), r[2]) for r in raws} == {(n, s) for n in range(1281) for s in (0, 1)}
    assert {r[3].bit_length() for r in raws} == set(range(1, 2561))
    assert W.decode(1, data)[1] == [W.value_of(1, r) for r in raws]


def test_every_exponent_width_unpacks_word_for_word(sim, exp_table):
    """records equal to the model's: sign word 1 for a negative value only -- a flagged zero arrives with sign word 0"""
    raws, data = exp_table
    err, rec = sim_unpack(sim, 0, data)
    assert err == 0
    assert np.array_equal(rec, W.raw_records(0, [W.arrives_as(0, r) for r in raws]))
    assert np.array_equal(rec, W.records(0, W.decode(0, data)[1]))


def test_every_form_width_unpacks_word_for_word(sim, form_table):
    """a, |b| and c at every bit length of their planes, the words at the plane edges (39/40, 79/80, 159/160) among them; sign
    word 0 for a flagged zero b; words 161..167 zero"""
    raws, data = form_table
    err, rec = sim_unpack(sim, 1, data)
    assert err == 0
    want = W.raw_records(1, [W.arrives_as(1, r) for r in raws])
    assert np.array_equal(rec, want)
    assert not rec.reshape(-1, 168)[:, 161:].any()
    # the same records as ciphertexts: kind 2 differs in the count only
    err, rec2 = sim_unpack(sim, 2, W.encode(2, [len(raws) // 2], [W.value_of(1, r) for r in raws]))
    assert err == 0 and np.array_equal(rec2, want)


def test_every_exponent_width_packs_byte_for_byte(sim, exp_table):
    """minus zero (sign word 1 on magnitude zero) packs as zero does; no byte past the length is written"""
    raws, data = exp_table
    assert sim_pack(sim, 0, [len(raws)], W.raw_records(0, raws)) == data


def test_every_form_width_packs_byte_for_byte(sim, form_table):
    raws, data = form_table
    recs = W.raw_records(1, raws)
    assert sim_pack(sim, 1, [len(raws)], recs) == data
    assert sim_pack(sim, 2, [3, len(raws) // 6], recs) == W.encode(2, [3, len(raws) // 6], [W.value_of(1, r) for r in raws])
    # words 161..167 and a sign word other than 1 do not reach the bytes
    noisy = recs.reshape(-1, 168).copy()
    noisy[:, 161:] = 0xDEADBEEF
    noisy[noisy[:, 160] != 0, 160] = 0x80000000
    assert sim_pack(sim, 1, [len(raws)], noisy.reshape(-1)) == data


def test_the_size_bound_is_reached_and_never_exceeded(sim, exp_table, form_table):
    """all-maximal records fill 133 and 667 bytes each, table entries included: the figures of the width rule (bits/8 + 1 at
    992, 1280, 1280 and 2560 bits), which cofhe_hip_packed_size_bound must equal; the slot's last byte, one past the plane, is
    written and is zero.  sim_pack asserts the bound for every other case"""
    assert W.BOUND_EXP == 8 + 992 // 8 + 1 == 133 and W.BOUND_FORM == 24 + 2 * (1280 // 8 + 1) + 2560 // 8 + 1 == 667
    for kind, raw, per in ((0, W.MAX_EXP, 133), (1, W.MAX_FORM, 667), (2, W.MAX_FORM, 667)):
        n = 4
        shape = [n] if kind < 2 else [n // 2]
        data = sim_pack(sim, kind, shape, W.raw_records(kind, [raw] * n), room=0)
        assert len(data) == 4 + 4 + n * per
        assert data == W.encode(kind, shape, [W.value_of(kind, raw)] * n)
        assert data[-1] == 0 and data[-2] == 0xFF
        err, rec = sim_unpack(sim, kind, data)
        assert err == 0 and np.array_equal(rec, W.raw_records(kind, [raw] * n))
    # one byte less than the body needs: refused, nothing packed
    recs = W.raw_records(0, [W.MAX_EXP])
    off, body, ln = np.zeros(1, dtype=np.uint64), np.zeros(124, dtype=np.uint8), C.c_uint64()
    assert sim.wire_sim_pack(recs.ctypes.data_as(C.c_void_p), C.c_uint64(1), C.c_int(0), off.ctypes.data_as(C.c_void_p),
                             body.ctypes.data_as(C.c_void_p), C.c_uint64(124), C.byref(ln)) == -1
    assert ln.value == 125 and (body == 0xA5).all()


@pytest.mark.parametrize("kind", [0, 1])
def test_legal_encodings_our_writer_never_produces(sim, kind):
    """padded slots, a last slot that runs on to the end of the buffer, slots without the spare byte, empty slots: the same
    integers to the reference's reader, the same records to ours, and the canonical bytes when packed again"""
    cases = W.legal_cases(kind)
    assert len(cases) >= 10
    for cs in cases:
        shape, vals = W.decode(kind, cs.data)
        assert vals == cs.values, cs.label
        canonical = W.encode(kind, shape, cs.values)
        assert cs.data != canonical, cs.label
        err, rec = sim_unpack(sim, kind, cs.data)
        assert err == 0, cs.label
        assert np.array_equal(rec, W.records(kind, cs.values)), cs.label
        assert sim_pack(sim, kind, shape, rec) == canonical, cs.label


@pytest.mark.parametrize("kind", [0, 1])
def test_every_refusal_reports_its_error_bits(sim, kind):
    """exactly the expected bits: a fault in one integer raises nothing for its neighbours"""
    cases = W.refusal_cases(kind)
    seen = set()
    for cs in cases:
        if cs.bits is None:                  # the host refuses these before a kernel runs (tests/test_gpu_wire.py)
            continue
        err, _ = sim_unpack(sim, kind, cs.data)
        assert err == cs.bits, (cs.label, err)
        seen.add(cs.bits)
    assert seen == ({1, 2} if kind == 0 else {1, 2, 4})
    assert sum(cs.bits is None for cs in cases) == 4


def test_a_flag_on_a_or_c_is_read_as_negative_by_the_reference_and_refused_here(sim):
    """the bytes of (-a, b, c), (a, b, -c) and the negative definite (-a, b, -c): the model's reader negates, ours refuses with
    bit 4; the flag on b keeps its meaning and a flagged zero b is +0"""
    f = (11, 3, 1 << 700)
    base = W._slots(1, [f])
    for flags, want in (((1, 0, 0), (-11, 3, 1 << 700)), ((0, 0, 1), (11, 3, -(1 << 700))), ((1, 0, 1), (-11, 3, -(1 << 700)))):
        data = W.from_slots([1], [(b, bool(fl)) for (b, _), fl in zip(base, flags)])
        assert W.decode(1, data) == ([1], [want])
        assert sim_unpack(sim, 1, data)[0] == W.ERR_AC
    data = W.from_slots([1], [(b, fl) for (b, _), fl in zip(base, (False, True, False))])
    err, rec = sim_unpack(sim, 1, data)
    assert err == 0 and np.array_equal(rec, W.records(1, [(11, -3, 1 << 700)]))
    zb = W._slots(1, [(11, 0, 1 << 700)])
    assert zb[1] == (b"\0", True)
    err, rec = sim_unpack(sim, 1, W.from_slots([1], zb))
    assert err == 0 and rec[160] == 0


def test_the_geometry_is_the_layouts(sim):
    assert [sim.wire_sim_rec_words(k) for k in (0, 1, 2)] == [32, 168, 168]
    assert [sim.wire_sim_ints_per_rec(k) for k in (0, 1, 2)] == [1, 3, 3]
    # one 4-byte group more than the plane: the slot's spare byte
    assert [sim.wire_sim_pack_groups(k) for k in (0, 1, 2)] == [32, 81, 81]
