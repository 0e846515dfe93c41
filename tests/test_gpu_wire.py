"""The wire format on the GPU (k_unpack, k_widths, k_tile_sums, k_scan_tiles, k_offsets, k_pack behind unpack_tensor_device and
pack_tensor_device) against the plain-Python model of wire_cases: every slot width, unwritten bytes (every output starts as
0xA5), the tile edges and the second pass of the offset scan, unaligned buffers, every rank, the refusals each with its
message, and the flag on a and c.

unpack_tensor_device validates forms, so arbitrary widths reach k_unpack for kind 0 only (forms at arbitrary widths:
tests/test_wire_cpu.py, the same body on the host); pack_tensor_device does not validate, so forms of every width are packed.
Flagged bytes go to unpack_tensor_device first, then to the host reader, and to an arithmetic entry point only after both
have refused them in the same test."""
import ctypes as C
import struct
import time

import numpy as np
import pytest

import wire_cases as W
from gpu_inputs import P, _device_status_stays_clear, _random_tensor, engine, hx  # noqa: F401

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def E(params128):
    return engine(hx(params128["delta"]))


@pytest.fixture(scope="module")
def valid_cts(params128):
    """343 valid ciphertexts: 2058 integers, just past one tile of the scan"""
    return _random_tensor(hx(params128["delta"]), 343, 1515)


def forms_of(cts):
    return [(f.a, f.b, f.c) for ct in cts for f in ct]


def a5(torch, nbytes):
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")


def put(torch, data, shift=0):
    """the bytes at `shift` from an aligned allocation, 0xA5 around them; returns (owner, device address)"""
    buf = a5(torch, shift + len(data) + GUARD)
    assert buf.data_ptr() % 256 == 0
    if len(data):
        buf[shift:shift + len(data)] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy())
    return buf, buf.data_ptr() + shift


def unpack(torch, E, kind, data, shift=0, n_rec=None, capacity=None):
    """(shape, records) through unpack_tensor_device; the words past the last record must still be 0xA5"""
    if n_rec is None:
        n_rec = len(W.split(kind, data)[1]) // W.INTS[kind]
    words = n_rec * W.REC_WORDS[kind]
    rec = a5(torch, 4 * words + GUARD)
    own, ptr = put(torch, data, shift)
    shape, n = E.unpack_tensor_device(ptr, len(data), kind, rec.data_ptr(), n_rec if capacity is None else capacity)
    assert n == n_rec
    got = rec.cpu().numpy()
    assert (got[4 * words:] == 0xA5).all(), "a word past the last record was written"
    return shape, got[:4 * words].view(np.uint32)


def pack(torch, E, kind, shape, recs, shift=0):
    """the bytes through pack_tensor_device with capacity = the size bound; every byte around them must still be 0xA5"""
    recs = np.ascontiguousarray(recs, dtype=np.uint32)
    n_rec = recs.size // W.REC_WORDS[kind]
    d_rec = torch.from_numpy(recs.view(np.int32)).cuda() if recs.size else torch.zeros(1, dtype=torch.int32, device="cuda")
    cap = E.packed_size_bound(n_rec, kind, len(shape))
    assert cap == 4 + 4 * len(shape) + n_rec * (W.BOUND_EXP if kind == 0 else W.BOUND_FORM)
    out = a5(torch, shift + cap + GUARD)
    ln = E.pack_tensor_device(d_rec.data_ptr(), n_rec, kind, shape, out.data_ptr() + shift, cap)
    assert ln <= cap
    got = out.cpu().numpy()
    assert (got[:shift] == 0xA5).all() and (got[shift + ln:] == 0xA5).all(), "a byte outside the tensor was written"
    return got[shift:shift + ln].tobytes()


def raw_pack(E, d_rec, n_rec, kind, shape, d_out, capacity, ndim=None):
    """pack_tensor_device without the wrapper's exception: (return code, *len as the call left it, message)"""
    sh = (C.c_uint32 * max(len(shape), 1))(*shape)
    ln = C.c_size_t(0xDEAD)
    rc = E.L.cofhe_hip_pack_tensor_device(E.ctx, C.c_void_p(d_rec), C.c_uint64(n_rec), C.c_int(kind), C.c_uint32(len(shape) if ndim is None else ndim),
                                          sh, C.c_void_p(d_out), C.c_size_t(capacity), C.byref(ln), C.c_void_p(0))
    return rc, ln.value, E.L.cofhe_hip_last_error().decode() if rc else ""


def test_every_exponent_width(E):
    """kind 0 at every bit length 0..992, three values each, sign word clear and set: the records and the bytes of the model;
    minus zero packs as zero and arrives as +0"""
    import torch
    raws = W.exponent_widths()
    data = W.encode(0, [len(raws)], [W.value_of(0, r) for r in raws])
    shape, rec = unpack(torch, E, 0, data)
    assert shape == [len(raws)]
    assert np.array_equal(rec, W.raw_records(0, [W.arrives_as(0, r) for r in raws]))
    assert pack(torch, E, 0, [len(raws)], W.raw_records(0, raws)) == data
    assert E.device_status(clear=False) == 0


def test_exponent_encodings_our_writer_never_produces(E):
    import torch
    for cs in W.legal_cases(0):
        shape, rec = unpack(torch, E, 0, cs.data)
        assert np.array_equal(rec, W.records(0, cs.values)), cs.label
        assert pack(torch, E, 0, shape, rec) == W.encode(0, shape, cs.values), cs.label
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_every_refusal_by_its_message(E, kind):
    """the refusals of wire_cases, each with the message it names; the error bits are judged before the form gate, so the
    kind-1 cases need no valid forms.  The host reader gives the same answer for the same bytes"""
    import torch
    from cofhe_amd import CofheHipError
    host = E.bytes_to_exponents if kind == 0 else E.pdr_bytes_to_records
    for cs in W.refusal_cases(kind):
        own, ptr = put(torch, cs.data)
        rec = a5(torch, 4 * 3 * W.REC_WORDS[kind])
        with pytest.raises(CofheHipError, match=cs.message):
            E.unpack_tensor_device(ptr, len(cs.data), kind, rec.data_ptr(), 3)
        with pytest.raises(CofheHipError, match=cs.message):
            host(cs.data)
    assert E.device_status(clear=False) == 0


def test_every_form_width_packs_byte_for_byte(E):
    """a and |b| at every bit length up to 1280, c up to 2560, b of either sign word and minus zero: 7686 records, 23058
    integers, 12 tiles of the scan.  Bytes equal to the model's; an all-maximal tensor is exactly as long as the bound"""
    import torch
    raws = W.form_widths()
    n = len(raws)
    vals = [W.value_of(1, r) for r in raws]
    recs = W.raw_records(1, raws)
    assert pack(torch, E, 1, [n], recs) == W.encode(1, [n], vals)
    assert pack(torch, E, 2, [n // 2], recs) == W.encode(2, [n // 2], vals)
    for kind, raw, shape in ((0, W.MAX_EXP, [2, 2]), (1, W.MAX_FORM, [4]), (2, W.MAX_FORM, [2])):
        data = pack(torch, E, kind, shape, W.raw_records(kind, [raw] * 4))
        assert len(data) == E.packed_size_bound(4, kind, len(shape))
        assert data == W.encode(kind, shape, [W.value_of(kind, raw)] * 4)
    assert E.device_status(clear=False) == 0


TILE_EDGE_SHAPES = {341: ([341], [11, 31], [1, 11, 31], [11, 1, 31, 1]), 342: ([342], [18, 19], [2, 9, 19], [2, 3, 3, 19]),
                    343: ([343], [7, 49], [7, 7, 7], [7, 7, 7, 1])}


@pytest.mark.parametrize("n", [341, 342, 343])
def test_valid_ciphertexts_at_the_tile_edge_every_rank_every_alignment(E, valid_cts, n):
    """2046, 2052 and 2058 integers (one tile of the scan is 2048, no multiple of 6) at ranks 1 to 4, and one ciphertext at
    rank 0; the buffer at 0, 1, 4 and 7 bytes from an aligned address, so the offset table is 8-byte aligned or not whatever
    the rank.  Records and bytes equal to the model's, which makes every alignment identical to the aligned case"""
    import torch
    for cts, shapes in ((valid_cts[:n], TILE_EDGE_SHAPES[n]), (valid_cts[n - 1:n], ([],))):
        vals = forms_of(cts)
        want = W.records(2, vals)
        for shape in shapes:
            data = W.encode(2, shape, vals)
            for shift in (0, 1, 4, 7):
                got_shape, rec = unpack(torch, E, 2, data, shift)
                assert got_shape == shape and np.array_equal(rec, want), (shape, shift)
                assert pack(torch, E, 2, shape, want, shift) == data, (shape, shift)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("n", [2047, 2048, 2049, 4097])
def test_the_scan_at_its_tile_edges(E, n):
    """kind 0, widths uniform over 0..992 bits: one tile less one, one tile, one tile and one, two tiles and one"""
    import torch
    mags, neg, _ = W.exponents_vec(n, n)
    data, recs = W.encode_vec([n], mags, neg), W.records_vec(mags, neg)
    assert pack(torch, E, 0, [n], recs) == data
    assert np.array_equal(unpack(torch, E, 0, data)[1], recs)
    assert E.device_status(clear=False) == 0


def test_the_scan_takes_a_second_pass(E):
    """524 289 integers = 257 tiles: k_scan_tiles scans 256 tile sums per pass and carries the running sum into the next, so
    this is the smallest tensor whose last tile's base depends on the carry.  Widths uniform over 0..992 bits from a fixed
    seed: all tile sums differ, and a lost carry moves every offset of tile 256.  The whole offset table and the whole body
    are compared with the vectorised model (which test_wire_cpu.py holds to the scalar one), then the bytes are unpacked to
    the same records.  The body is 33 MB; bodies beyond 4 GiB are out of scope here.  Most of the time is the host's: making
    67 MB of records and comparing 37 MB of bytes"""
    import torch
    n = 256 * 2048 + 1
    t0 = time.time()
    mags, neg, _ = W.exponents_vec(n, 257)
    data, recs = W.encode_vec([n], mags, neg), W.records_vec(mags, neg)
    t1 = time.time()
    d_rec = torch.from_numpy(recs.view(np.int32)).cuda()
    cap = E.packed_size_bound(n, 0, 1)
    out = a5(torch, cap + GUARD)
    ln = E.pack_tensor_device(d_rec.data_ptr(), n, 0, [n], out.data_ptr(), cap)
    torch.cuda.synchronize()
    t2 = time.time()
    assert ln == len(data)
    got = out.cpu().numpy()
    tab = 8 + 8 * n
    assert got[:8].tobytes() == data[:8]
    want = np.frombuffer(data, dtype=np.uint8)
    assert np.array_equal(got[8:tab].view("<u8"), want[8:tab].view("<u8")), "the offset table"
    assert np.array_equal(got[tab:ln], want[tab:]), "the body"
    assert (got[ln:] == 0xA5).all()
    rec = a5(torch, 4 * 32 * n + GUARD)
    shape, cnt = E.unpack_tensor_device(out.data_ptr(), ln, 0, rec.data_ptr(), n)
    assert (shape, cnt) == ([n], n)
    back = rec.cpu().numpy()
    assert np.array_equal(back[:4 * 32 * n].view(np.uint32), recs) and (back[4 * 32 * n:] == 0xA5).all()
    print("second pass of the scan: %.2f s making the case on the host, %.2f s upload + pack, %.2f s in all" % (t1 - t0, t2 - t1, time.time() - t0))
    assert E.device_status(clear=False) == 0


def test_a_flag_on_a_or_c_is_refused(E, valid_cts):
    """bit 63 set in the table entry of c1.a, c1.c, c2.a, c2.c, and of a and c together: the reference's reader would negate
    them, which is no form of this class group; refused by unpack_tensor_device, by the host reader, and only then by an
    arithmetic entry point.  The same flag on b is the form's inverse, which is taken"""
    import torch
    from cofhe_amd import CofheHipError
    ct = valid_cts[5]
    vals = forms_of([ct])
    good = W.encode(2, [1], vals)
    rec = a5(torch, 4 * 2 * 168)
    for which in ((0,), (2,), (3,), (5,), (0, 2)):
        bad = bytearray(good)
        for j in which:
            (o,) = struct.unpack_from("<Q", bad, 8 + 8 * j)
            assert o >> 63 == 0
            struct.pack_into("<Q", bad, 8 + 8 * j, o | W.FLAG)
        bad = bytes(bad)
        read = W.decode(2, bad)[1]
        assert all(read[j // 3][j % 3] == -vals[j // 3][j % 3] < 0 for j in which)
        own, ptr = put(torch, bad)
        with pytest.raises(CofheHipError, match=W.MSG_RANGE):
            E.unpack_tensor_device(ptr, len(bad), 2, rec.data_ptr(), 2)
        with pytest.raises(CofheHipError, match=W.MSG_RANGE):
            E.bytes_to_records(bad)
        with pytest.raises(CofheHipError, match=W.MSG_RANGE):
            E.add_ciphertext_tensors(bad, good)
        with pytest.raises(CofheHipError, match=W.MSG_RANGE):
            E.add_ciphertext_tensors(good, bad)
    (a, b, c), second = vals
    if 0 < b < a < c:
        inv = W.encode(2, [1], [(a, -b, c), second])
        assert np.array_equal(unpack(torch, E, 2, inv)[1], W.records(2, [(a, -b, c), second]))
    assert unpack(torch, E, 2, good)[0] == [1]
    assert E.device_status(clear=False) == 0


def test_every_rank_both_ways(E, valid_cts):
    """ranks 0 to 8 for kind 0 and kind 2: at every even rank the offset table is 4 bytes off alignment and goes through an
    aligned copy.  Rank 9 is refused both ways"""
    import torch
    from cofhe_amd import CofheHipError
    for rank, shape in W.RANK_SHAPES.items():
        assert len(shape) == rank
        n = W.elements(shape)
        vals = [(-1) ** i * ((1 << (97 * i)) + i) for i in range(n)]
        data = W.encode(0, shape, vals)
        got_shape, rec = unpack(torch, E, 0, data)
        assert got_shape == shape and np.array_equal(rec, W.records(0, vals)), shape
        assert pack(torch, E, 0, shape, rec) == data, shape
        fv = forms_of(valid_cts[10:10 + n])
        data = W.encode(2, shape, fv)
        got_shape, rec = unpack(torch, E, 2, data)
        assert got_shape == shape and np.array_equal(rec, W.records(2, fv)), shape
        assert pack(torch, E, 2, shape, rec) == data, shape
    nine = W.header([1] * 9) + struct.pack("<Q", 0) + b"\1"
    own, ptr = put(torch, nine)
    rec = a5(torch, 4 * 168)
    with pytest.raises(CofheHipError, match=W.MSG_RANK):
        E.unpack_tensor_device(ptr, len(nine), 0, rec.data_ptr(), 1)
    out = a5(torch, 512)
    rc, _, msg = raw_pack(E, rec.data_ptr(), 1, 0, [1] * 9, out.data_ptr(), 512)
    assert rc != 0 and W.MSG_RANK in msg
    assert (rec.cpu().numpy() == 0xA5).all() and (out.cpu().numpy() == 0xA5).all()
    assert E.device_status(clear=False) == 0


def test_zero_sized_too_large_and_kinds_out_of_range(E):
    """[0] and [3, 0]: the header alone, len = 4 + 4 ndim, no record written; [2^21, 2^21] is too large; kind -1 and 3"""
    import torch
    from cofhe_amd import CofheHipError
    rec = a5(torch, 4 * 168 * 2)
    for kind in (0, 1, 2):
        for shape in W.ZERO_SHAPES:
            hl = 4 + 4 * len(shape)
            out = a5(torch, 64)
            rc, ln, msg = raw_pack(E, rec.data_ptr(), 0, kind, shape, out.data_ptr(), hl)
            assert (rc, ln) == (0, hl), msg
            got = out.cpu().numpy()
            assert got[:hl].tobytes() == W.header(shape) and (got[hl:] == 0xA5).all()
            rc, _, msg = raw_pack(E, rec.data_ptr(), 0, kind, shape, out.data_ptr(), hl - 1)
            assert rc != 0 and W.MSG_OUT_SMALL in msg
            assert E.unpack_tensor_device(out.data_ptr(), hl, kind, rec.data_ptr(), 0) == (shape, 0)
            assert E.unpack_tensor_device(out.data_ptr(), hl + 9, kind, rec.data_ptr(), 2) == (shape, 0)
            with pytest.raises(CofheHipError, match=W.MSG_SHORT):
                E.unpack_tensor_device(out.data_ptr(), hl - 1, kind, rec.data_ptr(), 2)
        big = W.header(W.TOO_LARGE)
        own, ptr = put(torch, big)
        with pytest.raises(CofheHipError, match=W.MSG_LARGE):
            E.unpack_tensor_device(ptr, len(big), kind, rec.data_ptr(), 2)
        out = a5(torch, 64)
        rc, _, msg = raw_pack(E, rec.data_ptr(), 1, kind, W.TOO_LARGE, out.data_ptr(), 64)
        assert rc != 0 and W.MSG_LARGE in msg and (out.cpu().numpy() == 0xA5).all()
    one = W.encode(0, [1], [5])
    own, ptr = put(torch, one)
    for kind in W.BAD_KINDS:
        with pytest.raises(CofheHipError, match=W.MSG_KIND):
            E.unpack_tensor_device(ptr, len(one), kind, rec.data_ptr(), 2)
        out = a5(torch, 64)
        rc, _, msg = raw_pack(E, rec.data_ptr(), 1, kind, [1], out.data_ptr(), 64)
        assert rc != 0 and W.MSG_KIND in msg and (out.cpu().numpy() == 0xA5).all()
    assert (rec.cpu().numpy() == 0xA5).all(), "no call of this test may write a record"
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("kind", [0, 2])
def test_capacities(E, valid_cts, kind):
    """capacity = len succeeds; len - 1 fails with the needed length reported and no body byte written; a capacity below the
    header fails; a shape that does not match the record count; a record buffer one record short"""
    import torch
    from cofhe_amd import CofheHipError
    shape = [2, 3]
    vals = [3, -(1 << 991), 0, 255, 256, -1] if kind == 0 else forms_of(valid_cts[20:26])
    data = W.encode(kind, shape, vals)
    recs = W.records(kind, vals)
    n_rec = recs.size // W.REC_WORDS[kind]
    hl = 4 + 4 * 2 + 8 * n_rec * W.INTS[kind]
    d_rec = torch.from_numpy(recs.view(np.int32)).cuda()
    out = a5(torch, len(data) + GUARD)
    rc, ln, msg = raw_pack(E, d_rec.data_ptr(), n_rec, kind, shape, out.data_ptr(), len(data))
    assert (rc, ln) == (0, len(data)), msg
    got = out.cpu().numpy()
    assert got[:ln].tobytes() == data and (got[ln:] == 0xA5).all()
    for cap in (len(data) - 1, hl):
        out = a5(torch, len(data) + GUARD)
        rc, ln, msg = raw_pack(E, d_rec.data_ptr(), n_rec, kind, shape, out.data_ptr(), cap)
        assert rc != 0 and W.MSG_OUT_SMALL in msg and ln == len(data), (cap, ln, msg)
        assert (out.cpu().numpy()[hl:] == 0xA5).all(), "no body byte without room for the body"
    for cap in (hl - 1, 11, 0):
        out = a5(torch, len(data) + GUARD)
        rc, _, msg = raw_pack(E, d_rec.data_ptr(), n_rec, kind, shape, out.data_ptr(), cap)
        assert rc != 0 and W.MSG_OUT_SMALL in msg and (out.cpu().numpy() == 0xA5).all(), cap
    for bad_shape in ([2, 2], [7], [], [6, 0]):
        out = a5(torch, len(data) + GUARD)
        rc, _, msg = raw_pack(E, d_rec.data_ptr(), n_rec, kind, bad_shape, out.data_ptr(), len(data))
        assert rc != 0 and W.MSG_COUNT in msg and (out.cpu().numpy() == 0xA5).all(), bad_shape
    own, ptr = put(torch, data)
    rec = a5(torch, 4 * recs.size)
    with pytest.raises(CofheHipError, match=W.MSG_REC_SMALL):
        E.unpack_tensor_device(ptr, len(data), kind, rec.data_ptr(), n_rec - 1)
    assert (rec.cpu().numpy() == 0xA5).all()
    assert np.array_equal(unpack(torch, E, kind, data)[1], recs)
    assert E.device_status(clear=False) == 0
