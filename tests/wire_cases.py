"""The wire format as a plain-Python model, and the case tables shared by the CPU tier (wire.hpp compiled for the host) and the
GPU tier (k_unpack, k_widths, the scan kernels, k_pack behind unpack_tensor_device and pack_tensor_device).  TEST INFRASTRUCTURE.
Imports nothing of cofhe_amd.

The format (wire.hip): u32 ndim; u32 shape[ndim]; u64 off[count]; body.  off[j] is the byte offset of integer j in the body,
bit 63 set when the value is not positive (negative OR zero).  The writer gives integer x a slot of bits/8 + 1 little-endian
magnitude bytes, bits = the bit length of |x| and 1 for zero.  The reader takes each slot's length from the next offset and
the last one's from the buffer size, and negates a value whose flag is set.

kind 0: one integer per element (plaintext exponents); kind 1: one form (a, b, c) per element; kind 2: two forms per element.
`values` are Python integers for kind 0 and (a, b, c) triples, one per RECORD, for kinds 1 and 2.  A raw value is what a
record can hold and an integer cannot: (magnitude, sign word) for kind 0, (a, |b|, sign word, c) for forms -- minus zero is
raw (0, 1)."""
import os
import random
import struct
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import pyref as P  # noqa: E402
import plain_mm_cases as PM  # noqa: E402
import simlib as S  # noqa: E402

FLAG = 1 << 63
M63 = FLAG - 1
INTS = {0: 1, 1: 3, 2: 3}                 # integers per record
REC_WORDS = {0: 32, 1: 168, 2: 168}
EXP_BITS, AB_BITS, C_BITS = 992, 1280, 2560
# the capacity in bytes of the plane of integer `which` of a record
CAP = {0: (124,), 1: (160, 160, 320), 2: (160, 160, 320)}
# per record, from the width rule: 8 table bytes per integer and bits/8 + 1 slot bytes at full plane width
BOUND_EXP = 8 + (EXP_BITS // 8 + 1)                                                    # 133
BOUND_FORM = 3 * 8 + (AB_BITS // 8 + 1) + (AB_BITS // 8 + 1) + (C_BITS // 8 + 1)       # 667
assert (BOUND_EXP, BOUND_FORM) == (133, 667)

MSG_TABLE = "corrupt offset table"
MSG_EXP = "exponent wider than 992 bits"
MSG_RANGE = "form coefficient outside the supported range"
MSG_SHORT = "tensor buffer too short"
ERR_TABLE, ERR_WIDE, ERR_AC = 1, 2, 4     # wire.hpp: WIRE_ERR_*


# ------------------------------------------------------------------------------------------------ the model
def header(shape):
    return struct.pack("<I", len(shape)) + b"".join(struct.pack("<I", d) for d in shape)


def slot_width(x):
    return max(abs(x).bit_length(), 1) // 8 + 1


def elements(shape):
    n = 1
    for d in shape:
        n *= d
    return n


def from_slots(shape, slots, tail=b""):
    """bytes from [(slot bytes, flag)] as they stand: what a writer other than ours may send; tail: bytes after the last slot,
    which the reader counts into it"""
    offs, last = [], 0
    for blob, flag in slots:
        offs.append(last | (FLAG if flag else 0))
        last += len(blob)
    return header(shape) + b"".join(struct.pack("<Q", o) for o in offs) + b"".join(b for b, _ in slots) + tail


def encode(kind, shape, values):
    """the reference's writer.  kinds 1 and 2 go through the oracle's own serialisers"""
    if kind == 0:
        assert elements(shape) == len(values)
        return from_slots(shape, [(abs(v).to_bytes(slot_width(v), "little"), v <= 0) for v in values])
    forms = [P.Form(*v) for v in values]
    assert elements(shape) * kind == len(forms)
    if kind == 1:
        return P.serialize_form_tensor(shape, forms)
    return P.serialize_ciphertext_tensor(shape, list(zip(forms[0::2], forms[1::2])))


def split(kind, data):
    """(shape, [table entries], body) of a well-formed buffer"""
    (ndim,) = struct.unpack_from("<I", data, 0)
    shape = list(struct.unpack_from("<%dI" % ndim, data, 4))
    count = elements(shape) * (1 if kind == 0 else 3 * kind)
    pos = 4 + 4 * ndim
    offs = list(struct.unpack_from("<%dQ" % count, data, pos))
    return shape, offs, data[pos + 8 * count:]


def decode(kind, data):
    """the reference's reader: (shape, values); a set flag negates, so a flagged zero is zero and a flagged a is negative"""
    shape, offs, body = split(kind, data)
    vals = []
    for i, o in enumerate(offs):
        st = o & M63
        en = (offs[i + 1] & M63) if i + 1 < len(offs) else len(body)
        assert st <= en <= len(body)
        v = int.from_bytes(body[st:en], "little")
        vals.append(-v if o >> 63 else v)
    if kind == 0:
        return shape, vals
    return shape, [tuple(vals[i:i + 3]) for i in range(0, len(vals), 3)]


def records(kind, values):
    """the uint32 words of layout.hpp for these values"""
    if kind == 0:
        return PM.exp_records(values)
    return np.concatenate([S.form_record(*v) for v in values]) if len(values) else np.zeros(0, dtype=np.uint32)


def raw_records(kind, raws):
    """records word for word from raw values: any sign word beside any magnitude"""
    if kind == 0:
        out = PM.exp_records([m for m, _ in raws]).reshape(-1, 32)
        out[:, 31] = [s for _, s in raws]
        return out.reshape(-1)
    return np.concatenate([S.raw_record(*r) for r in raws])


def value_of(kind, raw):
    """the integer(s) a raw value travels as: minus zero is zero"""
    if kind == 0:
        return -raw[0] if raw[1] else raw[0]
    a, b, sw, c = raw
    return (a, -b if sw else b, c)


def arrives_as(kind, raw):
    """the raw value that unpacking its bytes gives: the sign word is 1 for a negative value and 0 otherwise"""
    if kind == 0:
        return (raw[0], 1 if raw[1] and raw[0] else 0)
    a, b, sw, c = raw
    return (a, b, 1 if sw and b else 0, c)


# ------------------------------------------------------------------------------------------------ kind 0, vectorised
def exponents_vec(n, seed):
    """n exponents of bit lengths drawn uniformly over 0..992, top bit set, and signs, as (mags uint8 [n, 125] little-endian
    with a zero last column, neg bool [n], bits int64 [n])"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, EXP_BITS + 1, n)
    mags = np.zeros((n, 125), dtype=np.uint8)
    mags[:, :124] = rng.integers(0, 256, (n, 124), dtype=np.uint8)
    top = (bits - 1) // 8                                      # index of the top byte; -1 for zero
    col = np.arange(125)[None, :]
    mags[col > top[:, None]] = 0
    rows = np.nonzero(bits)[0]
    r = (bits[rows] - 1) % 8                                   # position of the top bit in the top byte
    keep = ((1 << (r + 1)) - 1).astype(np.uint8)
    mags[rows, top[rows]] = (mags[rows, top[rows]] & keep) | (1 << r).astype(np.uint8)
    neg = rng.integers(0, 2, n).astype(bool)
    return mags, neg, bits


def ints_of_vec(mags, neg, idx):
    return [(-1 if neg[i] else 1) * int.from_bytes(mags[i].tobytes(), "little") for i in idx]


def bit_lengths_vec(mags):
    nz = mags != 0
    any_nz = nz.any(axis=1)
    top = mags.shape[1] - 1 - np.argmax(nz[:, ::-1], axis=1)
    tb = mags[np.arange(len(mags)), top].astype(np.int64)
    bl = np.zeros(len(mags), dtype=np.int64)
    for k in range(8):
        bl[tb >> k != 0] = k + 1
    return np.where(any_nz, top * 8 + bl, 0)


def encode_vec(shape, mags, neg):
    """encode(0, ...) over arrays: widths from the bit lengths, offsets from one cumulative sum, the body one masked copy"""
    n = len(mags)
    assert elements(shape) == n
    bits = bit_lengths_vec(mags)
    width = np.maximum(bits, 1) // 8 + 1
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(width)[:-1].astype(np.uint64)
    off |= np.where(neg | (bits == 0), np.uint64(FLAG), np.uint64(0)).astype(np.uint64)
    body = mags[np.arange(mags.shape[1])[None, :] < width[:, None]]
    return header(shape) + off.astype("<u8").tobytes() + body.tobytes()


def records_vec(mags, neg):
    n = len(mags)
    out = np.zeros((n, 128), dtype=np.uint8)
    out[:, :124] = mags[:, :124]
    out = out.view("<u4").reshape(n, 32).copy()
    out[:, 31] = (neg & mags.any(axis=1)).astype(np.uint32)
    return out.reshape(-1)


# ------------------------------------------------------------------------------------------------ widths
def _three(n, rng):
    """2^(n-1), 2^n - 1 and a random value with the top bit set; zero three times for n = 0"""
    if n == 0:
        return [0, 0, 0]
    return [1 << (n - 1), (1 << n) - 1, (1 << (n - 1)) | rng.getrandbits(n - 1) if n > 1 else 1]


def exponent_widths():
    """raw kind-0 values: every bit length 0..992, three values each, sign word clear and set (minus zero among them)"""
    rng = random.Random(992)
    out = []
    for n in range(EXP_BITS + 1):
        for v in _three(n, rng):
            out += [(v, 0), (v, 1)]
    return out


def form_widths():
    """raw form records, not reduced forms: record i of each of the three value families has an a of i mod 1280 + 1 bits, a |b|
    of i mod 1281 bits with sign word i div 1281 (so |b| = 0 comes with sign word 1 too: minus zero) and a c of i mod 2560 + 1
    bits; 2562 lengths, so a and |b| see every length twice and c every length once"""
    rng = random.Random(2560)
    out = []
    for i in range(2 * (AB_BITS + 1)):
        a3, b3, c3 = _three(i % AB_BITS + 1, rng), _three(i % (AB_BITS + 1), rng), _three(i % C_BITS + 1, rng)
        out += [(a3[k], b3[k], i // (AB_BITS + 1), c3[k]) for k in range(3)]
    return out


MAX_EXP = ((1 << EXP_BITS) - 1, 1)
MAX_FORM = ((1 << AB_BITS) - 1, (1 << AB_BITS) - 1, 1, (1 << C_BITS) - 1)


# ------------------------------------------------------------------------------------------------ non-canonical but legal
Legal = namedtuple("Legal", "label kind data values")       # values: what both readers must see


def _slots(kind, values):
    flat = values if kind == 0 else [x for v in values for x in v]
    return [(abs(x).to_bytes(slot_width(x), "little"), x <= 0) for x in flat]


def legal_cases(kind):
    """encodings our writer never produces and every reader takes; kind 0 or 1 (two records each, so that a slot in the middle
    and the last slot are both seen)"""
    rng = random.Random(77 + kind)
    if kind == 0:
        vals = [-((1 << 991) | rng.getrandbits(991)), (1 << 500) + 3]
    else:
        vals = [((1 << 1279) | rng.getrandbits(1279), -((1 << 1279) | rng.getrandbits(1200)), (1 << 2559) | rng.getrandbits(2559)),
                (5, -3, (1 << 2559) + 9)]
    shape = [len(vals)]
    base = _slots(kind, vals)
    caps = [CAP[kind][j % INTS[kind]] for j in range(len(base))]
    out = []

    # zero bytes on top of every slot: one, up to the plane, up to plane + 3 (the all-zero top word group), far beyond
    for label, length in (("pad1", lambda b, cap: len(b) + 1), ("pad_to_plane", lambda b, cap: cap), ("pad_to_plane_plus_3", lambda b, cap: cap + 3),
                          ("pad_far_beyond", lambda b, cap: 2 * cap + 301)):
        slots = [(b + bytes(max(length(b, cap) - len(b), 0)), f) for (b, f), cap in zip(base, caps)]
        out.append(Legal(label, kind, from_slots(shape, slots), vals))
    for tail in (1, 7, 400):
        out.append(Legal("last_slot_runs_on_%d" % tail, kind, from_slots(shape, base, tail=bytes(tail)), vals))
    # the magnitude cut to its significant bytes: no slot has the writer's spare byte (one cut to one byte where it is a zero byte)
    trimmed = [(b.rstrip(b"\0") or b"\0", f) for b, f in base]
    out.append(Legal("no_spare_byte", kind, from_slots(shape, trimmed), vals))
    # a zero-length slot reads as zero: for b and for an exponent, with and without the flag, in the middle and at the end
    for flag in (False, True):
        if kind == 0:
            zs, zv = [base[0], (b"", flag)], [vals[0], 0]
            out.append(Legal("empty_slot_last_flag%d" % flag, kind, from_slots(shape, zs), zv))
            zs, zv = [(b"", flag), base[1]], [0, vals[1]]
            out.append(Legal("empty_slot_first_flag%d" % flag, kind, from_slots(shape, zs), zv))
        else:
            zs = list(base)
            zs[1] = zs[4] = (b"", flag)
            zv = [(vals[0][0], 0, vals[0][2]), (vals[1][0], 0, vals[1][2])]
            out.append(Legal("empty_b_flag%d" % flag, kind, from_slots(shape, zs), zv))
    return out


# ------------------------------------------------------------------------------------------------ refusals
# bits: the err word of the unpack body (None: the host refuses before any kernel runs); message: what the library says
Refusal = namedtuple("Refusal", "label kind data bits message")


def refusal_cases(kind):
    """kind 0 or 1.  One fault each, in the first or the second of two records, the other integers as in a valid tensor"""
    rng = random.Random(55 + kind)
    wide_msg = MSG_EXP if kind == 0 else MSG_RANGE
    if kind == 0:
        vals = [(1 << 700) | rng.getrandbits(700), -12345]
    else:
        vals = [((1 << 300) | rng.getrandbits(300), -((1 << 200) | rng.getrandbits(200)), (1 << 600) | rng.getrandbits(600)), (7, 3, 11)]
    shape = [len(vals)]
    base = _slots(kind, vals)
    n_int = len(base)
    out = []

    def with_slot(j, blob, flag=None):
        s = list(base)
        s[j] = (blob, s[j][1] if flag is None else flag)
        return from_slots(shape, s)

    # a non-zero byte just above the plane (cap * 8 + 1 bits) and at the last byte of an over-long slot whose other high bytes
    # are zero, in a middle slot and in the last one
    for j in range(n_int):
        cap = CAP[kind][j % INTS[kind]]
        low = base[j][0].rstrip(b"\0") or b"\1"
        low = low + bytes(cap - len(low))
        out.append(Refusal("bit_%d_slot%d" % (8 * cap + 1, j), kind, with_slot(j, low + b"\1"), ERR_WIDE, wide_msg))
        out.append(Refusal("last_byte_of_long_slot%d" % j, kind, with_slot(j, low + bytes(40) + b"\x80"), ERR_WIDE, wide_msg))
    if kind != 0:
        for j, name in ((0, "a"), (2, "c"), (3, "a2"), (5, "c2")):
            out.append(Refusal("%s_zero_bytes" % name, kind, with_slot(j, bytes(3), False), ERR_AC, MSG_RANGE))
            out.append(Refusal("%s_zero_flagged" % name, kind, with_slot(j, bytes(1), True), ERR_AC, MSG_RANGE))
            out.append(Refusal("%s_empty_slot" % name, kind, with_slot(j, b"", False), ERR_AC, MSG_RANGE))
            out.append(Refusal("%s_flagged" % name, kind, with_slot(j, base[j][0], True), ERR_AC, MSG_RANGE))
        s = list(base)
        s[0], s[2] = (s[0][0], True), (s[2][0], True)
        out.append(Refusal("a_and_c_flagged", kind, from_slots(shape, s), ERR_AC, MSG_RANGE))
    good = from_slots(shape, base)
    tab = 4 + 4 * len(shape)
    body_len = len(good) - tab - 8 * n_int

    def with_offset(j, o):
        b = bytearray(good)
        struct.pack_into("<Q", b, tab + 8 * j, o)
        return bytes(b)

    last = n_int - 1
    out.append(Refusal("offset_beyond_body", kind, with_offset(last, body_len + 1), ERR_TABLE, MSG_TABLE))
    out.append(Refusal("offset_far_beyond_body_flagged", kind, with_offset(last, FLAG | (1 << 40)), ERR_TABLE, MSG_TABLE))
    out.append(Refusal("offset_2_63_minus_1", kind, with_offset(last, M63), ERR_TABLE, MSG_TABLE))
    out.append(Refusal("offset_2_63_minus_1_first_but_one", kind, with_offset(1, M63), ERR_TABLE, MSG_TABLE))
    # the values are small enough that the slot which swallows its neighbours still fits its plane: bit 1 alone
    if kind != 0:
        out.append(Refusal("offsets_decrease", kind, with_offset(2, 0), ERR_TABLE, MSG_TABLE))
    else:
        out.append(Refusal("offsets_decrease", kind, _swap_offsets(from_slots([3], base + [base[0]]), 4 + 4, 1, 2), ERR_TABLE, MSG_TABLE))
    out.append(Refusal("table_cut_short", kind, good[:tab + 8 * n_int - 1], None, MSG_SHORT))
    out.append(Refusal("shape_cut_short", kind, good[:tab - 1], None, MSG_SHORT))
    out.append(Refusal("three_bytes", kind, good[:3], None, MSG_SHORT))
    out.append(Refusal("no_bytes", kind, b"", None, MSG_SHORT))
    return out


def _swap_offsets(data, tab, i, j):
    b = bytearray(data)
    oi, oj = struct.unpack_from("<Q", b, tab + 8 * i)[0], struct.unpack_from("<Q", b, tab + 8 * j)[0]
    struct.pack_into("<Q", b, tab + 8 * i, oj)
    struct.pack_into("<Q", b, tab + 8 * j, oi)
    return bytes(b)


# ------------------------------------------------------------------------------------------------ headers
RANK_SHAPES = {0: [], 1: [6], 2: [2, 3], 3: [1, 2, 3], 4: [1, 3, 1, 2], 5: [1, 1, 6, 1, 1], 6: [3, 1, 1, 1, 1, 2], 7: [1, 2, 1, 1, 3, 1, 1],
               8: [1, 1, 1, 1, 1, 1, 1, 2]}
ZERO_SHAPES = ([0], [3, 0])
TOO_LARGE = [1 << 21, 1 << 21]
BAD_KINDS = (-1, 3)
MSG_RANK, MSG_LARGE, MSG_KIND = "tensor rank above 8", "tensor too large", "kind must be 0"
MSG_COUNT, MSG_OUT_SMALL, MSG_REC_SMALL = "shape does not match the record count", "output buffer too small", "record buffer too small"
