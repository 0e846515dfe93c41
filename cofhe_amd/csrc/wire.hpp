// wire.hpp -- the per-thread bodies of k_unpack, k_widths and k_pack (wire.hip): the reference's binary tensor format read
// into records and written from them, in a header so that the host build of the CPU tests (tests/hostsim/wire_sim.cpp,
// COFHE_HOSTSIM) compiles the very code the kernels run.  Each body is one function of the thread's linear index; the kernels
// are index computation plus a call.  The prefix sum between k_widths and k_pack (three scan kernels) stays in wire.hip.
//
// An integer of the format is a slot of little-endian magnitude bytes and one 64-bit table entry: the slot's byte offset, bit
// 63 set when the value is not positive.  The writer gives a slot bits/8 + 1 bytes (bits = 1 for zero), so a slot is one byte
// longer than the magnitude at every multiple of 8 bits, and one byte longer than the whole limb plane at full plane width.
// The reader takes any length: missing bytes are zero, bytes beyond the plane must be zero.
//
// The flag means "negative" only where a negative value exists: on b of a form and on an exponent, where a flagged zero is
// the reference's spelling of zero and reads as +0.  a and c of a form are positive: a flagged zero is refused as zero, and a
// flag on a non-zero a or c -- which the reference's reader would negate into no form of a negative discriminant's class
// group -- is refused too, so that one ciphertext has one spelling.
#pragma once
#include <stdint.h>

#include "layout.hpp"

#if defined(COFHE_HOSTSIM)
#define WIRE_DEV inline
#define WIRE_HD inline
#define WIRE_CLZ(v) __builtin_clz(v)
#else
#include <hip/hip_runtime.h>
#define WIRE_DEV __device__ inline
#define WIRE_HD __host__ __device__ inline
#define WIRE_CLZ(v) __clz(v)
#endif

namespace cofhe {

constexpr uint64_t WIRE_OFFMASK = ~(1ull << 63);
constexpr int WIRE_EXP_MAG_WORDS = 31, WIRE_EXP_REC_WORDS = 32;      // exponent records (qf.hpp)
// err bits of the unpack body
constexpr uint32_t WIRE_ERR_TABLE = 1;       // corrupt offset table
constexpr uint32_t WIRE_ERR_WIDE = 2;        // value wider than its limb plane
constexpr uint32_t WIRE_ERR_AC = 4;          // a or c of a form is zero, or carries the flag

// kind 2 / 1: forms, 2 or 1 per element (3 integers each); kind 0: plaintext exponents (1 integer)
struct Geometry {
    int ints_per_rec;      // integers per destination record: 3 (a, b, c) or 1
    int rec_words;         // 168 or 32
};
WIRE_HD Geometry geometry(int kind) { return kind == 0 ? Geometry{1, WIRE_EXP_REC_WORDS} : Geometry{3, REC_WORDS}; }

// destination of integer `which` of a record: first word, capacity in words
WIRE_DEV void slot_of(int kind, int which, int &first, int &cap) {
    if (kind == 0) {
        first = 0;
        cap = WIRE_EXP_MAG_WORDS;
    } else if (which == 0) {
        first = REC_A;
        cap = 40;
    } else if (which == 1) {
        first = REC_B;
        cap = 40;
    } else {
        first = REC_C;
        cap = 80;
    }
}

WIRE_DEV void int_span(const uint64_t *__restrict__ off, uint64_t idx, uint64_t count, uint64_t body_len, uint64_t &st, uint64_t &en,
                       bool &flag) {
    const uint64_t o = off[idx];
    st = o & WIRE_OFFMASK;
    flag = (o >> 63) != 0;
    en = idx + 1 < count ? (off[idx + 1] & WIRE_OFFMASK) : body_len;
}

// k_unpack, thread tid = destination word tid of the record array: the word to store (when `store`) and the err bits to OR
struct UnpackWord {
    uint32_t val, err;
    bool store;
};
WIRE_DEV UnpackWord wire_unpack_word(const uint8_t *__restrict__ body, const uint64_t *__restrict__ off, uint64_t body_len, uint64_t n_rec,
                                     int kind, uint64_t tid) {
    const Geometry gm = geometry(kind);
    const uint64_t r = tid / gm.rec_words;
    const int w = (int)(tid % gm.rec_words);
    if (r >= n_rec) return UnpackWord{0u, 0u, false};
    const uint64_t count = n_rec * gm.ints_per_rec;
    const int sign_word = kind == 0 ? WIRE_EXP_MAG_WORDS : REC_SIGN;
    uint32_t val = 0, err = 0;
    if (w == sign_word) {
        // sign of b (forms) / of the exponent: the flag also marks zero, which is not negative
        const uint64_t idx = r * gm.ints_per_rec + (kind == 0 ? 0 : 1);
        uint64_t st, en;
        bool flag;
        int_span(off, idx, count, body_len, st, en, flag);
        bool nonzero = false;
        if (flag && st <= en && en <= body_len)
            for (uint64_t i = st; i < en; i++) nonzero |= body[i] != 0;
        val = (flag && nonzero) ? 1u : 0u;
    } else if (w < sign_word) {
        int which = 0, first, cap;
        if (kind != 0) which = w < REC_B ? 0 : w < REC_C ? 1 : 2;
        slot_of(kind, which, first, cap);
        const uint64_t idx = r * gm.ints_per_rec + which;
        uint64_t st, en;
        bool flag;
        int_span(off, idx, count, body_len, st, en, flag);
        if (st > en || en > body_len) return UnpackWord{0u, WIRE_ERR_TABLE, false};
        const uint64_t len = en - st;
        const uint64_t b0 = (uint64_t)(w - first) * 4;
        for (int i = 0; i < 4; i++)
            if (b0 + i < len) val |= (uint32_t)body[st + b0 + i] << (8 * i);
        if (w - first == cap - 1) {                  // top word of the plane: nothing may lie above it
            bool over = false;
            for (uint64_t i = (uint64_t)cap * 4; i < len; i++) over |= body[st + i] != 0;
            if (over) err |= WIRE_ERR_WIDE;
        }
        if (w == first && kind != 0 && which != 1) { // a and c are positive: not zero, and never flagged
            bool nonzero = false;
            for (uint64_t i = 0; i < len; i++) nonzero |= body[st + i] != 0;
            if (!nonzero) err |= WIRE_ERR_AC;
            if (flag && nonzero) err |= WIRE_ERR_AC;
        }
    }
    return UnpackWord{val, err, true};
}

// k_widths, thread j = integer j: its slot bytes, flag bit in bit 63 (same packing as the offset table); j < n_rec * ints_per_rec
WIRE_DEV uint64_t wire_width(const uint32_t *__restrict__ rec, int kind, uint64_t j) {
    const Geometry gm = geometry(kind);
    const uint64_t r = j / gm.ints_per_rec;
    const int which = (int)(j % gm.ints_per_rec);
    int first, cap;
    slot_of(kind, which, first, cap);
    const uint32_t *p = rec + r * gm.rec_words + first;
    uint32_t bits = 0;
    for (int i = cap - 1; i >= 0; i--) {
        const uint32_t v = p[i];
        if (v) {
            bits = (uint32_t)i * 32 + 32 - WIRE_CLZ(v);
            break;
        }
    }
    const uint32_t sign = rec[r * gm.rec_words + (kind == 0 ? WIRE_EXP_MAG_WORDS : REC_SIGN)];
    const bool signed_slot = kind == 0 || which == 1;
    const bool flag = bits == 0 || (signed_slot && sign != 0);
    return (uint64_t)((bits ? bits : 1) / 8 + 1) | (flag ? (1ull << 63) : 0ull);
}

// k_pack, thread tid = (integer tid / max_words, group of 4 output bytes tid % max_words): writes up to 4 bytes of the slot
WIRE_DEV void wire_pack_group(const uint32_t *__restrict__ rec, const uint64_t *__restrict__ off, const uint64_t *__restrict__ width,
                              uint64_t n_rec, int kind, int max_words, uint8_t *__restrict__ body, uint64_t tid) {
    const Geometry gm = geometry(kind);
    const uint64_t j = tid / max_words;
    const int w = (int)(tid % max_words);
    if (j >= n_rec * gm.ints_per_rec) return;
    const uint64_t r = j / gm.ints_per_rec;
    const int which = (int)(j % gm.ints_per_rec);
    int first, cap;
    slot_of(kind, which, first, cap);
    const uint64_t len = width[j] & WIRE_OFFMASK;
    const uint64_t b0 = (uint64_t)w * 4;
    if (b0 >= len) return;
    const uint32_t v = w < cap ? rec[r * gm.rec_words + first + w] : 0u;      // the slot may be one byte longer than the plane
    uint8_t *dst = body + (off[j] & WIRE_OFFMASK) + b0;
    for (int i = 0; i < 4; i++)
        if (b0 + i < len) dst[i] = (uint8_t)(v >> (8 * i));
}

// 4-byte groups per slot that k_pack is launched with, the extra byte included
constexpr int wire_pack_groups(int kind) { return kind == 0 ? WIRE_EXP_MAG_WORDS + 1 : 81; }

}  // namespace cofhe
