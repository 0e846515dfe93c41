// comb.hpp -- fixed-base comb powers: base^e[i] for many exponents e[i] against one cached table per base.
//
// Signed radix-2^w digits in Booth form, read straight from the exponent record:
//   d_j = window_j(x) + bit_(wj-1)(x) - 2^w bit_(wj+w-1)(x),   window_j(x) = bits wj .. wj+w-1 of x, bit_(-1) = 0,
// so that |d_j| <= 2^(w-1), sum_j d_j 2^(wj) = x, and every digit is a function of w + 1 bits: no carry chain, no
// digit buffer.  A B-bit magnitude needs floor(B/w) + 1 positions.  The table of a base b holds
//   T[j][d] = b^(d 2^(wj)),  1 <= d <= 2^(w-1),  j < floor(992/w) + 1     (entry j 2^(w-1) + d - 1)
// so that b^x is the product of at most floor(B/w) + 1 entries, one per position, an entry inverted where its digit is
// negative and the principal form where it is zero.  No squarings at all: the product is a pairwise tree.
//
// Slots: the entries of one output record (a column) are its slots, in a fixed order that the host derives from the
// call alone (w, the longest exponent, k):
//   [0, npos_r)                 positions of r against the column's r table (half 0: h or the base, half 1: pk)
//   [npos_r, npos_r + npos_m)   positions of m mod 2^k against the table of f -- half 1 of an encryption only; the
//                               other half has principal forms there
//   npos_r + npos_m             the leaf (re-randomisation, plaintext addend): record 2i + h of the input ciphertexts,
//                               inverted where the shape says so (m - ct)
//   up to an even count         principal forms
// Columns are the output records: (c1 of ciphertext 0, c2 of ciphertext 0, c1 of ciphertext 1, ...), or one per
// exponent for plain powers.  The fused first level composes slots 2s and 2s + 1 of a column; k_compose_pairs does the rest.
// A plaintext addend without randomness (c2_only) has ONE column per ciphertext, its c2: no r positions, the positions
// of m, the leaf 2i + 1 -- ct + m = (c1, c2 o f^m) spends nothing on c1.  With randomness it is an encryption's two
// columns plus the leaf: (c1 o h^r, c2 o pk^r o f^m) in one tree.
#pragma once
#include "qf.hpp"

namespace cofhe {

constexpr int COMB_W_MIN = 2, COMB_W_MAX = 10;
constexpr uint32_t COMB_EXP_BITS = EXP_MAG_WORDS * 32;               // 992: the magnitude of an exponent record
constexpr uint32_t comb_positions(uint32_t bits, uint32_t w) { return bits / w + 1; }
constexpr uint32_t comb_table_positions(uint32_t w) { return comb_positions(COMB_EXP_BITS, w); }
constexpr uint32_t comb_entries(uint32_t w) { return 1u << (w - 1); }          // entries per position
// a table position j is built from chain entry b^(2^(wj)): the highest is w floor(992/w) <= 992 < the chain's 994
constexpr uint32_t comb_chain_index(uint32_t j, uint32_t w) { return w * j; }

// cnt (<= 32) bits of the magnitude from bit lo (>= -1) on; bits below 0 and at or above nbits read as 0
CF_DEV uint32_t comb_field(const uint32_t *e, int lo, int cnt, int nbits) {
    int sh = 0;
    if (lo < 0) {
        sh = -lo;
        cnt -= sh;
        lo = 0;
    }
    if (nbits > (int)COMB_EXP_BITS) nbits = (int)COMB_EXP_BITS;
    if (cnt <= 0 || lo >= nbits) return 0u;
    if (lo + cnt > nbits) cnt = nbits - lo;
    const int i = lo >> 5, o = lo & 31;
    uint64_t t = e[i];
    if (i + 1 < EXP_MAG_WORDS) t |= (uint64_t)e[i + 1] << 32;
    return (uint32_t)((t >> o) & ((1ull << cnt) - 1ull)) << sh;
}

// Booth digit j (window width w) of the magnitude's low nbits bits; the record's sign word is NOT applied
CF_DEV int comb_digit(const uint32_t *e, int j, int w, int nbits) {
    const uint32_t f = comb_field(e, w * j - 1, w + 1, nbits);          // bit 0: bit_(wj-1); bits 1..w: the window
    return (int)(f >> 1) + (int)(f & 1u) - (int)(((f >> w) & 1u) << w);
}

// the shape of one call: what the host derives (from w, the longest exponent and k) and every kernel reads
struct CombShape {
    uint32_t w;         // window width
    uint32_t npos_r;    // positions of r (or of the exponents of plain powers)
    uint32_t npos_m;    // positions of m mod 2^k (encryption), else 0
    uint32_t leaf;      // 1: one slot holds the input record (re-randomisation)
    uint32_t halves;    // columns per item: 2 (ciphertexts) or 1 (plain powers)
    uint32_t kbits;     // k (encryption, plaintext addend)
    // the plaintext addend; zero in every other call
    uint32_t c2_only;   // 1: one column per ciphertext, its c2 (half 1, leaf record 2i + 1)
    uint32_t m_neg;     // 1: the digits of m change sign (ct - m)
    uint32_t leaf_inv;  // 1: the leaf is inverted (m - ct)
};
constexpr uint32_t comb_slots(const CombShape &s) { return (s.npos_r + s.npos_m + s.leaf + 1u) & ~1u; }

// what slot s of a column of half h selects
struct CombSel {
    int table;          // -1 principal form, 0 / 1: the r table of half 0 / 1, 2: the table of f, 3: the leaf
    int pos;            // position j (tables)
    int digit;          // signed digit, sign word applied (tables; 0 for principal / leaf)
};
CF_DEV CombSel comb_select(const CombShape &s, uint32_t h, uint32_t slot, const uint32_t *r_exp, const uint32_t *m_exp) {
    CombSel o{-1, 0, 0};
    if (slot < s.npos_r) {
        const int d = comb_digit(r_exp, (int)slot, (int)s.w, (int)COMB_EXP_BITS);
        o.pos = (int)slot;
        o.digit = r_exp[EXP_MAG_WORDS] ? -d : d;
        o.table = d != 0 ? (int)h : -1;
    } else if (slot < s.npos_r + s.npos_m) {
        if (h == 1) {
            const int j = (int)(slot - s.npos_r);
            const int d = comb_digit(m_exp, j, (int)s.w, (int)s.kbits);          // f has order 2^k: m mod 2^k
            o.pos = j;
            o.digit = ((m_exp[EXP_MAG_WORDS] != 0) != (s.m_neg != 0)) ? -d : d;
            o.table = d != 0 ? 2 : -1;
        }
    } else if (s.leaf && slot == s.npos_r + s.npos_m) {
        o.table = 3;
    }
    return o;
}
// the record of a table entry (table != -1, 3)
CF_DEV uint32_t comb_entry(const CombShape &s, const CombSel &sel) {
    const int a = sel.digit < 0 ? -sel.digit : sel.digit;
    return (uint32_t)sel.pos * comb_entries(s.w) + (uint32_t)(a - 1);
}

}  // namespace cofhe
