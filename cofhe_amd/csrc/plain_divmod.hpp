// plain_divmod.hpp -- the bodies of k_plain_divmod, k_divx_prep and k_divx_rows (divide_exact.hip): the exact floor division of
// ciphertexts by small public divisors from one opened value, in a header so that the host build of the CPU tests
// (tests/hostsim/divx_sim.cpp, COFHE_HOSTSIM) compiles the very code the kernels run.
//
// With s(v) the centred residue of v mod 2^k, a public divisor 1 <= D <= DIVX_MAX_ROWS, D < 2^(k-1), q(v) = floor(s(v) / D) and
// m(v) = s(v) - D q(v) in [0, D), the exact-division tuple of an element is ([r], [T_0], .., [T_{D-1}]) with r uniform in Z/2^k
// and T_j = (q(r) + [m(r) + j >= D]) mod 2^k: the quotient of the mask plus the carry of the two remainders, tabulated over the D
// remainders the opened value can have.  With e = Dec(x - r) the result is [T_{m(e)}] plus the plaintext q(e), which is
// floor(s(x) / D) whenever s(x) = s(r) + s(e) over the integers, and x - D y = (m(r) + m(e)) mod D.
//
// plain_divmod_element is plain_divfloor_element (plain_div.hpp) that keeps the remainder: the negative branch divides m - 1 of
// the residue -m, giving q' and rho'; then q = ~q' within k bits and the remainder is D - 1 - rho'.  A divisor is invalid as in
// plain_div.hpp and also when it exceeds `rows`: quotient 0, remainder 0 and CF_ST_DIV_CAP.  A valid divisor fits 13 bits, so
// mp_divrem takes its word route; nothing loops on data.
//
// The rows are written in two passes.  divx_prep_element leaves per element a block of DIVX_PREP_WORDS words: the record of q(r),
// the record of q(r) + 1 mod 2^k, and a record whose word 0 is the threshold D - m(r) (in [1, D]) and whose word 1 is D (0, 0 for
// an invalid divisor).  divx_rows_piece then stores one piece of one output record: row j is the zero record for j >= D, the
// second record for j >= threshold and the first below it.
#pragma once
#include "plain_div.hpp"

namespace cofhe {

constexpr uint32_t DIVX_MAX_ROWS = 4096;                     // the widest tuple, as a lookup of LUT_MAX_BITS
constexpr int DIVX_PREP_WORDS = 3 * PMM_REC_WORDS;           // q(r) | q(r) + 1 | threshold, D, zeros
constexpr int DIVX_ROWS_THREADS = 256;
constexpr int DIVX_SELECT_THREADS = 256;                     // k_divx_select: one wavefront per output ciphertext
constexpr int DIVX_SELECT_WAVES = DIVX_SELECT_THREADS / 64;

// the divisor of an element, or bad: a set sign word, a residue of 0, 2^(k-1) or more, or more than rows (rows <= DIVX_MAX_ROWS)
CF_DEV bool divx_load_divisor(Ctx &c, const uint32_t *drec, uint32_t rows, uint32_t kbits, Mp<1> &den, uint32_t &D) {
    den = pdv_load_magnitude(c, drec, kbits);
    const int sign_limb = (int)((kbits - 1) >> 5);
    const uint32_t sign_bit = 1u << ((kbits - 1) & 31);
    D = mp_get_limb(c, den, 0);
    return drec[PMM_MAG_WORDS] == 0 && !mp_is_zero(c, den) && (mp_get_limb(c, den, sign_limb) & sign_bit) == 0 && mp_bitlen(c, den) <= 32 &&
           D <= rows;
}

// q = floor(s(v) / D) mod 2^kbits and the remainder m = s(v) - D q(v) of a valid divisor (den its plane, D its value); every lane
// of the group calls this with the same arguments and gets the same m
CF_DEV uint32_t divx_divmod(Ctx &c, const uint32_t *vrec, const Mp<1> &den, uint32_t D, uint32_t kbits, Mp<1> &q) {
    const int sign_limb = (int)((kbits - 1) >> 5);
    const uint32_t sign_bit = 1u << ((kbits - 1) & 31);
    Mp<1> num = pdv_load_residue(c, vrec, kbits);
    const bool neg = (mp_get_limb(c, num, sign_limb) & sign_bit) != 0;
    if (neg) num = pdv_complement(c, num, kbits);                   // m - 1 of the magnitude m = 2^k - v
    mp_divrem<1, 1>(c, num, den, q);
    const uint32_t rho = mp_get_limb(c, num, 0);
    if (neg) q = pdv_complement(c, q, kbits);                       // 2^k - (q' + 1)
    return neg ? D - 1u - rho : rho;
}

// qrec = q(v), *rem = m(v), 1 <= kbits <= PDV_MAX_KBITS and 1 <= rows <= DIVX_MAX_ROWS (the launcher's checks)
CF_DEV void plain_divmod_element(Ctx &c, const uint32_t *vrec, const uint32_t *drec, uint32_t *qrec, uint32_t *rem, uint32_t rows, uint32_t kbits) {
    Mp<1> den, q;
    uint32_t D, m = 0;
    if (divx_load_divisor(c, drec, rows, kbits, den, D)) {
        m = divx_divmod(c, vrec, den, D, kbits, q);
    } else {
        CF_STATUS(c, CF_ST_DIV_CAP);
        mp_zero(q);
    }
    pdv_store(c, q, qrec);
    if (c.gl == 0) *rem = m;
}

// the element's block of the store pass: every word of the three records written
CF_DEV void divx_prep_element(Ctx &c, const uint32_t *rrec, const uint32_t *drec, uint32_t *prep, uint32_t rows, uint32_t kbits) {
    Mp<1> den, q, q1, head;
    uint32_t D, thr = 0;
    if (divx_load_divisor(c, drec, rows, kbits, den, D)) {
        thr = D - divx_divmod(c, rrec, den, D, kbits, q);
        Mp<1> one;
        mp_set_word(c, one, 1u);
        (void)mp_add(c, q1, q, one);                                // q + 1 mod 2^k: the bits from k up are masked off
        const int L = pmm_limbs(kbits);
        const uint32_t top = pmm_top_mask(kbits);
        CF_UNROLL for (int j = 0; j < CH; j++) {
            const int i = c.gl * CH + j;
            q1.v[0][j] = i < L - 1 ? q1.v[0][j] : (i == L - 1 ? q1.v[0][j] & top : 0u);
        }
    } else {
        CF_STATUS(c, CF_ST_DIV_CAP);
        D = 0;
        mp_zero(q);
        mp_zero(q1);
    }
    mp_zero(head);
    if (c.gl == 0) {
        head.v[0][0] = thr;
        head.v[0][1] = D;
    }
    pdv_store(c, q, prep);
    pdv_store(c, q1, prep + PMM_REC_WORDS);
    pdv_store(c, head, prep + 2 * PMM_REC_WORDS);
}

// One piece of W words (4: a 16-byte store, the launcher found `out` aligned; 1: a dword) of the rows out[i rows + j], i < n,
// j < rows: piece idx of n rows (32 / W).  Consecutive threads take consecutive pieces of one record, so the stores are contiguous
// throughout; the two words read of the element's block are one address for the lanes that share an element, and the piece read
// of its first or second record is contiguous across the lanes of one output record.
template <int W>
PMM_DEV void divx_rows_piece(const uint32_t *prep, uint32_t *out, uint64_t idx, uint32_t rows) {
    constexpr uint32_t pieces = (uint32_t)PMM_REC_WORDS / W;
    const uint64_t rec = idx / pieces, i = rec / rows;
    const uint32_t piece = (uint32_t)(idx - rec * pieces), j = (uint32_t)(rec - i * rows);
    const uint32_t *blk = prep + i * DIVX_PREP_WORDS;
    const uint32_t thr = blk[2 * PMM_REC_WORDS], D = blk[2 * PMM_REC_WORDS + 1];
    const uint32_t *src = blk + (j >= thr ? PMM_REC_WORDS : 0) + piece * W;
    const bool live = j < D;
#if defined(COFHE_HOSTSIM)
    for (int t = 0; t < W; t++) out[idx * W + t] = live ? src[t] : 0u;
#else
    if constexpr (W == 4)
        ((uint4 *)out)[idx] = live ? *(const uint4 *)src : make_uint4(0u, 0u, 0u, 0u);
    else
        out[idx] = live ? src[0] : 0u;
#endif
}

// the tuple entry of element i that a remainder selects, in 64 bits; an index of rows or more is never read: entry 0 and *bad
PMM_DEV uint64_t divx_entry(uint64_t i, uint32_t rows, uint32_t index, bool *bad) {
    *bad = index >= rows;
    return i * (uint64_t)rows + (*bad ? 0u : index);
}

}  // namespace cofhe
