// compare.hpp -- the threshold arithmetic of k_cmp_close and the body of k_cmp_rows (compare.hip): the sign of a ciphertext on
// a window of up to 64 bits from digit comparisons, in a header so that the host build of the CPU tests
// (tests/hostsim/compare_sim.cpp, COFHE_HOSTSIM) compiles the very code the kernels run.
//
// x lies in the signed window of l bits, 2 <= l <= min(k, 64); r mod 2^l is read as n = ceil(l / d) digits of d bits, 1 <= d <= 8
// (the top digit holds the l - (n - 1) d bits that remain and zeros above them).  Per element the tuple is ([r], [T]) with r
// uniform in Z/2^k and T[j][c] = 2^j sgn(r_j - c) mod 2^k, j < n, c < 2^d.  With the one opened value e = Dec(x - r) and
// u = e mod 2^l: x < 0 exactly when (u + r) mod 2^l >= 2^(l-1), which is r mod 2^l in the cyclic interval [A, B) with
// A = (2^(l-1) - u) mod 2^l and B = -u mod 2^l, so that [x < 0] = [r >= A] - [r >= B] + [A > B].  For a public threshold t,
// S_t = sum_j 2^j sgn(r_j - t_j) lies in (-2^n, 2^n) and [r >= t] = [S_t >= 0]: the highest differing digit outweighs the rest.
// [S_t] is the product of the n entries T[j][t_j]; A and B differ in bit l - 1 only, hence in the top digit only, so the two
// products share the n - 1 factors below it.  A lookup of n + 1 bits turns [S_t] into [S_t >= 0].
//
// A record is 31 magnitude words and a sign word (non-zero: negative).  l <= 64, so the low l bits of the magnitude are in
// words 0 and 1, and 2^l divides 2^k, so the residue mod 2^k of -m has the low bits of the 64-bit two's complement of them
// whatever else m holds: -0 and magnitudes of 2^k and above follow the rule of lut_index_of and need no case of their own.
#pragma once
#include "plain_mm.hpp"

namespace cofhe {

constexpr uint32_t CMP_MAX_BITS = 64;                        // the window
constexpr uint32_t CMP_MAX_DIGIT_BITS = 8;                   // 256 entries per digit
constexpr uint32_t CMP_MAX_DIGITS = 11;                      // n + 1 <= 12 bits, the largest lookup that closes the comparison
constexpr int CMP_ROWS_THREADS = 256;

constexpr uint32_t cmp_digits(uint32_t bits, uint32_t digit_bits) { return (bits + digit_bits - 1u) / digit_bits; }

// what every entry point checks before it looks at a pointer (constexpr: the launchers on the host call it too); lut_max_bits:
// the widest lookup, which has to hold n + 1 bits
constexpr bool cmp_shape_ok(uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint32_t lut_max_bits) {
    if (kbits == 0 || kbits > 32u * PMM_MAX_LIMBS - 1u) return false;
    if (bits < 2u || bits > CMP_MAX_BITS || bits > kbits) return false;
    if (digit_bits == 0 || digit_bits > CMP_MAX_DIGIT_BITS) return false;
    const uint32_t n = cmp_digits(bits, digit_bits);
    return n + 1u <= lut_max_bits && n + 1u <= kbits;
}

constexpr uint64_t cmp_mask(uint32_t bits) { return bits >= 64u ? ~0ull : (1ull << bits) - 1ull; }

// the value of an exponent record mod 2^bits, from its words 0 and 1 and its sign word
PMM_DEV uint64_t cmp_low_of(uint32_t word0, uint32_t word1, uint32_t sign_word, uint32_t bits) {
    const uint64_t m = ((uint64_t)word1 << 32) | word0;
    return (sign_word != 0 ? 0ull - m : m) & cmp_mask(bits);
}
PMM_DEV uint64_t cmp_low(const uint32_t *rec, uint32_t bits) { return cmp_low_of(rec[0], rec[1], rec[PMM_MAG_WORDS], bits); }

// the two thresholds of an opened value and the public term of the sign
struct CmpThresholds {
    uint64_t a, b;                                           // A = (2^(bits-1) - u) mod 2^bits, B = -u mod 2^bits
    uint32_t wrap;                                           // [A > B]
};
PMM_DEV CmpThresholds cmp_thresholds(uint64_t u, uint32_t bits) {
    CmpThresholds t;
    t.b = (0ull - u) & cmp_mask(bits);
    t.a = ((1ull << (bits - 1u)) - u) & cmp_mask(bits);
    t.wrap = t.a > t.b ? 1u : 0u;
    return t;
}

// digit j of a value below 2^bits: j digit_bits < bits <= 64, so the shift is below 64
PMM_DEV uint32_t cmp_digit(uint64_t v, uint32_t j, uint32_t digit_bits) {
    return (uint32_t)(v >> (j * digit_bits)) & ((1u << digit_bits) - 1u);
}

// word w of the record 2^j sgn(rj - c): the magnitude in word 0, a set sign word for a negative entry, all zero for equality
PMM_DEV uint32_t cmp_row_word(uint32_t rj, uint32_t c, uint32_t j, uint32_t w) {
    if (rj == c) return 0u;
    return w == 0u ? 1u << j : (w == (uint32_t)PMM_MAG_WORDS && rj < c) ? 1u : 0u;
}

// One piece of W words (4: a 16-byte store, the launcher found `out` aligned; 1: a dword) of the rows out[(i n + j) 2^d + c],
// i < elements, j < n = cmp_digits(bits, d), c < 2^d: piece idx of elements n 2^d (32 / W).  Consecutive threads take consecutive
// pieces of one record, so the stores are contiguous throughout; the two words read of r[i] are one address for the lanes that
// share an element (every lane of a wavefront once a tuple has 8 records or more).
template <int W>
PMM_DEV void cmp_rows_piece(const uint32_t *r, uint32_t *out, uint64_t idx, uint32_t bits, uint32_t digit_bits) {
    constexpr uint32_t pieces = (uint32_t)PMM_REC_WORDS / W;
    const uint32_t n = cmp_digits(bits, digit_bits);
    const uint64_t rec = idx / pieces, ej = rec >> digit_bits, i = ej / n;
    const uint32_t piece = (uint32_t)(idx - rec * pieces), c = (uint32_t)(rec - (ej << digit_bits)), j = (uint32_t)(ej - i * n);
    const uint32_t rj = cmp_digit(cmp_low(r + i * PMM_REC_WORDS, bits), j, digit_bits);
    uint32_t v[W];
    PMM_UNROLL
    for (int t = 0; t < W; t++) v[t] = cmp_row_word(rj, c, j, piece * W + (uint32_t)t);
#if defined(COFHE_HOSTSIM)
    for (int t = 0; t < W; t++) out[idx * W + t] = v[t];
#else
    if constexpr (W == 4)
        ((uint4 *)out)[idx] = make_uint4(v[0], v[1], v[2], v[3]);
    else
        out[idx] = v[0];
#endif
}

// the tuple entry of element i that a threshold's digit j selects: a ciphertext index into tuples[elements][n][2^d]
PMM_DEV uint64_t cmp_entry(uint64_t i, uint32_t n, uint32_t j, uint32_t digit_bits, uint64_t threshold) {
    return (((i * n + j) << digit_bits) + cmp_digit(threshold, j, digit_bits));
}

}  // namespace cofhe
