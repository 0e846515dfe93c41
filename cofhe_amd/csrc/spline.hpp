// spline.hpp -- the bodies of k_spline_rows and k_spline_powers and the segment index of k_spline_close (spline.hip):
// piecewise-polynomial activations on ciphertext tensors from one opened value, in a header so that the host build of the CPU
// tests (tests/hostsim/spline_sim.cpp, COFHE_HOSTSIM) compiles the very code the kernels run.
//
// Plaintexts live in Z/2^k.  A spline table is 2^b pieces of d + 1 plaintext coefficients over a window of W = t + b <= k bits:
// b segment bits above t segment-width bits.  Piece pi < 2^b has the origin o(pi) = sigma(pi) 2^t, sigma(pi) the b-bit two's
// complement reading of pi, and evaluates S_pi(x) = sum_i c[pi][i] (x - o(pi))^i mod 2^k.  The segment of x is
// pi(x) = floor((x mod 2^W) / 2^t).  Per element the tuple is ([r], [q_{j,i}], j < 2^b, i <= d) with r uniform in Z/2^k,
// rho = pi(r), pi_j = (j + rho) mod 2^b and q_{j,.} the Taylor shift (poly_shift.hpp) of piece pi_j at (r - o(pi_j)) mod 2^k:
//   sum_i q_{j,i} E^i = sum_i c[pi_j][i] (E + r - o(pi_j))^i.
// With the one opened value e = Dec(x - r) and j = pi(e), [y] = [q_{j,0}] o prod_{i=1..d} [q_{j,i}]^(e^i mod 2^k): since
// e + r = x mod 2^k and 2^W divides 2^k, y = S_{pi'}(x) with pi' = (pi(x) - c) mod 2^b, c = [(e mod 2^t) + (r mod 2^t) >= 2^t]:
// the element's own piece or the one below (the lost carry of the low t bits, as the division's "floor quotient or one less").
//
// THE CALLER'S CONTRACT: piece pi approximates the function on [o(pi), o(pi) + 2^(t+1)), two segments; x stays out of the lowest
// segment (sigma = -2^(b-1)), where the piece below wraps round to the top piece; fixed-point scales are the caller's.
// t = 0 has no carry: the result is exact on the element's own piece.
//
// A record is 31 magnitude words and a sign word (non-zero: negative); everything here enters as its residue mod 2^k by
// pmm_reduce (plain_mm.hpp), so -0 and magnitudes of 2^k and above need no case of their own, and leaves by pmm_store as a
// record in [0, 2^k) with sign word 0.
#pragma once
#include "poly_shift.hpp"

namespace cofhe {

constexpr uint32_t SPLINE_MAX_TUPLE = 4096;                  // 2^b (d + 1) ciphertexts per element: the largest lookup tuple
constexpr int SPL_THREADS = 64;                              // threads of a k_spline_rows / k_spline_powers workgroup

// what every entry point checks before it looks at a pointer (constexpr: the launchers on the host call it too)
constexpr bool spline_shape_ok(uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits) {
    if (kbits == 0 || kbits > 32u * PMM_MAX_LIMBS - 1u) return false;
    if (bits == 0 || bits > 12u || d == 0 || d > (uint32_t)POLY_MAX_DEGREE) return false;
    if (((uint64_t)(d + 1) << bits) > SPLINE_MAX_TUPLE) return false;
    return (uint64_t)shift + bits <= kbits;
}

// limb l of value 2^t, value a 32-bit number
PMM_DEV uint32_t spline_limb(uint32_t value, uint32_t t, int l) {
    const int w = (int)(t >> 5);
    const uint64_t v = (uint64_t)value << (t & 31u);
    return l == w ? (uint32_t)v : l == w + 1 ? (uint32_t)(v >> 32) : 0u;
}

// bits t .. t + b - 1 of a residue of L limbs (the field may straddle a word boundary and lie in any word; t + b <= 32 L)
template <int LMAX>
PMM_DEV uint32_t spline_field(const uint32_t (&v)[LMAX], int L, uint32_t t, uint32_t b) {
    const int w = (int)(t >> 5);
    const uint32_t s = t & 31u;
    uint32_t lo = 0, hi = 0;
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) {                          // selects, not an indexed read: v stays in registers
        if (l < L) {
            lo = l == w ? v[l] : lo;
            hi = l == w + 1 ? v[l] : hi;
        }
    }
    const uint64_t two = ((uint64_t)hi << 32) | lo;
    return (uint32_t)(two >> s) & ((1u << b) - 1u);
}

// bits t .. t + b - 1 of an exponent record's residue mod 2^kbits, 1 <= b <= 12, t + b <= kbits <= 32 LMAX: under a set sign word
// the field of the two's complement of the magnitude; -0 and magnitudes of 2^kbits and above follow the same rule
template <int LMAX>
PMM_DEV uint32_t spline_index_limbs(const uint32_t *rec, uint32_t t, uint32_t b, uint32_t kbits) {
    uint32_t v[LMAX];
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) v[l] = 0;
    pmm_reduce<LMAX>(rec, pmm_limbs(kbits), kbits, v, 1);
    return spline_field<LMAX>(v, pmm_limbs(kbits), t, b);
}
PMM_DEV uint32_t spline_index(const uint32_t *rec, uint32_t t, uint32_t b, uint32_t kbits) {
    return pmm_limbs(kbits) <= PMM_FIXED_LIMBS ? spline_index_limbs<PMM_FIXED_LIMBS>(rec, t, b, kbits)
                                               : spline_index_limbs<PMM_MAX_LIMBS>(rec, t, b, kbits);
}

// row j of element i's tuple reads piece (j + rho) mod 2^b, rho the segment of r
PMM_DEV uint32_t spline_row_piece(uint32_t j, uint32_t rho, uint32_t b) { return (j + rho) & ((1u << b) - 1u); }

// One (element, row): the d + 1 records q[0 .. d] of the Taylor shift of the piece `coef` (d + 1 records) = piece (j + rho) mod 2^b
// at (r - o(piece)) mod 2^k.  The shift point is built as a record of its own (xr: every index a constant once the loops
// unroll, so it lives in registers) and handed to poly_shift_body, whose working array is a register array for k <= 256
// (UF = POLY_MAX_DEGREE + 1) and the row's own output records beyond (UF = 1), as in poly_shift_element.
template <int LMAX, int UF>
PMM_DEV void spline_row_body(const uint32_t *pieces, uint64_t tab, const uint32_t *rrec, uint32_t *q, uint32_t j, uint32_t b, uint32_t t, int d,
                             uint32_t kbits, uint32_t *w, uint64_t wj) {
    const int L = pmm_limbs(kbits);
    uint32_t v[LMAX];
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) v[l] = 0;
    pmm_reduce<LMAX>(rrec, L, kbits, v, 1);
    const uint32_t piece = spline_row_piece(j, spline_field<LMAX>(v, L, t, b), b);
    // r - piece 2^t, and + 2^(t + b) where sigma(piece) is negative (nothing when t + b = k): r - sigma(piece) 2^t mod 2^k
    const uint32_t top = piece >> (b - 1u);
    uint32_t borrow = 0, carry = 0;
    uint32_t xr[PMM_REC_WORDS];
    PMM_UNROLL
    for (int l = 0; l < PMM_REC_WORDS; l++) xr[l] = 0;
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) {
        if (l < L) {
            const uint64_t sub = (uint64_t)v[l] - spline_limb(piece, t, l) - borrow;
            borrow = (uint32_t)(sub >> 32) & 1u;
            const uint64_t add = (uint64_t)(uint32_t)sub + spline_limb(top, t + b, l) + carry;
            carry = (uint32_t)(add >> 32);
            xr[l] = l == L - 1 ? (uint32_t)add & pmm_top_mask(kbits) : (uint32_t)add;
        }
    }
    const uint32_t *coef = pieces + ((tab << b) + piece) * (uint64_t)(d + 1) * PMM_REC_WORDS;
    poly_shift_body<LMAX, UF>(coef, xr, q, 1, 0, d, L, kbits, w, wj);
}

// thread idx of n 2^b: element i = idx >> b, row j; out[(i 2^b + j) (d + 1) + c], c <= d; element i reads table i mod n_tab
PMM_DEV void spline_rows_element(const uint32_t *pieces, uint64_t n_tab, const uint32_t *r, uint32_t *out, uint64_t idx, uint32_t b, uint32_t t,
                                 int d, uint32_t kbits) {
    const uint64_t i = idx >> b;
    const uint32_t j = (uint32_t)(idx - (i << b));
    uint32_t *q = out + idx * (uint64_t)(d + 1) * PMM_REC_WORDS;
    const uint32_t *rrec = r + i * PMM_REC_WORDS;
    if (pmm_limbs(kbits) <= PMM_FIXED_LIMBS) {
        uint32_t w[(POLY_MAX_DEGREE + 1) * PMM_FIXED_LIMBS];
        spline_row_body<PMM_FIXED_LIMBS, POLY_MAX_DEGREE + 1>(pieces, i % n_tab, rrec, q, j, b, t, d, kbits, w, PMM_FIXED_LIMBS);
    } else {
        spline_row_body<PMM_MAX_LIMBS, 1>(pieces, i % n_tab, rrec, q, j, b, t, d, kbits, q, PMM_REC_WORDS);
    }
}

// out[(c - 1) n + i] = e[i]^c mod 2^k, c = 1 .. d: power-major, the layout k_pow_dot reads its exponents in
template <int LMAX>
PMM_DEV void spline_powers_body(const uint32_t *e, uint32_t *out, uint64_t n, uint64_t i, int d, uint32_t kbits) {
    const int L = pmm_limbs(kbits);
    uint32_t ev[LMAX], p[LMAX];
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) ev[l] = 0;
    pmm_reduce<LMAX>(e + i * PMM_REC_WORDS, L, kbits, ev, 1);
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) p[l] = ev[l];
    for (int c = 1; c <= d; c++) {
        if (c > 1) {
            uint32_t acc[LMAX];
            PMM_UNROLL
            for (int l = 0; l < LMAX; l++) acc[l] = 0;
            pmm_mac<LMAX>(acc, p, 1, ev, 1, L);
            PMM_UNROLL
            for (int l = 0; l < LMAX; l++) p[l] = acc[l];
        }
        pmm_store<LMAX>(p, L, kbits, out + ((uint64_t)(c - 1) * n + i) * PMM_REC_WORDS);
    }
}
PMM_DEV void spline_powers_element(const uint32_t *e, uint32_t *out, uint64_t n, uint64_t i, int d, uint32_t kbits) {
    if (pmm_limbs(kbits) <= PMM_FIXED_LIMBS)
        spline_powers_body<PMM_FIXED_LIMBS>(e, out, n, i, d, kbits);
    else
        spline_powers_body<PMM_MAX_LIMBS>(e, out, n, i, d, kbits);
}

}  // namespace cofhe
