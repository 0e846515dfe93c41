// poly_shift.hpp -- the body of k_poly_shift (pow_dot.hip): the Taylor shift of a polynomial mod 2^k on exponent records,
//   q[i E + e] = sum_{j >= i} C(j, i) coef[j] x[e]^(j - i) mod 2^k,   i = 0 .. d,
// in a header so that the host build of the CPU tests (tests/hostsim/poly_shift_sim.cpp, COFHE_HOSTSIM) compiles the very code
// the kernel runs.  With x = a + e the q_i are the coefficients of p in powers of a: the exponents of the closing step of a
// polynomial evaluation on ciphertexts (cofhe_hip_poly_close_records).
//
// Repeated synthetic division: for i = 0 .. d - 1, for j = d - 1 down to i: c[j] += x c[j + 1]; afterwards c[i] = q_i.  No
// binomials, no divisions, d (d + 1) / 2 low-half products.  Values enter as residues mod 2^k and leave as records in
// [0, 2^k) with sign word 0, exactly as in the plaintext matrix product, whose load, product and store these are
// (plain_mm.hpp: pmm_reduce, pmm_mac, pmm_store).
//
// One thread per element.  The working array c[0 .. d] of L = ceil(k / 32) limbs each is addressed as w[j wj + l]: for
// k <= 256 the kernel hands in a register array (wj = LMAX = L, every loop unrolled, so every index is a constant); beyond
// that (runtime L <= PMM_MAX_LIMBS) it hands in the element's own OUTPUT records (wj = E records apart), which the final
// store rewrites in full: no scratch and no LDS either way.
#pragma once
#include "plain_mm.hpp"
#include "pow_dot.hpp"

#if defined(COFHE_HOSTSIM)
#define PSH_UNROLL(n)
#else
#define PSH_PRAGMA(x) _Pragma(#x)
#define PSH_UNROLL(n) PSH_PRAGMA(unroll n)
#endif

namespace cofhe {

constexpr int PSH_THREADS = 64;             // threads of a k_poly_shift workgroup

// UF: unroll count of the loops over the coefficients (POLY_MAX_DEGREE + 1 = all of them: the register array; 1: none)
template <int LMAX, int UF>
PMM_DEV void poly_shift_body(const uint32_t *coef, const uint32_t *xrec, uint32_t *q, uint64_t E, uint64_t e, int d, int L, uint32_t kbits,
                             uint32_t *w, uint64_t wj) {
    uint32_t xv[LMAX];
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) xv[l] = 0;
    pmm_reduce<LMAX>(xrec, L, kbits, xv, 1);
    PSH_UNROLL(UF)
    for (int j = 0; j <= POLY_MAX_DEGREE; j++)
        if (j <= d) pmm_reduce<LMAX>(coef + (uint64_t)j * PMM_REC_WORDS, L, kbits, w + j * wj, 1);
    PSH_UNROLL(UF)
    for (int i = 0; i < POLY_MAX_DEGREE; i++) {
        PSH_UNROLL(UF)
        for (int j = POLY_MAX_DEGREE - 1; j >= 0; j--) {
            if (i < d && j < d && j >= i) {                   // guards, not bounds: the loops unroll for a runtime d too
                uint32_t acc[LMAX];
                PMM_UNROLL
                for (int l = 0; l < LMAX; l++) acc[l] = l < L ? w[j * wj + l] : 0u;
                pmm_mac<LMAX>(acc, xv, 1, w + (j + 1) * wj, 1, L);
                PMM_UNROLL
                for (int l = 0; l < LMAX; l++)
                    if (l < L) w[j * wj + l] = acc[l];
            }
        }
    }
    PSH_UNROLL(UF)
    for (int j = 0; j <= POLY_MAX_DEGREE; j++) {
        if (j <= d) {
            uint32_t acc[LMAX];
            PMM_UNROLL
            for (int l = 0; l < LMAX; l++) acc[l] = l < L ? w[j * wj + l] : 0u;
            pmm_store<LMAX>(acc, L, kbits, q + ((uint64_t)j * E + e) * PMM_REC_WORDS);
        }
    }
}

// element e of E: the dispatch on the limb count, as k_plain_matmul's
template <int LMAX>
PMM_DEV void poly_shift_fixed(const uint32_t *coef, const uint32_t *x, uint32_t *q, uint64_t E, uint64_t e, int d, uint32_t kbits) {
    uint32_t w[(POLY_MAX_DEGREE + 1) * LMAX];
    poly_shift_body<LMAX, POLY_MAX_DEGREE + 1>(coef, x + e * PMM_REC_WORDS, q, E, e, d, LMAX, kbits, w, LMAX);
}
PMM_DEV void poly_shift_element(const uint32_t *coef, const uint32_t *x, uint32_t *q, uint64_t E, uint64_t e, int d, uint32_t kbits) {
    switch (pmm_limbs(kbits)) {
        case 1: poly_shift_fixed<1>(coef, x, q, E, e, d, kbits); break;
        case 2: poly_shift_fixed<2>(coef, x, q, E, e, d, kbits); break;
        case 3: poly_shift_fixed<3>(coef, x, q, E, e, d, kbits); break;
        case 4: poly_shift_fixed<4>(coef, x, q, E, e, d, kbits); break;
        case 5: poly_shift_fixed<5>(coef, x, q, E, e, d, kbits); break;
        case 6: poly_shift_fixed<6>(coef, x, q, E, e, d, kbits); break;
        case 7: poly_shift_fixed<7>(coef, x, q, E, e, d, kbits); break;
        case 8: poly_shift_fixed<PMM_FIXED_LIMBS>(coef, x, q, E, e, d, kbits); break;
        default:
            poly_shift_body<PMM_MAX_LIMBS, 1>(coef, x + e * PMM_REC_WORDS, q, E, e, d, pmm_limbs(kbits), kbits, q + e * PMM_REC_WORDS,
                                              E * PMM_REC_WORDS);
            break;
    }
}

}  // namespace cofhe
