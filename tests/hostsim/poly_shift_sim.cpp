// Host build of k_poly_shift's body (cofhe_amd/csrc/poly_shift.hpp) with COFHE_HOSTSIM: the very function the kernel runs,
// one call per element as the kernel has one thread per element.  TEST INFRASTRUCTURE ONLY; not linked into the product library.
#define COFHE_HOSTSIM 1
#include "../../cofhe_amd/csrc/poly_shift.hpp"

using namespace cofhe;

extern "C" {
// q[i n + e] = sum_{j >= i} C(j, i) coef[j] x[e]^(j - i) mod 2^kbits, i <= d, on exponent records; returns 0, or -1 for a
// kbits or a degree the kernel's launcher refuses
int poly_shift_sim(const uint32_t *coef, const uint32_t *x, uint32_t *q, uint64_t n, uint32_t d, uint32_t kbits) {
    if (kbits == 0 || kbits > 32u * PMM_MAX_LIMBS || d > (uint32_t)POLY_MAX_DEGREE) return -1;
    for (uint64_t e = 0; e < n; e++) poly_shift_element(coef, x, q, n, e, (int)d, kbits);
    return 0;
}
int poly_shift_sim_fixed_limbs(void) { return PMM_FIXED_LIMBS; }
}
