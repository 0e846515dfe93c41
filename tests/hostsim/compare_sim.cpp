// Host build of the threshold arithmetic of k_cmp_close and the body of k_cmp_rows (cofhe_amd/csrc/compare.hpp): the very
// functions the kernels call, driven by plain loops in the kernels' own index order.  TEST INFRASTRUCTURE ONLY; not linked into
// the product library.
#define COFHE_HOSTSIM 1
#include "../../cofhe_amd/csrc/compare.hpp"

using namespace cofhe;

extern "C" {
int cmp_sim_max_digits(void) { return (int)CMP_MAX_DIGITS; }
// 1 where the launchers accept the shape (lut_max_bits: the widest lookup), 0 where they refuse it
int cmp_sim_shape_ok(uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint32_t lut_max_bits) {
    return cmp_shape_ok(bits, digit_bits, kbits, lut_max_bits) ? 1 : 0;
}
// per opened value: u, A, B, wrap, and the n digits of A and of B (dig[(i 2 + s) n + j]); -1 for what the launchers refuse
int cmp_sim_thresholds(const uint32_t *e, uint64_t count, uint32_t bits, uint32_t digit_bits, uint32_t kbits, uint64_t *u, uint64_t *a,
                       uint64_t *b, uint32_t *wrap, uint32_t *dig, uint64_t *entries) {
    if (!cmp_shape_ok(bits, digit_bits, kbits, 12)) return -1;
    const uint32_t n = cmp_digits(bits, digit_bits);
    for (uint64_t i = 0; i < count; i++) {
        u[i] = cmp_low(e + i * PMM_REC_WORDS, bits);
        const CmpThresholds t = cmp_thresholds(u[i], bits);
        a[i] = t.a;
        b[i] = t.b;
        wrap[i] = t.wrap;
        for (uint32_t j = 0; j < n; j++) {
            dig[(i * 2 + 0) * n + j] = cmp_digit(t.a, j, digit_bits);
            dig[(i * 2 + 1) * n + j] = cmp_digit(t.b, j, digit_bits);
            entries[(i * 2 + 0) * n + j] = cmp_entry(i, n, j, digit_bits, t.a);
            entries[(i * 2 + 1) * n + j] = cmp_entry(i, n, j, digit_bits, t.b);
        }
    }
    return 0;
}
// the rows as k_cmp_rows writes them: 16-byte pieces where `out` is 16-byte aligned, dwords otherwise (the launcher's test)
int cmp_sim_rows(const uint32_t *r, uint32_t *out, uint64_t count, uint32_t bits, uint32_t digit_bits, uint32_t kbits) {
    if (!cmp_shape_ok(bits, digit_bits, kbits, 12)) return -1;
    const bool vec16 = ((uintptr_t)out & 15) == 0;
    const uint64_t recs = (count * cmp_digits(bits, digit_bits)) << digit_bits;
    const uint64_t total = recs * (vec16 ? PMM_REC_WORDS / 4 : PMM_REC_WORDS);
    for (uint64_t idx = 0; idx < total; idx++) {
        if (vec16)
            cmp_rows_piece<4>(r, out, idx, bits, digit_bits);
        else
            cmp_rows_piece<1>(r, out, idx, bits, digit_bits);
    }
    return vec16 ? 16 : 4;
}
}
