// Host build of the segment index and of the bodies of k_spline_rows and k_spline_powers (cofhe_amd/csrc/spline.hpp): the very
// functions the kernels call, driven by plain loops in the kernels' own index order, one call per thread of the kernel.  TEST
// INFRASTRUCTURE ONLY; not linked into the product library.  spline_sim_main.cpp runs it stand-alone for the host sanitizers.
#define COFHE_HOSTSIM 1
#include "../../cofhe_amd/csrc/spline.hpp"

using namespace cofhe;

extern "C" {
int spline_sim_max_tuple(void) { return (int)SPLINE_MAX_TUPLE; }
// 0, or -1 for what the launchers refuse
int spline_sim_check(uint32_t bits, uint32_t shift, uint32_t d, uint32_t kbits, uint64_t n_tab, uint64_t n) {
    return spline_shape_ok(bits, shift, d, kbits) && n_tab != 0 && n % n_tab == 0 ? 0 : -1;
}
// idx[i] = bits shift .. shift + bits - 1 of rec[i] mod 2^kbits
int spline_sim_index(const uint32_t *recs, uint64_t n, uint32_t bits, uint32_t shift, uint32_t kbits, uint32_t *idx) {
    if (spline_sim_check(bits, shift, 1, kbits, 1, n)) return -1;
    for (uint64_t i = 0; i < n; i++) idx[i] = spline_index(recs + i * PMM_REC_WORDS, shift, bits, kbits);
    return 0;
}
// out[(i 2^bits + j) (d + 1) + c], as k_spline_rows
int spline_sim_rows(const uint32_t *pieces, uint64_t n_tab, const uint32_t *r, uint32_t *out, uint64_t n, uint32_t bits, uint32_t shift, uint32_t d,
                    uint32_t kbits) {
    if (spline_sim_check(bits, shift, d, kbits, n_tab, n)) return -1;
    for (uint64_t idx = 0; idx < (n << bits); idx++) spline_rows_element(pieces, n_tab, r, out, idx, bits, shift, (int)d, kbits);
    return 0;
}
// out[(c - 1) n + i] = e[i]^c mod 2^kbits, as k_spline_powers
int spline_sim_powers(const uint32_t *e, uint32_t *out, uint64_t n, uint32_t d, uint32_t kbits) {
    if (spline_sim_check(1, 0, d, kbits, 1, n)) return -1;
    for (uint64_t i = 0; i < n; i++) spline_powers_element(e, out, n, i, (int)d, kbits);
    return 0;
}
}
