// Host build of the index arithmetic of k_lut_rotate and k_lut_select (cofhe_amd/csrc/lut.hpp): the very functions the
// kernels call, driven by plain loops over the records in the kernels' own index order.  TEST INFRASTRUCTURE ONLY; not linked
// into the product library.
#define COFHE_HOSTSIM 1
#include <string.h>

#include "../../cofhe_amd/csrc/lut.hpp"

using namespace cofhe;

extern "C" {
int lut_sim_max_bits(void) { return (int)LUT_MAX_BITS; }
// idx[i] = the index of rec[i]; -1 for what the launchers refuse, nothing written
int lut_sim_index(const uint32_t *recs, uint64_t n, uint32_t bits, uint32_t *idx) {
    if (bits == 0 || bits > LUT_MAX_BITS) return -1;
    for (uint64_t i = 0; i < n; i++) idx[i] = lut_index(recs + i * PMM_REC_WORDS, bits);
    return 0;
}
// out[i 2^bits + j] = table[(i mod n_tab) 2^bits + ((j + r[i]) mod 2^bits)], records copied word for word as k_lut_rotate does
int lut_sim_rotate(const uint32_t *table, uint64_t n_tab, const uint32_t *r, uint32_t *out, uint64_t n, uint32_t bits) {
    if (bits == 0 || bits > LUT_MAX_BITS || n_tab == 0 || n % n_tab != 0) return -1;
    for (uint64_t rec = 0; rec < (n << bits); rec++) {
        const uint64_t i = rec >> bits;
        const uint32_t j = (uint32_t)(rec - (i << bits));
        const uint32_t src = lut_rotated_source(j, lut_index(r + i * PMM_REC_WORDS, bits), bits);
        memcpy(out + rec * PMM_REC_WORDS, table + (((i % n_tab) << bits) + src) * PMM_REC_WORDS, PMM_REC_WORDS * 4);
    }
    return 0;
}
}
