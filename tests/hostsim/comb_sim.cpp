// Host build of the comb's digit recoding and slot map (cofhe_amd/csrc/comb.hpp) with COFHE_HOSTSIM: the very functions
// k_comb_first runs, called from the CPU tests.  TEST INFRASTRUCTURE ONLY; not linked into the product library.
#define COFHE_HOSTSIM 1
#include <cstring>

#include "../../cofhe_amd/csrc/comb.hpp"

using namespace cofhe;

extern "C" {
// digits[j] = comb_digit(e, j, w, nbits), j < npos
void comb_sim_digits(const uint32_t *e, int w, int nbits, int npos, int32_t *digits) {
    for (int j = 0; j < npos; j++) digits[j] = comb_digit(e, j, w, nbits);
}
// every slot of a column: sel[4 s .. 4 s + 3] = table, position, signed digit, entry record (tables only, else 0)
void comb_sim_slots(uint32_t w, uint32_t npos_r, uint32_t npos_m, uint32_t leaf, uint32_t halves, uint32_t kbits, uint32_t h,
                    const uint32_t *r_exp, const uint32_t *m_exp, int32_t *sel, uint32_t *n_slots) {
    const CombShape s{w, npos_r, npos_m, leaf, halves, kbits};
    *n_slots = comb_slots(s);
    for (uint32_t k = 0; k < comb_slots(s); k++) {
        const CombSel c = comb_select(s, h, k, r_exp, m_exp);
        sel[4 * k + 0] = c.table;
        sel[4 * k + 1] = c.pos;
        sel[4 * k + 2] = c.digit;
        sel[4 * k + 3] = (c.table >= 0 && c.table <= 2) ? (int32_t)comb_entry(s, c) : 0;
    }
}
}
