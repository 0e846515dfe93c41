// Host build of k_plain_divfloor's body (cofhe_amd/csrc/plain_div.hpp) on the lane-group simulator of sim.cpp: the very function
// the kernel runs, one call per element by the 8 host threads of a limb group as the kernel has one group per element.
// TEST INFRASTRUCTURE ONLY; not linked into the product library.
#include "sim.cpp"       // the lane-group simulator (run_group), COFHE_HOSTSIM, sim_status and sim_flags

#include "../../cofhe_amd/csrc/plain_div.hpp"

extern "C" {
// q[e] = floor(s(v[e]) / div[e mod n_div]) mod 2^kbits on exponent records; returns 0, or -1 for what the kernel's launcher
// refuses (kbits out of range, n_div = 0, n no multiple of n_div) with nothing written
int plain_div_sim(const uint32_t *v, const uint32_t *div, uint64_t n_div, uint32_t *q, uint64_t n, uint32_t kbits) {
    if (kbits == 0 || kbits > PDV_MAX_KBITS || n_div == 0 || n % n_div != 0) return -1;
    run_group([&](Ctx &c) {
        for (uint64_t e = 0; e < n; e++)
            plain_divfloor_element(c, v + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, q + e * PMM_REC_WORDS, kbits);
    });
    return 0;
}
int plain_div_sim_max_kbits(void) { return (int)PDV_MAX_KBITS; }
int plain_div_sim_groups(void) { return PDV_GROUPS; }
}
