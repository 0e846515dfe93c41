// Host build of the bodies of k_plain_divmod, k_divx_prep and k_divx_rows (cofhe_amd/csrc/plain_divmod.hpp) on the lane-group
// simulator of sim.cpp: the very functions the kernels run, one call per element by the 8 host threads of a limb group as the
// kernels have one group per element, and the store pass piece by piece as its grid-stride loop visits them.
// TEST INFRASTRUCTURE ONLY; not linked into the product library.
#include "sim.cpp"       // the lane-group simulator (run_group), COFHE_HOSTSIM, sim_status and sim_flags

#include "../../cofhe_amd/csrc/plain_divmod.hpp"

namespace {
bool refused(uint32_t kbits, uint32_t rows, uint64_t n_div, uint64_t n) {
    return kbits == 0 || kbits > PDV_MAX_KBITS || rows == 0 || rows > DIVX_MAX_ROWS || n_div == 0 || n % n_div != 0;
}
}  // namespace

extern "C" {
// q[e] = floor(s(v[e]) / D) mod 2^kbits on exponent records and rem[e] = s(v[e]) - D q(v[e]), D = div[e mod n_div]; returns 0,
// or -1 for what the kernel's launcher refuses with nothing written
int divx_divmod_sim(const uint32_t *v, const uint32_t *div, uint64_t n_div, uint32_t *q, uint32_t *rem, uint64_t n, uint32_t rows,
                    uint32_t kbits) {
    if (refused(kbits, rows, n_div, n)) return -1;
    run_group([&](Ctx &c) {
        for (uint64_t e = 0; e < n; e++)
            plain_divmod_element(c, v + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, q + e * PMM_REC_WORDS, rem + e, rows, kbits);
    });
    return 0;
}
// out[i rows + j] = T_j of element i: the divmod pass into a buffer prefilled with a pattern (every word of a block must be
// written), then every piece of the store pass, of `width` words (4 or 1)
int divx_rows_sim(const uint32_t *r, const uint32_t *div, uint64_t n_div, uint32_t *out, uint64_t n, uint32_t rows, uint32_t kbits,
                  uint32_t width) {
    if (refused(kbits, rows, n_div, n) || (width != 1 && width != 4)) return -1;
    std::vector<uint32_t> prep(n * DIVX_PREP_WORDS, 0xA5A5A5A5u);
    run_group([&](Ctx &c) {
        for (uint64_t e = 0; e < n; e++)
            divx_prep_element(c, r + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, prep.data() + e * DIVX_PREP_WORDS, rows, kbits);
    });
    const uint64_t total = n * rows * (PMM_REC_WORDS / width);
    for (uint64_t idx = 0; idx < total; idx++) {
        if (width == 4)
            divx_rows_piece<4>(prep.data(), out, idx, rows);
        else
            divx_rows_piece<1>(prep.data(), out, idx, rows);
    }
    return 0;
}
// the entry that k_divx_select reads for element i, and whether it flagged the index
uint64_t divx_entry_sim(uint64_t i, uint32_t rows, uint32_t index, int *bad) {
    bool b;
    const uint64_t e = divx_entry(i, rows, index, &b);
    *bad = b ? 1 : 0;
    return e;
}
int divx_sim_max_rows(void) { return (int)DIVX_MAX_ROWS; }
}
