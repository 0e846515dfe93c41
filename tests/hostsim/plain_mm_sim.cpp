// Host build of the plaintext matrix product's body (cofhe_amd/csrc/plain_mm.hpp) with COFHE_HOSTSIM: the very functions
// k_plain_matmul runs, one simulated 16 x 16 workgroup per output tile, its two phases separated where the kernel has its
// barriers.  TEST INFRASTRUCTURE ONLY; not linked into the product library.
#define COFHE_HOSTSIM 1
#include <vector>

#include "../../cofhe_amd/csrc/plain_mm.hpp"

using namespace cofhe;

namespace {
template <int LMAX, bool FIXED>
void run(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, uint32_t m, uint32_t p, uint32_t kbits) {
    const int L = FIXED ? LMAX : pmm_limbs(kbits);
    std::vector<uint32_t> lds(2 * pmm_tile_words(PMM_MAX_LIMBS), 0xDEADBEEFu);
    for (uint32_t i0 = 0; i0 < n; i0 += PMM_TILE)
        for (uint32_t k0 = 0; k0 < p; k0 += PMM_TILE) {
            uint32_t acc[PMM_THREADS][LMAX] = {};
            for (uint32_t j0 = 0; j0 < m; j0 += PMM_TILE) {
                for (int tid = 0; tid < PMM_THREADS; tid++) pmm_stage<LMAX>(lds.data(), a, b, n, m, p, i0, k0, j0, tid, L, kbits);
                for (int tid = 0; tid < PMM_THREADS; tid++) pmm_accumulate<LMAX>(lds.data(), acc[tid], tid, L);
            }
            for (int tid = 0; tid < PMM_THREADS; tid++) {
                const uint32_t i = i0 + tid / PMM_TILE, k = k0 + tid % PMM_TILE;
                if (i < n && k < p) pmm_store<LMAX>(acc[tid], L, kbits, out + ((uint64_t)i * p + k) * PMM_REC_WORDS);
            }
        }
}
}  // namespace

extern "C" {
// out (n x p) = a (n x m) . b (m x p) mod 2^kbits on exponent records, dispatched on the limb count as k_plain_matmul does;
// returns 0, or -1 for a kbits the kernel's launcher refuses
int plain_mm_sim(const uint32_t *a, const uint32_t *b, uint32_t *out, uint32_t n, uint32_t m, uint32_t p, uint32_t kbits) {
    if (kbits == 0 || kbits > 32u * PMM_MAX_LIMBS) return -1;
    switch (pmm_limbs(kbits)) {
        case 1: run<1, true>(a, b, out, n, m, p, kbits); break;
        case 2: run<2, true>(a, b, out, n, m, p, kbits); break;
        case 3: run<3, true>(a, b, out, n, m, p, kbits); break;
        case 4: run<4, true>(a, b, out, n, m, p, kbits); break;
        case 5: run<5, true>(a, b, out, n, m, p, kbits); break;
        case 6: run<6, true>(a, b, out, n, m, p, kbits); break;
        case 7: run<7, true>(a, b, out, n, m, p, kbits); break;
        case 8: run<PMM_FIXED_LIMBS, true>(a, b, out, n, m, p, kbits); break;
        default: run<PMM_MAX_LIMBS, false>(a, b, out, n, m, p, kbits); break;
    }
    return 0;
}
int plain_mm_sim_tile(void) { return PMM_TILE; }
}
