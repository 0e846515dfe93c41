// Host build of the bodies of k_plain_conv2d and k_gather_patch_exponents (cofhe_amd/csrc/plain_conv.hpp) with COFHE_HOSTSIM:
// the very functions the kernels run.  The convolution runs one simulated 16 x 16 workgroup per output tile, its two phases
// separated where the kernel has its barriers; the gather runs the threads of a small grid one after the other.
// TEST INFRASTRUCTURE ONLY; not linked into the product library.
#include "sim.cpp"       // COFHE_HOSTSIM and what conv.hpp needs of the device headers

#include "../../cofhe_amd/csrc/plain_conv.hpp"

namespace {
// shape14 = B, H, W, C, kh, kw, Co, sh, sw, ph, pw, dh, dw, groups
ConvShape shape_of(const uint32_t *a) {
    return ConvShape{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], 0u, 0u, a[11], a[12], a[13]};
}

template <int LMAX, bool FIXED>
void run(const ConvShape &s, const uint32_t *img, const uint32_t *w, uint32_t *out, uint32_t kbits) {
    const int L = FIXED ? LMAX : pmm_limbs(kbits);
    const uint32_t n = conv_rows(s), m = conv_inner(s), p = s.Co;
    std::vector<uint32_t> lds(2 * pmm_tile_words(PMM_MAX_LIMBS), 0xDEADBEEFu);
    for (uint32_t i0 = 0; i0 < n; i0 += PMM_TILE)
        for (uint32_t k0 = 0; k0 < p; k0 += PMM_TILE) {
            uint32_t acc[PMM_THREADS][LMAX] = {};
            for (uint32_t j0 = 0; j0 < m; j0 += PMM_TILE) {
                for (int tid = 0; tid < PMM_THREADS; tid++) pconv_stage<LMAX>(lds.data(), s, img, w, n, m, p, i0, k0, j0, tid, L, kbits);
                for (int tid = 0; tid < PMM_THREADS; tid++) pmm_accumulate<LMAX>(lds.data(), acc[tid], tid, L);
            }
            for (int tid = 0; tid < PMM_THREADS; tid++) {
                const uint32_t i = i0 + tid / PMM_TILE, k = k0 + tid % PMM_TILE;
                if (i < n && k < p) pmm_store<LMAX>(acc[tid], L, kbits, out + ((uint64_t)i * p + k) * PMM_REC_WORDS);
            }
        }
}

struct Piece16 {          // the uint4 of the device build
    uint32_t x, y, z, w;
};
}  // namespace

extern "C" {
// out [B, Ho, Wo, Co] = img [B, H, W, C] * w [kh, kw, C, Co] mod 2^kbits on exponent records, dispatched on the limb count as
// k_plain_conv2d does; returns 0, 1 for a geometry the launcher refuses, or -1 for a kbits it refuses
int plain_conv_sim(const uint32_t *shape14, const uint32_t *img, const uint32_t *w, uint32_t *out, uint32_t kbits) {
    ConvShape s = shape_of(shape14);
    if (conv_shape_check(s) || s.groups != 1) return 1;
    if (kbits == 0 || kbits > 32u * PMM_MAX_LIMBS) return -1;
    switch (pmm_limbs(kbits)) {
        case 1: run<1, true>(s, img, w, out, kbits); break;
        case 2: run<2, true>(s, img, w, out, kbits); break;
        case 3: run<3, true>(s, img, w, out, kbits); break;
        case 4: run<4, true>(s, img, w, out, kbits); break;
        case 5: run<5, true>(s, img, w, out, kbits); break;
        case 6: run<6, true>(s, img, w, out, kbits); break;
        case 7: run<7, true>(s, img, w, out, kbits); break;
        case 8: run<PMM_FIXED_LIMBS, true>(s, img, w, out, kbits); break;
        default: run<PMM_MAX_LIMBS, false>(s, img, w, out, kbits); break;
    }
    return 0;
}
int plain_conv_sim_tile(void) { return PMM_TILE; }

// out = S^T (m x n exponent records) of img, by a grid of `threads` threads; the piece is chosen as the launcher chooses it,
// from the two pointers.  Returns the piece size in bytes (16 or 4), or -1 for a geometry the launcher refuses
int plain_conv_sim_gather(const uint32_t *shape14, const uint32_t *img, uint32_t *out, uint32_t threads) {
    ConvShape s = shape_of(shape14);
    if (conv_shape_check(s) || s.groups != 1 || threads == 0) return -1;
    const uint32_t n = conv_rows(s), m = conv_inner(s);
    const bool vec16 = (((uintptr_t)img | (uintptr_t)out) & 15) == 0;
    for (uint32_t t = 0; t < threads; t++) {
        if (vec16)
            gather_exps_body(s, (const Piece16 *)img, (Piece16 *)out, n, m, (uint32_t)EXP_REC_WORDS / 4, (uint64_t)t, (uint64_t)threads);
        else
            gather_exps_body(s, img, out, n, m, (uint32_t)EXP_REC_WORDS, (uint64_t)t, (uint64_t)threads);
    }
    return vec16 ? 16 : 4;
}
}
