// conv_ct.hip -- what the convolution with ciphertext filters and its Beaver triplet add on the device (launched by abi.hip,
// declared in kernels.hpp; the bodies: plain_conv.hpp): the convolution of a PLAINTEXT image with plaintext filters mod 2^k of
// cofhe_hip_conv2d_plain_plain_records, an implicit GEMM on the tile of the plaintext matrix product, and the transposed patch
// matrix of a plaintext image with which cofhe_hip_conv2d_ct_filters_records runs the product of
// cofhe_hip_matmul_plain_ct_records.  Neither touches a form's arithmetic.
#include <hip/hip_runtime.h>

#include "plain_conv.hpp"

using namespace cofhe;

namespace cofhe_k {

// one 16 x 16 output tile per workgroup (plain_mm.hpp), the left tile staged through conv_leaf; L limbs, a compile-time count
// when FIXED.  Row tiles along x (n = B Ho Wo outgrows the 65535 of the other grid dimensions long before Co does)
template <int LMAX, bool FIXED>
__device__ __forceinline__ void plain_conv2d_body(uint32_t *lds, const ConvShape &s, const uint32_t *__restrict__ img, const uint32_t *__restrict__ w,
                                                  uint32_t *__restrict__ out, uint32_t kbits) {
    const int L = FIXED ? LMAX : pmm_limbs(kbits);
    const int tid = (int)threadIdx.x;
    const uint32_t n = conv_rows(s), m = conv_inner(s), p = s.Co;
    const uint32_t i0 = blockIdx.x * PMM_TILE, k0 = blockIdx.y * PMM_TILE;
    uint32_t acc[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; l++) acc[l] = 0;
    for (uint32_t j0 = 0; j0 < m; j0 += PMM_TILE) {          // uniform over the workgroup: everybody meets both barriers
        pconv_stage<LMAX>(lds, s, img, w, n, m, p, i0, k0, j0, tid, L, kbits);
        __syncthreads();
        pmm_accumulate<LMAX>(lds, acc, tid, L);
        __syncthreads();
    }
    const uint32_t i = i0 + tid / PMM_TILE, k = k0 + tid % PMM_TILE;
    if (i < n && k < p) pmm_store<LMAX>(acc, L, kbits, out + ((uint64_t)i * p + k) * PMM_REC_WORDS);
}
// out [B, Ho, Wo, Co] = img [B, H, W, C] * w [kh, kw, C, Co] mod 2^kbits on exponent records, groups = 1, 1 <= kbits <=
// 32 PMM_MAX_LIMBS; grid (ceil(n/16), ceil(Co/16)).  The limb-count dispatch is k_plain_matmul's
__global__ void __launch_bounds__(PMM_THREADS) k_plain_conv2d(ConvShape s, const uint32_t *__restrict__ img, const uint32_t *__restrict__ w,
                                                              uint32_t *__restrict__ out, uint32_t kbits) {
    __shared__ uint32_t lds[2 * pmm_tile_words(PMM_MAX_LIMBS)];
    switch (pmm_limbs(kbits)) {
        case 1: plain_conv2d_body<1, true>(lds, s, img, w, out, kbits); break;
        case 2: plain_conv2d_body<2, true>(lds, s, img, w, out, kbits); break;
        case 3: plain_conv2d_body<3, true>(lds, s, img, w, out, kbits); break;
        case 4: plain_conv2d_body<4, true>(lds, s, img, w, out, kbits); break;
        case 5: plain_conv2d_body<5, true>(lds, s, img, w, out, kbits); break;
        case 6: plain_conv2d_body<6, true>(lds, s, img, w, out, kbits); break;
        case 7: plain_conv2d_body<7, true>(lds, s, img, w, out, kbits); break;
        case 8: plain_conv2d_body<PMM_FIXED_LIMBS, true>(lds, s, img, w, out, kbits); break;
        default: plain_conv2d_body<PMM_MAX_LIMBS, false>(lds, s, img, w, out, kbits); break;
    }
}

// S^T (m x n exponent records) of the plaintext image img, zero records in the padding (plain_conv.hpp).  vec16: the launcher
// found img and out 16-byte aligned
__global__ void __launch_bounds__(256) k_gather_patch_exponents(ConvShape s, const uint32_t *__restrict__ img, uint32_t *__restrict__ out, uint32_t n,
                                                                uint32_t m, uint32_t vec16) {
    const uint64_t first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, step = (uint64_t)gridDim.x * blockDim.x;
    if (vec16)
        gather_exps_body(s, (const uint4 *)img, (uint4 *)out, n, m, (uint32_t)EXP_REC_WORDS / 4, first, step);
    else
        gather_exps_body(s, img, out, n, m, (uint32_t)EXP_REC_WORDS, first, step);
}

}  // namespace cofhe_k
