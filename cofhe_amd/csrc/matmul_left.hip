// matmul_left.hip -- what the plaintext-left matrix product W . [x] and the matrix Beaver triplets add on the device
// (launched by abi.hip, declared in kernels.hpp): the transpose of a matrix of fixed-size records, with which
// cofhe_hip_matmul_plain_ct_records runs the ciphertext-left product on transposed views, and the plaintext matrix product
// mod 2^k of cofhe_hip_matmul_plain_plain_records (its body: plain_mm.hpp).  Neither touches a form's arithmetic.
#include <hip/hip_runtime.h>

#include "plain_mm.hpp"

using namespace cofhe;

namespace cofhe_k {

// out[c * rows + r] = in[r * cols + c] for elements of `words` 32-bit words.  Consecutive threads take consecutive pieces
// of one OUTPUT element, so an element is read and written contiguously; T is the piece (16 bytes, or a dword)
template <typename T>
__device__ __forceinline__ void transpose_body(const T *__restrict__ in, T *__restrict__ out, uint32_t rows, uint32_t cols, uint32_t pieces) {
    const uint64_t total = (uint64_t)rows * cols * pieces;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = idx / pieces;
        const uint32_t t = (uint32_t)(idx - e * pieces);
        const uint64_t c = e / rows, r = e - c * rows;
        out[idx] = in[(r * cols + c) * pieces + t];
    }
}
// vec16: the launcher found both pointers 16-byte aligned and words a multiple of 4
__global__ void __launch_bounds__(256) k_transpose_records(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, uint32_t rows, uint32_t cols,
                                                           uint32_t words, uint32_t vec16) {
    if (vec16)
        transpose_body((const uint4 *)in, (uint4 *)out, rows, cols, words / 4);
    else
        transpose_body(in, out, rows, cols, words);
}

// one 16 x 16 output tile per workgroup (plain_mm.hpp); L limbs, a compile-time count when FIXED
template <int LMAX, bool FIXED>
__device__ __forceinline__ void plain_matmul_body(uint32_t *lds, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                  uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t p, uint32_t kbits) {
    const int L = FIXED ? LMAX : pmm_limbs(kbits);
    const int tid = (int)threadIdx.x;
    const uint32_t i0 = blockIdx.y * PMM_TILE, k0 = blockIdx.x * PMM_TILE;
    uint32_t acc[LMAX];
#pragma unroll
    for (int l = 0; l < LMAX; l++) acc[l] = 0;
    for (uint32_t j0 = 0; j0 < m; j0 += PMM_TILE) {          // uniform over the workgroup: everybody meets both barriers
        pmm_stage<LMAX>(lds, a, b, n, m, p, i0, k0, j0, tid, L, kbits);
        __syncthreads();
        pmm_accumulate<LMAX>(lds, acc, tid, L);
        __syncthreads();
    }
    const uint32_t i = i0 + tid / PMM_TILE, k = k0 + tid % PMM_TILE;
    if (i < n && k < p) pmm_store<LMAX>(acc, L, kbits, out + ((uint64_t)i * p + k) * PMM_REC_WORDS);
}
// out (n x p) = a (n x m) . b (m x p) mod 2^kbits on exponent records, 1 <= kbits <= 32 PMM_MAX_LIMBS; grid (ceil(p/16), ceil(n/16))
__global__ void __launch_bounds__(PMM_THREADS) k_plain_matmul(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                              uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t p, uint32_t kbits) {
    __shared__ uint32_t lds[2 * pmm_tile_words(PMM_MAX_LIMBS)];
    switch (pmm_limbs(kbits)) {
        case 1: plain_matmul_body<1, true>(lds, a, b, out, n, m, p, kbits); break;
        case 2: plain_matmul_body<2, true>(lds, a, b, out, n, m, p, kbits); break;
        case 3: plain_matmul_body<3, true>(lds, a, b, out, n, m, p, kbits); break;
        case 4: plain_matmul_body<4, true>(lds, a, b, out, n, m, p, kbits); break;
        case 5: plain_matmul_body<5, true>(lds, a, b, out, n, m, p, kbits); break;
        case 6: plain_matmul_body<6, true>(lds, a, b, out, n, m, p, kbits); break;
        case 7: plain_matmul_body<7, true>(lds, a, b, out, n, m, p, kbits); break;
        case 8: plain_matmul_body<PMM_FIXED_LIMBS, true>(lds, a, b, out, n, m, p, kbits); break;
        default: plain_matmul_body<PMM_MAX_LIMBS, false>(lds, a, b, out, n, m, p, kbits); break;
    }
}

}  // namespace cofhe_k
