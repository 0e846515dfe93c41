// lut.hip -- the two kernels of a table lookup on ciphertext tensors from one opened value (launched by abi.hip, declared in
// kernels.hpp; the index arithmetic: lut.hpp).  k_lut_rotate writes the plaintext rows of the lookup tuples, the public table
// rotated by each element's mask; k_lut_select closes the lookup by copying the one tuple entry that the opened value names.
// Both are pure data movement: no composition runs, and neither touches the status word.
#include <hip/hip_runtime.h>

#include "layout.hpp"
#include "lut.hpp"

using namespace cofhe;

namespace cofhe_k {

// out[i 2^bits + j] = table[(i mod n_tab) 2^bits + ((j + r_i) mod 2^bits)], r_i the index of r[i], for i < n, j < 2^bits:
// exponent records of `pieces` pieces of type T (16 bytes, or a dword).  Consecutive threads take consecutive pieces of one
// OUTPUT record, so the stores are contiguous throughout and, j running fastest, so are the loads up to the wrap of a row (one
// break per row).  With 16-byte pieces a wavefront covers 8 records of one row (a row of 8 entries or more), so the two words it
// reads of r[i] are one address for all 64 lanes.
template <typename T>
__device__ __forceinline__ void rotate_body(const T *__restrict__ table, uint64_t n_tab, const uint32_t *__restrict__ r, T *__restrict__ out,
                                            uint64_t n, uint32_t bits, uint32_t pieces) {
    const uint64_t total = (n << bits) * pieces;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t rec = idx / pieces, i = rec >> bits;
        const uint32_t piece = (uint32_t)(idx - rec * pieces), j = (uint32_t)(rec - (i << bits));
        const uint32_t src = lut_rotated_source(j, lut_index(r + i * PMM_REC_WORDS, bits), bits);
        out[idx] = table[((((i % n_tab) << bits) + src) * pieces) + piece];
    }
}
// vec16: the launcher found table and out 16-byte aligned (r is read a word at a time either way)
__global__ void __launch_bounds__(256) k_lut_rotate(const uint32_t *__restrict__ table, uint64_t n_tab, const uint32_t *__restrict__ r,
                                                    uint32_t *__restrict__ out, uint64_t n, uint32_t bits, uint32_t vec16) {
    if (vec16)
        rotate_body((const uint4 *)table, n_tab, r, (uint4 *)out, n, bits, (uint32_t)PMM_REC_WORDS / 4);
    else
        rotate_body(table, n_tab, r, out, n, bits, (uint32_t)PMM_REC_WORDS);
}

// out[i] = tuples[i 2^bits + (e_i mod 2^bits)], e_i the index of e[i], for i < n: ciphertexts of `pieces` pieces of type T.  One
// wavefront per output ciphertext: its lanes read the same two words of e[i] (one address: a uniform read), and then move the
// 1344 contiguous bytes of the entry, lane l taking pieces l, l + 64, ..: 84 sixteen-byte pieces in two passes, or 336 dwords in
// six.  The grid strides over the elements beyond 2^31 wavefronts' worth of them.
template <typename T>
__device__ __forceinline__ void select_body(const uint32_t *__restrict__ e, const T *__restrict__ tuples, T *__restrict__ out, uint64_t n,
                                            uint32_t bits, uint32_t pieces) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * LUT_SELECT_WAVES + threadIdx.x / 64; i < n; i += (uint64_t)gridDim.x * LUT_SELECT_WAVES) {
        const uint64_t entry = (i << bits) + lut_index(e + i * PMM_REC_WORDS, bits);
        const T *src = tuples + entry * pieces;
        T *dst = out + i * pieces;
        for (uint32_t p = lane; p < pieces; p += 64u) dst[p] = src[p];
    }
}
// vec16: the launcher found tuples and out 16-byte aligned (e is read a word at a time either way)
__global__ void __launch_bounds__(LUT_SELECT_THREADS) k_lut_select(const uint32_t *__restrict__ e, const uint32_t *__restrict__ tuples,
                                                                   uint32_t *__restrict__ out, uint64_t n, uint32_t bits, uint32_t vec16) {
    if (vec16)
        select_body(e, (const uint4 *)tuples, (uint4 *)out, n, bits, 2u * REC_WORDS / 4);
    else
        select_body(e, tuples, out, n, bits, 2u * REC_WORDS);
}

}  // namespace cofhe_k
