// divide_exact.hip -- the kernels of the exact floor division of ciphertexts by small public divisors from one opened value
// (launched by abi.hip, declared in kernels.hpp; the protocol and the bodies: plain_divmod.hpp).  k_plain_divmod is
// k_plain_divfloor that keeps the remainder; k_divx_prep and k_divx_rows write the plaintext rows of the exact-division tuples,
// the quotient of each element's mask plus the carry of the two remainders for every remainder the opened value can have;
// k_divx_select closes the division by copying the one tuple entry that the opened value's remainder names.
// cofhe_hip_divx_close_records runs the plaintext addend of the comb on its output.
#include <hip/hip_runtime.h>

#include "layout.hpp"
#include "plain_divmod.hpp"

using namespace cofhe;

namespace cofhe_k {

// the context of one limb group per element without a workgroup protocol (as k_plain_divfloor): the LDS is the groups' slices,
// which only mp_divrem touches
__device__ __forceinline__ Ctx divx_group_ctx(uint32_t *lds, uint32_t *status) {
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    c.status = status;
    return c;
}

// q[e] = floor(s(v[e]) / D) mod 2^kbits and rem[e] = s(v[e]) - D q(v[e]) for D = div[e mod n_div], e < n: one limb group per
// element; n_div >= 1, 1 <= kbits <= PDV_MAX_KBITS, 1 <= rows <= DIVX_MAX_ROWS; q and rem must not overlap v or div.  An invalid
// divisor, one above rows included: quotient 0, remainder 0 and CF_ST_DIV_CAP in *status.
__global__ void __launch_bounds__(PDV_THREADS) k_plain_divmod(const uint32_t *__restrict__ v, const uint32_t *__restrict__ div, uint64_t n_div,
                                                              uint32_t *__restrict__ q, uint32_t *__restrict__ rem, uint64_t n, uint32_t rows,
                                                              uint32_t kbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[PDV_GROUPS * SCRATCH_WORDS];
    Ctx c = divx_group_ctx(lds, status);
    const uint64_t e = (uint64_t)blockIdx.x * PDV_GROUPS + threadIdx.x / G;
    if (e >= n) return;
    plain_divmod_element(c, v + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, q + e * PMM_REC_WORDS, rem + e, rows, kbits);
}

// prep[e] = q(r[e]) | q(r[e]) + 1 mod 2^kbits | (D - m(r[e]), D, 0 ..) for D = div[e mod n_div], e < n: the divmod pass of the
// rows, launched like k_plain_divmod; an invalid divisor leaves three zero records and CF_ST_DIV_CAP in *status
__global__ void __launch_bounds__(PDV_THREADS) k_divx_prep(const uint32_t *__restrict__ r, const uint32_t *__restrict__ div, uint64_t n_div,
                                                           uint32_t *__restrict__ prep, uint64_t n, uint32_t rows, uint32_t kbits,
                                                           uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[PDV_GROUPS * SCRATCH_WORDS];
    Ctx c = divx_group_ctx(lds, status);
    const uint64_t e = (uint64_t)blockIdx.x * PDV_GROUPS + threadIdx.x / G;
    if (e >= n) return;
    divx_prep_element(c, r + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, prep + e * DIVX_PREP_WORDS, rows, kbits);
}

// out[i rows + j] = T_j of element i for j < D_i and the zero record for D_i <= j < rows, i < n, on exponent records: pure data
// movement from the blocks of k_divx_prep, a grid-stride loop over pieces (divx_rows_piece).  vec16: the launcher found out
// 16-byte aligned (prep is a block of the block cache and always is); out must not overlap prep
__global__ void __launch_bounds__(DIVX_ROWS_THREADS) k_divx_rows(const uint32_t *__restrict__ prep, uint32_t *__restrict__ out, uint64_t n,
                                                                 uint32_t rows, uint32_t vec16) {
    const uint64_t total = n * rows * (vec16 ? (uint64_t)PMM_REC_WORDS / 4 : (uint64_t)PMM_REC_WORDS);
    for (uint64_t idx = (uint64_t)blockIdx.x * DIVX_ROWS_THREADS + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * DIVX_ROWS_THREADS) {
        if (vec16)
            divx_rows_piece<4>(prep, out, idx, rows);
        else
            divx_rows_piece<1>(prep, out, idx, rows);
    }
}

// out[i] = tuples[i rows + index[i]] for i < n: ciphertexts of `pieces` pieces of type T.  One wavefront per output ciphertext, as
// select_body of lut.hip: its lanes read the same word index[i] (one address: a uniform read), and then move the 1344 contiguous
// bytes of the entry, lane l taking pieces l, l + 64, ..: 84 sixteen-byte pieces in two passes, or 336 dwords in six.  The entry
// index is computed in 64 bits; an index of rows or more reads entry 0 and sets CF_ST_DIV_CAP.  The grid strides over the
// elements beyond 2^31 wavefronts' worth of them.
template <typename T>
__device__ __forceinline__ void divx_select_body(const uint32_t *__restrict__ index, const T *__restrict__ tuples, T *__restrict__ out, uint64_t n,
                                                 uint32_t rows, uint32_t pieces, uint32_t *__restrict__ status) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t i = (uint64_t)blockIdx.x * DIVX_SELECT_WAVES + threadIdx.x / 64; i < n; i += (uint64_t)gridDim.x * DIVX_SELECT_WAVES) {
        bool bad;
        const uint64_t entry = divx_entry(i, rows, index[i], &bad);
        if (bad && lane == 0 && status) atomicOr(status, CF_ST_DIV_CAP);
        const T *src = tuples + entry * pieces;
        T *dst = out + i * pieces;
        for (uint32_t p = lane; p < pieces; p += 64u) dst[p] = src[p];
    }
}
// vec16: the launcher found tuples and out 16-byte aligned (index is read a word at a time either way)
__global__ void __launch_bounds__(DIVX_SELECT_THREADS) k_divx_select(const uint32_t *__restrict__ index, const uint32_t *__restrict__ tuples,
                                                                     uint32_t *__restrict__ out, uint64_t n, uint32_t rows, uint32_t vec16,
                                                                     uint32_t *__restrict__ status) {
    if (vec16)
        divx_select_body(index, (const uint4 *)tuples, (uint4 *)out, n, rows, 2u * REC_WORDS / 4, status);
    else
        divx_select_body(index, tuples, out, n, rows, 2u * REC_WORDS, status);
}

}  // namespace cofhe_k
