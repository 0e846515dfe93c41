// conv.hip -- the kernels of cofhe_hip_conv2d_plain_ct_records and cofhe_hip_conv2d_grouped_plain_ct_records (launched by
// abi.hip, declared in kernels.hpp; the geometry and the level-0 body: conv.hpp).  k_conv_level0 is level 0 -> 1 of the matrix
// product's tree with its leaves read straight from the table of the IMAGE; k_gather_patches writes the patch matrix (im2col)
// for the route that runs the matrix product unchanged, and k_expand_group_filters the dense filter that route needs when the
// convolution has groups.
#include <hip/hip_runtime.h>

#include "conv.hpp"
#include "wg_ctx.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// One build: a level launch has thousands of workgroups, and the three-per-CU twins are for grids of at most 768.
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_conv_level0(ConvShape s, const uint32_t *__restrict__ table, const uint32_t *__restrict__ one_rec,
                                                                     const uint32_t *__restrict__ ent0, const uint32_t *__restrict__ off_cur,
                                                                     const uint32_t *__restrict__ off_next, const uint32_t *__restrict__ map_next,
                                                                     uint32_t n_next, uint32_t row0, uint32_t rows, uint32_t tw,
                                                                     uint32_t *__restrict__ dst, const uint32_t *__restrict__ absdelta, int half_dbits,
                                                                     uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_CTX_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    conv_level0_body(c, blockIdx.x, s, table, one_rec, ent0, off_cur, off_next, map_next, n_next, row0, rows, tw, dst, dd);
}

// out[(row m + j) 2 + h] = cts[conv_leaf(row, j) 2 + h], or the principal form in the padding, for row < n, j < m: records of
// `pieces` pieces of type T (16 bytes, or a dword).  Consecutive threads take consecutive pieces of one OUTPUT record.
template <typename T>
__device__ __forceinline__ void gather_body(const ConvShape &s, const T *__restrict__ cts, const T *__restrict__ one_rec, T *__restrict__ out,
                                            uint32_t n, uint32_t m, uint32_t pieces) {
    const uint64_t total = (uint64_t)n * m * 2 * pieces;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = idx / pieces;
        const uint32_t t = (uint32_t)(idx - e * pieces), h = (uint32_t)(e & 1u);
        const uint64_t row = (e >> 1) / m;
        const int64_t leaf = conv_leaf(s, (uint32_t)row, (uint32_t)((e >> 1) - row * m));
        out[idx] = leaf < 0 ? one_rec[t] : cts[((uint64_t)leaf * 2 + h) * pieces + t];
    }
}
// vec16: the launcher found cts and out 16-byte aligned (one_rec, the context's own record, always is)
__global__ void __launch_bounds__(256) k_gather_patches(ConvShape s, const uint32_t *__restrict__ cts, const uint32_t *__restrict__ one_rec,
                                                        uint32_t *__restrict__ out, uint32_t n, uint32_t m, uint32_t vec16) {
    if (vec16)
        gather_body(s, (const uint4 *)cts, (const uint4 *)one_rec, (uint4 *)out, n, m, (uint32_t)REC_WORDS / 4);
    else
        gather_body(s, cts, one_rec, out, n, m, (uint32_t)REC_WORDS);
}


// dense[(t C + c) Co + co] = w[(t Cg + c % Cg) Co + co] when channel c lies in the group of column co (c / Cg == co / Cog), else
// the zero exponent, for t < taps = kh kw: exponent records of `pieces` pieces of type T.  Consecutive threads take consecutive
// pieces of one OUTPUT record.
template <typename T>
__device__ __forceinline__ void expand_body(const T *__restrict__ w, T *__restrict__ dense, uint32_t taps, uint32_t C, uint32_t Co, uint32_t groups,
                                            uint32_t pieces) {
    const uint32_t Cg = C / groups, Cog = Co / groups;
    const uint64_t total = (uint64_t)taps * C * Co * pieces;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t e = idx / pieces;
        const uint32_t piece = (uint32_t)(idx - e * pieces), co = (uint32_t)(e % Co);
        const uint64_t tc = e / Co;
        const uint32_t c = (uint32_t)(tc % C), t = (uint32_t)(tc / C);
        T v{};
        if (c / Cg == co / Cog) v = w[(((uint64_t)t * Cg + c % Cg) * Co + co) * pieces + piece];
        dense[idx] = v;
    }
}
// vec16: the launcher found w 16-byte aligned (dense, a block of the block cache, always is)
__global__ void __launch_bounds__(256) k_expand_group_filters(const uint32_t *__restrict__ w, uint32_t *__restrict__ dense, uint32_t taps, uint32_t C,
                                                              uint32_t Co, uint32_t groups, uint32_t vec16) {
    if (vec16)
        expand_body((const uint4 *)w, (uint4 *)dense, taps, C, Co, groups, (uint32_t)EXP_REC_WORDS / 4);
    else
        expand_body(w, dense, taps, C, Co, groups, (uint32_t)EXP_REC_WORDS);
}

}  // namespace cofhe_k
