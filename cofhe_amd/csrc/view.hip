// view.hip -- the two kernels that rearrange resident tensors (launched by abi.hip, declared in kernels.hpp; the index
// arithmetic: view.hpp).  k_view_records writes the box of an affine view, k_gather_records the records an index array names.
// Both are pure data movement on records of `words` dwords: no composition runs, and only the gather touches the status word, for
// an index beyond its source.
//
// The lane mapping is k_lut_select's where the record is long enough: a record of 64 pieces or more (a ciphertext is 84
// sixteen-byte pieces, a form 42 -- the latter falls below and takes the short form) belongs to ONE wavefront, whose record index
// is made wave-uniform with readfirstlane, so that the decode of the coordinates and the 8 x 8 map run once per wavefront on
// scalar registers and the lanes then move the contiguous record, lane l taking pieces l, l + 64, ...  A shorter record belongs
// to eight lanes, so that a wavefront still issues full-width loads over eight records at once (an exponent record is 8
// sixteen-byte pieces: one per lane); there the decode runs per lane.
#include <hip/hip_runtime.h>

#include "view.hpp"

using namespace cofhe;

namespace cofhe_k {

namespace {
// the first record of this thread and the step of the grid-stride loop; `sub` is the thread's place among the `lanes` that share
// a record.  wave: one wavefront per record, the index uniform over it.
template <bool WAVE>
__device__ __forceinline__ void view_slot(uint64_t &first, uint64_t &step, uint32_t &sub, uint32_t &lanes) {
    if (WAVE) {
        const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        first = (uint64_t)blockIdx.x * VIEW_WAVES + wave;
        step = (uint64_t)gridDim.x * VIEW_WAVES;
        sub = threadIdx.x & 63u;
        lanes = 64u;
    } else {
        first = (uint64_t)blockIdx.x * (VIEW_THREADS / VIEW_GROUP) + threadIdx.x / VIEW_GROUP;
        step = (uint64_t)gridDim.x * (VIEW_THREADS / VIEW_GROUP);
        sub = threadIdx.x % VIEW_GROUP;
        lanes = VIEW_GROUP;
    }
}

template <typename T, bool WAVE>
__device__ __forceinline__ void view_body(const cofhe_hip_view &v, const T *__restrict__ src, const T *__restrict__ fill, T *__restrict__ dst,
                                          uint32_t pieces) {
    uint64_t n_box = 1;
#pragma unroll
    for (int d = 0; d < VIEW_MAX_DIMS; d++)
        if ((uint32_t)d < v.out_ndim) n_box *= v.out_extent[d];
    uint64_t first, step;
    uint32_t sub, lanes;
    view_slot<WAVE>(first, step, sub, lanes);
    for (uint64_t i = first; i < n_box; i += step) {
        uint64_t s = 0;
        const bool inside = view_source(v, i, &s);
        const T *from = inside ? src + s * pieces : fill;
        T *to = dst + view_dest(v, i) * pieces;
        for (uint32_t p = sub; p < pieces; p += lanes) to[p] = from[p];
    }
}

template <typename T, bool WAVE>
__device__ __forceinline__ void gather_body(const T *__restrict__ src, uint64_t n_src, const uint32_t *__restrict__ index, const T *__restrict__ fill,
                                            T *__restrict__ dst, uint64_t n_out, uint32_t pieces, uint32_t *__restrict__ status) {
    uint64_t first, step;
    uint32_t sub, lanes;
    view_slot<WAVE>(first, step, sub, lanes);
    for (uint64_t i = first; i < n_out; i += step) {
        const uint32_t ix = index[i];
        if (ix == COFHE_HIP_GATHER_KEEP) continue;
        const T *from = fill;
        if (ix < n_src)
            from = src + (uint64_t)ix * pieces;
        else if (ix != COFHE_HIP_GATHER_FILL && sub == 0)
            atomicOr(status, CF_ST_BAD_INDEX);
        if (!from) continue;                                  // no fill record: the output stays as it is
        T *to = dst + i * pieces;
        for (uint32_t p = sub; p < pieces; p += lanes) to[p] = from[p];
    }
}
}  // namespace

// vec16: the launcher found src, fill and dst 16-byte aligned and words a multiple of 4
__global__ void __launch_bounds__(VIEW_THREADS) k_view_records(cofhe_hip_view v, const uint32_t *__restrict__ src, const uint32_t *__restrict__ fill,
                                                               uint32_t *__restrict__ dst, uint32_t words, uint32_t vec16) {
    if (vec16) {
        if (words / 4 >= 64u)
            view_body<uint4, true>(v, (const uint4 *)src, (const uint4 *)fill, (uint4 *)dst, words / 4);
        else
            view_body<uint4, false>(v, (const uint4 *)src, (const uint4 *)fill, (uint4 *)dst, words / 4);
    } else if (words >= 64u) {
        view_body<uint32_t, true>(v, src, fill, dst, words);
    } else {
        view_body<uint32_t, false>(v, src, fill, dst, words);
    }
}

__global__ void __launch_bounds__(VIEW_THREADS) k_gather_records(const uint32_t *__restrict__ src, uint64_t n_src, const uint32_t *__restrict__ index,
                                                                 const uint32_t *__restrict__ fill, uint32_t *__restrict__ dst, uint64_t n_out,
                                                                 uint32_t words, uint32_t vec16, uint32_t *__restrict__ status) {
    if (vec16) {
        if (words / 4 >= 64u)
            gather_body<uint4, true>((const uint4 *)src, n_src, index, (const uint4 *)fill, (uint4 *)dst, n_out, words / 4, status);
        else
            gather_body<uint4, false>((const uint4 *)src, n_src, index, (const uint4 *)fill, (uint4 *)dst, n_out, words / 4, status);
    } else if (words >= 64u) {
        gather_body<uint32_t, true>(src, n_src, index, fill, dst, n_out, words, status);
    } else {
        gather_body<uint32_t, false>(src, n_src, index, fill, dst, n_out, words, status);
    }
}

}  // namespace cofhe_k
