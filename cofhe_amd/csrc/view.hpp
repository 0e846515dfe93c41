// view.hpp -- the index arithmetic of k_view_records (view.hip): rearranging resident tensors by an affine view, in a header
// that includes no HIP header, so that the host build of the CPU tests (tests/hostsim/view_sim.cpp, g++) compiles the very code
// the kernel runs, and so does the host half of abi.hip (the validator and the builders of the descriptors).
//
// A view (cofhe_hip_view, include/cofhe_hip.h) produces a box of out_extent elements.  For the output coordinate o the source
// coordinate on source axis a is c_a = start_a + sum_d map[a][d] o_d; where 0 <= c_a < src_extent_a on every source axis, element
// rowmajor_dst(dst_start + o) of the destination is element rowmajor_src(c) of the source, and the fill record otherwise.  The
// elements of the destination outside the box are not written.
//
// The two functions decode the linear index of a box element with the same chain of divisions (the compiler shares it where both
// are called for one element) and keep every loop at its full 8 x 8 trip count under a guard: the descriptor is a kernel argument,
// and only constant subscripts let it stay in scalar registers.  The sums run on unsigned 64-bit words, where a partial sum may
// wrap: view_check has established that every c_a fits an int64, so the final sum is exact.
#pragma once
#include <stdint.h>

#include "../../include/cofhe_hip.h"

#if defined(__HIPCC__)
#define VIEW_FN __host__ __device__ inline
#define VIEW_UNROLL _Pragma("unroll")
#else
#define VIEW_FN inline
#define VIEW_UNROLL
#endif

// Device status bit of the index gather, next to the CF_ST_* bits of lane.hpp (1 .. 16; cofhe_hip_device_status): an index beyond
// the source -- the fill record was written, nothing was read there.  It lives here and not in lane.hpp because lane.hpp is one
// of the sources the composition kernels' code hash covers (bench.py: kernel_code_hash), and this bit changes none of them.
#define CF_ST_BAD_INDEX 32u

namespace cofhe {

constexpr int VIEW_MAX_DIMS = COFHE_HIP_VIEW_MAX_DIMS;
constexpr uint64_t VIEW_MAX_ELEMENTS = 1ull << 48;           // of the source, the box and the destination: byte offsets fit 2^63
constexpr int VIEW_THREADS = 256;                            // k_view_records, k_gather_records
constexpr int VIEW_WAVES = VIEW_THREADS / 64;                // records of 64 pieces or more: one wavefront each
constexpr int VIEW_GROUP = 8;                                // shorter records: eight lanes each

// quotient and remainder of the decode: 32-bit where both operands allow it (every tensor that fits a GPU)
VIEW_FN uint64_t view_divmod(uint64_t x, uint64_t d, uint64_t *q) {
    if (((x | d) >> 32) == 0) {
        const uint32_t xs = (uint32_t)x, ds = (uint32_t)d;
        *q = xs / ds;
        return xs % ds;
    }
    *q = x / d;
    return x % d;
}

// the linear index into the source of element box_linear (row-major over out_extent) of the box, or false: the fill record
VIEW_FN bool view_source(const cofhe_hip_view &v, uint64_t box_linear, uint64_t *src_index) {
    uint64_t c[VIEW_MAX_DIMS];
    VIEW_UNROLL
    for (int a = 0; a < VIEW_MAX_DIMS; a++) c[a] = (uint64_t)v.start[a];
    uint64_t rem = box_linear;
    VIEW_UNROLL
    for (int d = VIEW_MAX_DIMS - 1; d >= 0; d--) {
        if ((uint32_t)d < v.out_ndim) {
            const uint64_t o = view_divmod(rem, v.out_extent[d], &rem);
            VIEW_UNROLL
            for (int a = 0; a < VIEW_MAX_DIMS; a++) c[a] += (uint64_t)(int64_t)v.map[a][d] * o;
        }
    }
    bool inside = true;
    uint64_t lin = 0;
    VIEW_UNROLL
    for (int a = 0; a < VIEW_MAX_DIMS; a++) {
        if ((uint32_t)a < v.src_ndim) {
            inside = inside && c[a] < v.src_extent[a];        // a negative coordinate is a large unsigned one
            lin = lin * v.src_extent[a] + c[a];
        }
    }
    *src_index = lin;
    return inside;
}

// the linear index into the destination of element box_linear of the box
VIEW_FN uint64_t view_dest(const cofhe_hip_view &v, uint64_t box_linear) {
    uint64_t o[VIEW_MAX_DIMS];
    uint64_t rem = box_linear;
    VIEW_UNROLL
    for (int d = VIEW_MAX_DIMS - 1; d >= 0; d--) {
        o[d] = 0;
        if ((uint32_t)d < v.out_ndim) o[d] = view_divmod(rem, v.out_extent[d], &rem);
    }
    uint64_t lin = 0;
    VIEW_UNROLL
    for (int d = 0; d < VIEW_MAX_DIMS; d++)
        if ((uint32_t)d < v.out_ndim) lin = lin * v.dst_extent[d] + (v.dst_start[d] + o[d]);
    return lin;
}

// The validator (host): the element counts of the source, the box and the destination, and whether some element of the box can
// read outside the source.  Null, or what is wrong: more than 8 axes, a box that does not lie inside dst_extent, a count beyond
// VIEW_MAX_ELEMENTS, or a source coordinate that can leave the range of an int64.  The o_d vary independently, so the range of c_a
// over the box is exactly [start_a + sum of the negative terms, start_a + sum of the positive terms] with the terms map[a][d]
// (out_extent_d - 1); each term is below 2^31 2^64 in magnitude and there are 8 of them, so a 128-bit sum cannot overflow.
inline const char *view_check(const cofhe_hip_view &v, uint64_t *n_src, uint64_t *n_box, uint64_t *n_dst, int *needs_fill) {
    if (v.out_ndim > (uint32_t)VIEW_MAX_DIMS || v.src_ndim > (uint32_t)VIEW_MAX_DIMS) return "view: more than 8 axes";
    auto count = [](const uint64_t *e, uint32_t nd, uint64_t *n) {        // false: too many; a zero extent gives 0 whatever the others are
        unsigned __int128 p = 1;
        bool zero = false;
        for (uint32_t i = 0; i < nd; i++) {
            if (e[i] == 0) zero = true;
            if (p <= VIEW_MAX_ELEMENTS) p *= e[i] ? e[i] : 1;
        }
        *n = zero ? 0 : (uint64_t)p;
        return zero || p <= VIEW_MAX_ELEMENTS;
    };
    uint64_t ns = 0, nb = 0, nd = 0;
    if (!count(v.src_extent, v.src_ndim, &ns) || !count(v.out_extent, v.out_ndim, &nb) || !count(v.dst_extent, v.out_ndim, &nd))
        return "view: more than 2^48 elements";
    for (uint32_t d = 0; d < v.out_ndim; d++)
        if (v.dst_start[d] > v.dst_extent[d] || v.out_extent[d] > v.dst_extent[d] - v.dst_start[d])
            return "view: the box does not lie inside the destination";
    int fill = 0;
    if (nb != 0) {
        for (uint32_t a = 0; a < v.src_ndim; a++) {
            __int128 lo = v.start[a], hi = v.start[a];
            for (uint32_t d = 0; d < v.out_ndim; d++) {
                const __int128 t = (__int128)v.map[a][d] * (__int128)(v.out_extent[d] - 1);
                if (t < 0) lo += t; else hi += t;
            }
            if (lo < (__int128)INT64_MIN || hi > (__int128)INT64_MAX) return "view: a source coordinate leaves the range of 64 bits";
            if (lo < 0 || hi >= (__int128)v.src_extent[a]) fill = 1;
        }
    }
    if (n_src) *n_src = ns;
    if (n_box) *n_box = nb;
    if (n_dst) *n_dst = nd;
    if (needs_fill) *needs_fill = fill;
    return nullptr;
}

}  // namespace cofhe
