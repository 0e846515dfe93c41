// plain_conv.hpp -- the bodies of k_plain_conv2d and k_gather_patch_exponents (conv_ct.hip): what a convolution with CIPHERTEXT
// filters adds next to the matrix Beaver triplets, in a header so that the host build of the CPU tests
// (tests/hostsim/plain_conv_sim.cpp, COFHE_HOSTSIM) compiles the very code the kernels run.
//
// Both work on a PLAINTEXT image [B, H, W, C] of exponent records, channels last, groups = 1, and read it through conv_leaf
// (conv.hpp), THE geometry: element (row, j) of the n x m patch matrix, n = B Ho Wo, m = kh kw C, is a pixel of the image or
// padding, and padding is the value zero.
//   pconv_stage        one step of the plaintext convolution out[row,co] = sum_j img[conv_leaf(row,j)] w[j,co] mod 2^k: the
//                      implicit GEMM on the tile of plain_mm.hpp.  pmm_stage with the left element fetched through conv_leaf;
//                      the accumulation, the store and the residue rules are plain_mm.hpp's own, and no patch matrix is written.
//   gather_exps_body   the patch matrix written out as exponent records, already transposed: S^T[j n + row] =
//                      img[conv_leaf(row,j)], an all-zero record in the padding -- the m x n exponent matrix that the product
//                      under cofhe_hip_matmul_plain_ct_records takes, without the transposition of an n x m one.
#pragma once
#include "conv.hpp"
#include "plain_mm.hpp"

namespace cofhe {

// pmm_stage for the convolution: thread tid stages element (i0 + r, j0 + c) of the patch matrix of img and element
// (j0 + r, k0 + c) of the filters w (m x p, p = Co); zero where the leaf is padding or the element lies beyond the matrix
template <int LMAX>
PMM_DEV void pconv_stage(uint32_t *lds, const ConvShape &s, const uint32_t *img, const uint32_t *w, uint32_t n, uint32_t m, uint32_t p,
                         uint32_t i0, uint32_t k0, uint32_t j0, int tid, int L, uint32_t kbits) {
    const uint32_t r = (uint32_t)tid / PMM_TILE, c = (uint32_t)tid % PMM_TILE;
    const int64_t leaf = i0 + r < n && j0 + c < m ? conv_leaf(s, i0 + r, j0 + c) : -1;
    pmm_stage_one<LMAX>(lds + tid, leaf < 0 ? nullptr : img + (uint64_t)leaf * PMM_REC_WORDS, L, kbits);
    pmm_stage_one<LMAX>(lds + pmm_tile_words(L) + tid,
                        j0 + r < m && k0 + c < p ? w + ((uint64_t)(j0 + r) * p + (k0 + c)) * PMM_REC_WORDS : nullptr, L, kbits);
}

// out[(j n + row) pieces + t] = img[conv_leaf(row, j) pieces + t], or zero in the padding, for j < m, row < n: records of `pieces`
// pieces of type T (16 bytes, or a dword).  Consecutive indices are consecutive pieces of one OUTPUT record; a thread takes
// the indices first, first + step, ..
template <typename T>
PMM_DEV void gather_exps_body(const ConvShape &s, const T *__restrict__ img, T *__restrict__ out, uint32_t n, uint32_t m, uint32_t pieces,
                              uint64_t first, uint64_t step) {
    const uint64_t total = (uint64_t)m * n * pieces;
    for (uint64_t idx = first; idx < total; idx += step) {
        const uint64_t e = idx / pieces;
        const uint32_t t = (uint32_t)(idx - e * pieces);
        const uint64_t j = e / n;
        const int64_t leaf = conv_leaf(s, (uint32_t)(e - j * n), (uint32_t)j);
        T v{};
        if (leaf >= 0) v = img[(uint64_t)leaf * pieces + t];
        out[idx] = v;
    }
}

}  // namespace cofhe
