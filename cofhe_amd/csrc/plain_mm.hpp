// plain_mm.hpp -- the body of k_plain_matmul (matmul_left.hip): out[i,k] = sum_j a[i,j] b[j,k] mod 2^kbits on exponent
// records, in a header so that the host build of the CPU tests (tests/hostsim/plain_mm_sim.cpp, COFHE_HOSTSIM) compiles the
// very code the kernel runs.
//
// An exponent record is 32 words: 31 magnitude words and a sign word (non-zero: negative).  A value enters the product as
// its residue in [0, 2^k): the low L = ceil(k/32) limbs of the magnitude, the top limb masked to k - 32 (L - 1) bits, and the
// two's complement of that (masked again) where the sign word is set -- so magnitudes of 2^k and above and -0 are fine.
// The product of two residues is the low half of the schoolbook product, L (L + 1) / 2 word products: everything at or above
// limb L vanishes mod 2^k.  The sum stays in L registers; only the store masks the top limb (2^k divides 2^(32 L)).
//
// One workgroup of PMM_THREADS = 16 x 16 threads owns a 16 x 16 tile of the output and walks the inner dimension 16 at a
// time: pmm_stage reduces one element of a and one of b per thread into the tile buffers (limb-major: limb l of element (r, c)
// at l * 256 + r * 16 + c, so that the 16 threads of a row read consecutive words of b and one word of a), a barrier,
// pmm_accumulate runs the 16 products of the thread's output, a barrier.  Elements beyond the matrices are staged as zero.
#pragma once
#include <stdint.h>

#if defined(COFHE_HOSTSIM)
#define PMM_DEV inline
#define PMM_UNROLL
#else
#include <hip/hip_runtime.h>
#define PMM_DEV __device__ __forceinline__
#define PMM_UNROLL _Pragma("unroll")
#endif

namespace cofhe {

constexpr int PMM_TILE = 16, PMM_THREADS = PMM_TILE * PMM_TILE;
constexpr int PMM_REC_WORDS = 32, PMM_MAG_WORDS = 31;        // an exponent record
constexpr int PMM_FIXED_LIMBS = 8;                           // k <= 256: the limb count is a template argument
constexpr int PMM_MAX_LIMBS = 20;                            // k <= 639, the bound of the decryption table (2 k + 1 <= 1280)
constexpr int pmm_limbs(uint32_t kbits) { return (int)((kbits + 31) / 32); }
constexpr uint32_t pmm_top_mask(uint32_t kbits) { return (kbits & 31) ? (1u << (kbits & 31)) - 1u : 0xFFFFFFFFu; }
constexpr int pmm_tile_words(int limbs) { return PMM_THREADS * limbs; }      // one of the two tile buffers

// the residue of one record into limb-major tile storage: v[l * stride], l < L
template <int LMAX>
PMM_DEV void pmm_reduce(const uint32_t *rec, int L, uint32_t kbits, uint32_t *v, int stride) {
    const uint32_t top = pmm_top_mask(kbits);
    const bool neg = rec[PMM_MAG_WORDS] != 0;
    uint32_t borrow = 1;                                      // -x = ~x + 1
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) {
        if (l < L) {                                          // a guard, not a break: the loop unrolls for a runtime L too
            uint32_t w = rec[l];
            if (neg) {
                w = ~w + borrow;
                borrow = borrow & (w == 0);
            }
            if (l == L - 1) w &= top;
            v[l * stride] = w;
        }
    }
}

// acc += a * b mod 2^(32 L); a, b in tile storage (strides in words)
template <int LMAX>
PMM_DEV void pmm_mac(uint32_t (&acc)[LMAX], const uint32_t *a, int a_stride, const uint32_t *b, int b_stride, int L) {
    uint32_t bv[LMAX];
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++) bv[l] = l < L ? b[l * b_stride] : 0u;
    PMM_UNROLL
    for (int i = 0; i < LMAX; i++) {
        if (i < L) {
            const uint64_t ai = a[i * a_stride];
            uint64_t carry = 0;
            PMM_UNROLL
            for (int j = 0; j < LMAX - i; j++) {
                if (i + j < L) {
                    const uint64_t t = ai * bv[j] + acc[i + j] + carry;      // <= (2^32 - 1)^2 + 2 (2^32 - 1) = 2^64 - 1
                    acc[i + j] = (uint32_t)t;
                    carry = t >> 32;
                }
            }
        }
    }
}

// The two phases of one step of 16 along the inner dimension, for thread tid of the workgroup that owns the output tile at
// (i0, k0); a workgroup barrier separates them, and another follows pmm_accumulate.  lds: 2 * pmm_tile_words(L) words.
// one thread's element of a tile buffer (t = buffer + tid): the residue of rec, or zero for a null rec -- an element beyond the
// matrix, or the padding of a convolution (plain_conv.hpp)
template <int LMAX>
PMM_DEV void pmm_stage_one(uint32_t *t, const uint32_t *rec, int L, uint32_t kbits) {
    if (rec) {
        pmm_reduce<LMAX>(rec, L, kbits, t, PMM_THREADS);
    } else {
        for (int l = 0; l < L; l++) t[l * PMM_THREADS] = 0;
    }
}
template <int LMAX>
PMM_DEV void pmm_stage(uint32_t *lds, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t m, uint32_t p, uint32_t i0, uint32_t k0,
                       uint32_t j0, int tid, int L, uint32_t kbits) {
    const uint32_t r = (uint32_t)tid / PMM_TILE, c = (uint32_t)tid % PMM_TILE;
    pmm_stage_one<LMAX>(lds + tid, i0 + r < n && j0 + c < m ? a + ((uint64_t)(i0 + r) * m + (j0 + c)) * PMM_REC_WORDS : nullptr, L, kbits);
    pmm_stage_one<LMAX>(lds + pmm_tile_words(L) + tid, j0 + r < m && k0 + c < p ? b + ((uint64_t)(j0 + r) * p + (k0 + c)) * PMM_REC_WORDS : nullptr,
                        L, kbits);
}
template <int LMAX>
PMM_DEV void pmm_accumulate(const uint32_t *lds, uint32_t (&acc)[LMAX], int tid, int L) {
    const int r = tid / PMM_TILE, c = tid % PMM_TILE;
    const uint32_t *ta = lds + r * PMM_TILE, *tb = lds + pmm_tile_words(L) + c;
    for (int jj = 0; jj < PMM_TILE; jj++) pmm_mac<LMAX>(acc, ta + jj, PMM_THREADS, tb + jj * PMM_TILE, PMM_THREADS, L);
}

// the sum as an exponent record: a value in [0, 2^k), zero words above it, sign word 0
template <int LMAX>
PMM_DEV void pmm_store(const uint32_t (&acc)[LMAX], int L, uint32_t kbits, uint32_t *rec) {
    const uint32_t top = pmm_top_mask(kbits);
    PMM_UNROLL
    for (int l = 0; l < LMAX; l++)
        if (l < L) rec[l] = l == L - 1 ? acc[l] & top : acc[l];
    for (int l = L; l < PMM_REC_WORDS; l++) rec[l] = 0;
}

}  // namespace cofhe
