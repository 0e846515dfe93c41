// lut.hpp -- the index arithmetic of k_lut_rotate and k_lut_select (lut.hip): table lookups on ciphertext tensors from one
// opened value, in a header so that the host build of the CPU tests (tests/hostsim/lut_sim.cpp, COFHE_HOSTSIM) compiles the very
// code the kernels run.
//
// A lookup evaluates a public table g of 2^b plaintexts, 1 <= b <= LUT_MAX_BITS, b <= k, on values known to lie in a b-bit
// range.  Per element the tuple is ([r], [T_0], .., [T_{2^b - 1}]) with r uniform in Z/2^k and T_j = g[(j + r) mod 2^b]; with
// the one opened value e = Dec(x - r) the result is [T_{e mod 2^b}], since (e + r) mod 2^b = x mod 2^b.  Both kernels need one
// number per element: the low b bits of an exponent record's value mod 2^k.
//
// A record is 31 magnitude words and a sign word (non-zero: negative).  b <= 12 < 32, so the low b bits of the magnitude are in
// word 0, and 2^b divides 2^k, so the residue mod 2^k of -m has the low bits (2^b - (m mod 2^b)) mod 2^b whatever else m holds:
// -0 and magnitudes of 2^k and above follow the same rule and need no case of their own.  Two words of the record are read.
#pragma once
#include "plain_mm.hpp"

namespace cofhe {

constexpr uint32_t LUT_MAX_BITS = 12;                        // 4096 entries per element: 5.5 MB of tuple each
constexpr int LUT_SELECT_THREADS = 256;                      // k_lut_select: one wavefront per output ciphertext
constexpr int LUT_SELECT_WAVES = LUT_SELECT_THREADS / 64;

// the value of an exponent record mod 2^bits, from its word 0 and its sign word
PMM_DEV uint32_t lut_index_of(uint32_t word0, uint32_t sign_word, uint32_t bits) {
    const uint32_t mask = (1u << bits) - 1u, m = word0 & mask;
    return sign_word != 0 ? ((mask + 1u) - m) & mask : m;
}
PMM_DEV uint32_t lut_index(const uint32_t *rec, uint32_t bits) { return lut_index_of(rec[0], rec[PMM_MAG_WORDS], bits); }

// entry j of a rotated row reads entry (j + r) mod 2^bits of the table; r is an index (below 2^bits), j < 2^bits
PMM_DEV uint32_t lut_rotated_source(uint32_t j, uint32_t r_index, uint32_t bits) { return (j + r_index) & ((1u << bits) - 1u); }

}  // namespace cofhe
