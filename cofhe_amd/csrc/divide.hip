// divide.hip -- the kernel of a division of ciphertexts by public divisors from one opened value (launched by abi.hip, declared
// in kernels.hpp): k_plain_divfloor, the signed floor division mod 2^k on exponent records of cofhe_hip_divfloor_plain_records
// (its body: plain_div.hpp).  cofhe_hip_div_close_records runs the plaintext addend of the comb on its output.
#include <hip/hip_runtime.h>

#include "plain_div.hpp"

using namespace cofhe;

namespace cofhe_k {

// q[e] = floor(s(v[e]) / div[e mod n_div]) mod 2^kbits for e < n: one limb group per element, no workgroup protocol (as
// k_invert_records); n_div >= 1, 1 <= kbits <= PDV_MAX_KBITS; q must not overlap v or div.  The LDS is the groups' slices,
// which only mp_divrem touches.  An invalid divisor: quotient 0 and CF_ST_DIV_CAP in *status.
__global__ void __launch_bounds__(PDV_THREADS) k_plain_divfloor(const uint32_t *__restrict__ v, const uint32_t *__restrict__ div, uint64_t n_div,
                                                                uint32_t *__restrict__ q, uint64_t n, uint32_t kbits,
                                                                uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[PDV_GROUPS * SCRATCH_WORDS];
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    c.status = status;
    const uint64_t e = (uint64_t)blockIdx.x * PDV_GROUPS + threadIdx.x / G;
    if (e >= n) return;
    plain_divfloor_element(c, v + e * PMM_REC_WORDS, div + (e % n_div) * PMM_REC_WORDS, q + e * PMM_REC_WORDS, kbits);
}

}  // namespace cofhe_k
