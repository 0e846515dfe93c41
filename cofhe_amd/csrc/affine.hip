// affine.hip -- ciphertext differences and record inverses (launched by abi.hip, declared in kernels.hpp):
// cofhe_hip_sub_ciphertext_records and cofhe_hip_invert_records.  The plaintext addend of cofhe_hip_add_plain_records is a
// shape of the fixed-base comb (comb.hpp, comb.hip).
#include <hip/hip_runtime.h>

#include "affine.hpp"
#include "wg_ctx.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// out[i] = a[i] o b[i]^-1 per record of n_ct ciphertexts: k_add_ct's protocol (cofhe_hip.hip) with the second operand
// inverted after its load.  flag: the verdict of k_c1_distinct; when both tensors share their c1, so does the difference, and
// the launch runs n_ct + 1 compositions (every c2 and the one c1) and leaves the rest to k_c1_spread.  only: 0 this launch
// acts whatever the flag says; 1 / 2: it is one of a pair of launches and acts when the tensors share their c1 / when they
// do not (the other launch of the pair returns at once).
__device__ __forceinline__ void sub_ct_body(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, uint32_t *__restrict__ out, uint64_t n_ct,
                                            const uint32_t *__restrict__ flag, const uint32_t *__restrict__ absdelta, int half_dbits,
                                            uint32_t *__restrict__ status, uint32_t only) {
    __shared__ uint32_t lds[WG_CTX_LDS_WORDS];
    const uint32_t distinct = *flag;
    if (only != 0 && (only == 1) != (distinct == 0)) return;
    const uint64_t n = distinct ? 2 * n_ct : n_ct + 1;
    if ((uint64_t)blockIdx.x * WG_GROUPS >= n) return;           // whole workgroups only: nobody is left at a barrier
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < n ? g0 : n - 1;                      // beyond the work: recompute the last item, store nothing
    const uint64_t rec = distinct ? g : (g < n_ct ? 2 * g + 1 : 0);
    QForm r;
    qf_sub_records(c, r, a + rec * REC_WORDS, b + rec * REC_WORDS, dd);
    if (g0 < n) qf_store(c, r, out + rec * REC_WORDS);
}
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_sub_ct(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                                uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag,
                                                                const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status, uint32_t only) {
    sub_ct_body(a, b, out, n_ct, flag, absdelta, half_dbits, status, only);
}
// three workgroups per CU (see k_compose_wg3): for grids of at most 768 workgroups
__global__ void __launch_bounds__(WG_BLOCK, 3) k_sub_ct3(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                         uint32_t *__restrict__ out, uint64_t n_ct, const uint32_t *__restrict__ flag,
                                                         const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status, uint32_t only) {
    sub_ct_body(a, b, out, n_ct, flag, absdelta, half_dbits, status, only);
}

// out[r] = in[r]^-1 for the n records r = i stride + offset, i < n; one limb group per record, no workgroup protocol
// (stride 1: every record of a tensor; stride 2, offset 0: the c1 of every ciphertext).  in == out allowed.
__global__ void __launch_bounds__(WG_BLOCK) k_invert_records(const uint32_t *in, uint32_t *out, uint64_t n, uint32_t stride,
                                                             uint32_t offset) {
    __shared__ uint32_t lds[WG_GROUPS * SCRATCH_WORDS];
    Ctx c;
    const int lane = (int)(threadIdx.x & 63);
    c.gl = lane & (G - 1);
    c.base4 = (lane & ~(G - 1)) << 2;
    c.scr = lds + (threadIdx.x / G) * SCRATCH_WORDS;
    const uint64_t g = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    if (g >= n) return;
    const uint64_t rec = g * stride + offset;
    qf_invert_record(c, in + rec * REC_WORDS, out + rec * REC_WORDS);
}

}  // namespace cofhe_k
