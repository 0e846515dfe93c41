// pow_dot.hip -- the two kernels of a polynomial evaluation on ciphertexts (launched by abi.hip, declared in kernels.hpp):
// k_pow_dot, the per-record multi-exponentiation with shared squarings of cofhe_hip_pow_dot_records (its schedule:
// pow_dot.hpp; its lockstep loop: pow_dot_walk.hpp, shared with k_spline_close), and k_poly_shift, the Taylor shift mod 2^k on exponent records of cofhe_hip_poly_shift_records (its body:
// poly_shift.hpp).  cofhe_hip_poly_close_records runs the one on the output of the other.
#include <hip/hip_runtime.h>

#include "poly_shift.hpp"
#include "pow_dot.hpp"
#include "pow_dot_walk.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// out[2 e + h] = prod_{i < d} bases[(i E + e) 2 + h]^exps[i E + e], e < n_ct, h in {0, 1}, 1 <= d <= POLY_MAX_DEGREE: one limb
// group per output record, the walk of pow_dot.hpp.  A sequence kernel like k_pow (cofhe_hip.hip): the 32 groups of a
// workgroup advance in lockstep, one qf_compose<true, false> per round; the running product lives in the OUTPUT record (which
// therefore must not overlap the bases or the exponents: the launcher refuses that), every round reloads its operands, and a
// group without work squares base 0 of its record and stores nothing.  No form is kept in registers across a composition.
// Rounds of a workgroup = the longest walk among its 32 records, at most max_rounds (from the exponents' 992 bits: the loop
// has a fixed cap whatever the data says).
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_pow_dot(const uint32_t *__restrict__ bases, const uint32_t *__restrict__ exps,
                                                                 uint32_t *__restrict__ out, uint64_t n_ct, uint32_t d,
                                                                 const uint32_t *__restrict__ one_rec, const uint32_t *__restrict__ absdelta,
                                                                 int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_CTX_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t n_records = 2 * n_ct;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_records;
    const uint64_t g = alive ? g0 : n_records - 1;
    const int nd = (int)d;
    // base i of this record and the stand-in of an idle round (base 0)
    const uint32_t *xrec = bases + g * REC_WORDS;
    const uint64_t xstride = n_records * REC_WORDS;
    uint32_t *accp = out + g * REC_WORDS;
    PowDotDigits dig;
    dig.exps = exps + (g >> 1) * EXP_REC_WORDS;
    dig.stride = n_ct * EXP_REC_WORDS;
    PowDotState s = pow_dot_prepare(dig, nd);
    const bool all_zero = s.t < 0;
    pow_dot_walk(c, dd, alive, nd, dig, s, accp, [&](int i) { return xrec + (uint64_t)i * xstride; });
    if (alive && all_zero) {
        QForm acc;
        qf_load(c, acc, one_rec);
        qf_store(c, acc, accp);
    }
}

// q[i n + e] = sum_{j >= i} C(j, i) coef[j] x[e]^(j - i) mod 2^kbits, i <= d, on exponent records (poly_shift.hpp): one thread
// per element, 1 <= kbits <= 32 PMM_MAX_LIMBS, d <= POLY_MAX_DEGREE; q must not overlap coef or x
__global__ void __launch_bounds__(PSH_THREADS) k_poly_shift(const uint32_t *__restrict__ coef, const uint32_t *__restrict__ x,
                                                            uint32_t *__restrict__ q, uint64_t n, uint32_t d, uint32_t kbits) {
    const uint64_t e = (uint64_t)blockIdx.x * PSH_THREADS + threadIdx.x;
    if (e >= n) return;
    poly_shift_element(coef, x, q, n, e, (int)d, kbits);
}

}  // namespace cofhe_k
