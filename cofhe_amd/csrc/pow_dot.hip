// pow_dot.hip -- the two kernels of a polynomial evaluation on ciphertexts (launched by abi.hip, declared in kernels.hpp):
// k_pow_dot, the per-record multi-exponentiation with shared squarings of cofhe_hip_pow_dot_records (its schedule:
// pow_dot.hpp), and k_poly_shift, the Taylor shift mod 2^k on exponent records of cofhe_hip_poly_shift_records (its body:
// poly_shift.hpp).  cofhe_hip_poly_close_records runs the one on the output of the other.
#include <hip/hip_runtime.h>

#include "poly_shift.hpp"
#include "pow_dot.hpp"
#include "wg_ctx.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// the signed digits of the d exponents of one record: the non-adjacent form of qf.hpp (one 64-bit carry pack per base) times
// the sign word of the exponent
struct PowDotDigits {
    const uint32_t *exps;                   // exponent record of base 0; base i is `stride` words further
    uint64_t stride;
    uint64_t pack[POLY_MAX_DEGREE];
    __device__ __forceinline__ const uint32_t *rec(int i) const { return exps + (uint64_t)i * stride; }
    __device__ __forceinline__ int operator()(int i, int t) const {
        const uint32_t *e = rec(i);
        const int dg = exp_naf_digit(e, pack[i], t);
        return e[EXP_MAG_WORDS] ? -dg : dg;
    }
};

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
#pragma unroll
    for (int i = 0; i < POLY_MAX_DEGREE; i++) dig.pack[i] = i < nd ? exp_naf_prepare(dig.rec(i)) : 0ull;
    PowDotState s = pow_dot_begin(nd, [&](int i) {
        const uint32_t *e = dig.rec(i);
        const int nb = exp_bitlen(e);
        return nb == 0 ? -1 : exp_naf_top(e, dig.pack[i], nb);
    });
    const bool all_zero = s.t < 0;
    // a walk is at most 993 squarings and 8 x 994 digits
    const int max_rounds = (POLY_MAX_DEGREE + 1) * WNAF_POSITIONS;
    for (int round = 0; round < max_rounds; round++) {
        // this record's next composition, if any; the copy that starts the walk is none
        PowDotOp op = pow_dot_step(s, nd, dig);
        if (op.kind == PD_COPY) {
            QForm x;
            qf_load(c, x, xrec + (uint64_t)op.base * xstride);
            if (op.inv) qf_inverse(c, x);
            if (alive) qf_store(c, x, accp);
            op = pow_dot_step(s, nd, dig);
        }
        const bool has = alive && op.kind != PD_DONE;
        if (!__syncthreads_or(has ? 1 : 0)) break;
        QForm l_, rhs, r;
        qf_load(c, l_, has ? (const uint32_t *)accp : xrec);
        if (has && op.kind == PD_MUL) {
            qf_load(c, rhs, xrec + (uint64_t)op.base * xstride);
            if (op.inv) qf_inverse(c, rhs);
        } else {
            rhs = l_;
        }
        qf_compose<true, false, false>(c, r, l_, rhs, dd);
        if (has) qf_store(c, r, accp);
    }
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
