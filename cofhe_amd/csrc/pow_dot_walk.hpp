// pow_dot_walk.hpp -- the lockstep walk of the multi-exponentiation with shared squarings (schedule: pow_dot.hpp), as a device
// function parameterised by how a base record is addressed: k_pow_dot (pow_dot.hip) reads base i of a record a tensor further,
// k_spline_close (spline.hip) reads it in place from the selected row of the element's tuple.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "pow_dot.hpp"
#include "wg_ctx.hpp"

namespace cofhe_k {

// the signed digits of the d exponents of one record: the non-adjacent form of qf.hpp (one 64-bit carry pack per base) times
// the sign word of the exponent
struct PowDotDigits {
    const uint32_t *exps;                   // exponent record of base 0; base i is `stride` words further
    uint64_t stride;
    uint64_t pack[cofhe::POLY_MAX_DEGREE];
    __device__ __forceinline__ const uint32_t *rec(int i) const { return exps + (uint64_t)i * stride; }
    __device__ __forceinline__ int operator()(int i, int t) const {
        const uint32_t *e = rec(i);
        const int dg = cofhe::exp_naf_digit(e, pack[i], t);
        return e[cofhe::EXP_MAG_WORDS] ? -dg : dg;
    }
};

// dig.exps and dig.stride set: the carry packs of the nd exponents and the state at the top position
__device__ __forceinline__ cofhe::PowDotState pow_dot_prepare(PowDotDigits &dig, int nd) {
    using namespace cofhe;
#pragma unroll
    for (int i = 0; i < POLY_MAX_DEGREE; i++) dig.pack[i] = i < nd ? exp_naf_prepare(dig.rec(i)) : 0ull;
    return pow_dot_begin(nd, [&](int i) {
        const uint32_t *e = dig.rec(i);
        const int nb = exp_bitlen(e);
        return nb == 0 ? -1 : exp_naf_top(e, dig.pack[i], nb);
    });
}

// The walk of one record of a workgroup of 32: accp = prod_{i < nd} base_at(i)^exponent i, left in the record accp (nothing is
// stored when every exponent is zero: s.t < 0 on entry).  The 32 groups advance in lockstep, one qf_compose<true, false> per
// round; every round reloads its operands, and a group without work squares base_at(0) and stores nothing.  No form is kept in
// registers across a composition.  Rounds of a workgroup = the longest walk among its 32 records, at most max_rounds (from the
// exponents' 992 bits: the loop has a fixed cap whatever the data says).
// dig(i, t): the signed digit of base i at position t (PowDotDigits, or a functor that adds a base of its own to them).
template <typename Digit, typename BaseAt>
__device__ __forceinline__ void pow_dot_walk(cofhe::Ctx &c, const cofhe::QDisc &dd, bool alive, int nd, const Digit &dig,
                                             cofhe::PowDotState &s, uint32_t *accp, const BaseAt &base_at) {
    using namespace cofhe;
    // a walk is at most 993 squarings and 8 x 994 digits
    const int max_rounds = (POLY_MAX_DEGREE + 1) * WNAF_POSITIONS;
    for (int round = 0; round < max_rounds; round++) {
        // this record's next composition, if any; the copy that starts the walk is none
        PowDotOp op = pow_dot_step(s, nd, dig);
        if (op.kind == PD_COPY) {
            QForm x;
            qf_load(c, x, base_at(op.base));
            if (op.inv) qf_inverse(c, x);
            if (alive) qf_store(c, x, accp);
            op = pow_dot_step(s, nd, dig);
        }
        const bool has = alive && op.kind != PD_DONE;
        if (!__syncthreads_or(has ? 1 : 0)) break;
        QForm l_, rhs, r;
        qf_load(c, l_, has ? (const uint32_t *)accp : base_at(0));
        if (has && op.kind == PD_MUL) {
            qf_load(c, rhs, base_at(op.base));
            if (op.inv) qf_inverse(c, rhs);
        } else {
            rhs = l_;
        }
        qf_compose<true, false, false>(c, r, l_, rhs, dd);
        if (has) qf_store(c, r, accp);
    }
}

}  // namespace cofhe_k
