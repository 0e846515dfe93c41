// compare.hip -- the two kernels of the sign of a ciphertext on a window of up to 64 bits from digit comparisons (launched by
// abi.hip, declared in kernels.hpp; the protocol, the threshold arithmetic and the body of the plaintext kernel: compare.hpp).
// k_cmp_rows writes the plaintext rows of the comparison tuples, 2^j sgn(r_j - c) for every digit j of each element's mask and
// every candidate c; k_cmp_close closes the first round by composing, for both thresholds of the opened value, the one entry per
// digit that the threshold names.
#include <hip/hip_runtime.h>

#include "compare.hpp"
#include "wg_ctx.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {

// out[(i n + j) 2^d + c] = 2^j sgn(r_ij - c) on exponent records, r_ij digit j of r[i] mod 2^bits, i < elements, j < n =
// ceil(bits / d), c < 2^d: pure stores, a grid-stride loop over pieces (cmp_rows_piece).  vec16: the launcher found out 16-byte
// aligned (r is read a word at a time either way); out must not overlap r
__global__ void __launch_bounds__(CMP_ROWS_THREADS) k_cmp_rows(const uint32_t *__restrict__ r, uint32_t *__restrict__ out, uint64_t elements,
                                                               uint32_t bits, uint32_t digit_bits, uint32_t vec16) {
    const uint64_t recs = (elements * cmp_digits(bits, digit_bits)) << digit_bits;
    const uint64_t total = recs * (vec16 ? (uint64_t)EXP_REC_WORDS / 4 : (uint64_t)EXP_REC_WORDS);
    for (uint64_t idx = (uint64_t)blockIdx.x * CMP_ROWS_THREADS + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * CMP_ROWS_THREADS) {
        if (vec16)
            cmp_rows_piece<4>(r, out, idx, bits, digit_bits);
        else
            cmp_rows_piece<1>(r, out, idx, bits, digit_bits);
    }
}

// out[(2 i + s) 2 + h] = prod_{j < n} q(j, t_s), q(j, t) = tuples[((i n + j) 2^d + digit j of t) 2 + h], t_0 = A and t_1 = B the
// thresholds of u = e[i] mod 2^bits (compare.hpp), i < elements, h in {0, 1}: one limb group per (element, half).  A sequence
// kernel in the pattern of k_spline_close: the 32 groups of a workgroup advance in lockstep, one qf_compose<true, false, false>
// per round; every round reloads its operands, and a group without work squares its first entry and stores nothing.  The entries
// are read in place from the tuple and no form is kept in registers across a composition.  A and B share every digit below
// the top one, so the prefix L = prod_{j < n - 1} q(j, A) is built once, in the output record of [S_A] (which therefore must not
// overlap an input: the launcher refuses that); then [S_B] = L o q(n - 1, B) goes to its own record and [S_A] = L o q(n - 1, A)
// replaces L: n compositions per half, not 2 (n - 1).  For n = 1 the prefix is empty and both results are copies.  Every
// group of a launch has the same n, so the rounds are n for n >= 2 whatever the data says; the loop is capped by CMP_MAX_DIGITS.
// The lane 0 of each element's half 0 also writes wrap[i] = [A > B] as an exponent record.
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_cmp_close(const uint32_t *__restrict__ e, const uint32_t *__restrict__ tuples,
                                                                   uint32_t *__restrict__ out, uint32_t *__restrict__ wrap, uint64_t elements,
                                                                   uint32_t bits, uint32_t digit_bits, const uint32_t *__restrict__ absdelta,
                                                                   int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[WG_CTX_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t n_groups = 2 * elements;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const bool alive = g0 < n_groups;
    const uint64_t g = alive ? g0 : n_groups - 1;
    const uint64_t i = g >> 1;
    const uint32_t h = (uint32_t)(g & 1);
    const uint32_t n = cmp_digits(bits, digit_bits);
    const CmpThresholds th = cmp_thresholds(cmp_low(e + i * EXP_REC_WORDS, bits), bits);
    const auto entry = [&](uint32_t j, uint64_t t) { return tuples + (cmp_entry(i, n, j, digit_bits, t) * 2 + h) * REC_WORDS; };
    uint32_t *out_a = out + ((2 * i + 0) * 2 + h) * REC_WORDS, *out_b = out + ((2 * i + 1) * 2 + h) * REC_WORDS;
    if (alive && h == 0 && c.gl == 0) {
        uint32_t *w = wrap + i * EXP_REC_WORDS;
        w[0] = th.wrap;
        for (int l = 1; l < EXP_REC_WORDS; l++) w[l] = 0u;
    }
    // the copy that starts the prefix (n = 1: the two results themselves)
    {
        QForm x;
        qf_load(c, x, entry(0, th.a));
        if (alive) qf_store(c, x, out_a);
        if (n == 1) {
            qf_load(c, x, entry(0, th.b));
            if (alive) qf_store(c, x, out_b);
        }
    }
    // round k < n - 2 extends the prefix by digit k + 1; round n - 2 writes [S_B], round n - 1 [S_A]
    const uint32_t rounds = n >= 2 ? n : 0;
    for (uint32_t round = 0; round < CMP_MAX_DIGITS; round++) {
        const bool has = alive && round < rounds;
        if (!__syncthreads_or(has ? 1 : 0)) break;
        const bool to_b = round + 2 == n;
        const uint32_t j = round + 2 < n ? round + 1 : n - 1;
        QForm l_, rhs, r;
        qf_load(c, l_, has ? (const uint32_t *)out_a : entry(0, th.a));
        if (has)
            qf_load(c, rhs, entry(j, to_b ? th.b : th.a));
        else
            rhs = l_;
        qf_compose<true, false, false>(c, r, l_, rhs, dd);
        if (has) qf_store(c, r, to_b ? out_b : out_a);
    }
}

}  // namespace cofhe_k
