// comb.hip -- the kernels of the fixed-base comb (comb.hpp): the table build and the fused gather + first tree level.
// Launched by abi.hip (cofhe_hip_pow_fixed_base_many_records, cofhe_hip_encrypt_fresh_records,
// cofhe_hip_rerandomize_records, cofhe_hip_add_plain_records); the levels above the first are k_compose_pairs of cofhe_hip.hip.
#include <hip/hip_runtime.h>

#include "comb.hpp"
#include "wg_ctx.hpp"

using namespace cofhe;

#ifndef COFHE_WPS
#define COFHE_WPS 4      // minimum waves per SIMD the register allocator must leave room for (as cofhe_hip.hip)
#endif

namespace cofhe_k {
constexpr int COMB_LDS_WORDS = WG_CTX_LDS_WORDS;

// One level l of a comb table (w - 1 launches per table): T[j][u + half] = T[j][u] o T[j][half], 1 <= u <= half = 2^(l-1),
// for every position j < npos -- npos x half independent compositions.  T[j][1] is chain entry w j (copied by the host).
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_comb_table(uint32_t *__restrict__ table, uint32_t npos, uint32_t w, uint32_t half,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits,
                                                                    uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[COMB_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t total = (uint64_t)npos * half;
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < total ? g0 : total - 1;              // beyond the level: recompute the last item, store nothing
    const uint64_t j = g / half, u = g % half + 1;
    uint32_t *row = table + j * comb_entries(w) * REC_WORDS;
    QForm a, b, r;
    qf_load(c, a, row + (u - 1) * REC_WORDS);
    qf_load(c, b, row + (uint64_t)(half - 1) * REC_WORDS);
    qf_compose<true, false, false>(c, r, a, b, dd);
    if (g0 < total) qf_store(c, r, row + (u + half - 1) * REC_WORDS);
}

// Gather and first tree level in one pass: group g owns column g % ncols and slot pair g / ncols (output layout
// [pair][column], what k_compose_pairs walks with n = 1, q = ncols).  It selects the two slots' entries from the exponent
// records (comb_select: Booth digits on the fly), inverts an entry whose digit is negative, composes the two and stores
// one record.  tabs: the r tables of half 0 and 1 and the table of f; r_exps / m_exps / leaf: this chunk's records (r_exps
// null: a shape without r positions).  A c2_only shape has one column per ciphertext: half 1, leaf record 2 col + 1.
__global__ void __launch_bounds__(WG_BLOCK, COFHE_WPS) k_comb_first(CombShape s, const uint32_t *__restrict__ tab0, const uint32_t *__restrict__ tab1,
                                                                    const uint32_t *__restrict__ tabf, const uint32_t *__restrict__ r_exps,
                                                                    const uint32_t *__restrict__ m_exps, const uint32_t *__restrict__ leaf,
                                                                    uint64_t ncols, const uint32_t *__restrict__ one_rec, uint32_t *__restrict__ out,
                                                                    const uint32_t *__restrict__ absdelta, int half_dbits, uint32_t *__restrict__ status) {
    __shared__ uint32_t lds[COMB_LDS_WORDS];
    Ctx c = make_served_ctx(lds);
    const QDisc dd{absdelta, half_dbits};
    c.status = status;
    const uint64_t total = ncols * (comb_slots(s) / 2);
    const uint64_t g0 = (uint64_t)blockIdx.x * WG_GROUPS + threadIdx.x / G;
    const uint64_t g = g0 < total ? g0 : total - 1;
    const uint64_t col = g % ncols, pair = g / ncols;
    const uint64_t item = s.halves == 2 ? col >> 1 : col;
    const uint32_t h = s.halves == 2 ? (uint32_t)(col & 1) : s.c2_only;
    const uint32_t *me = m_exps ? m_exps + item * EXP_REC_WORDS : nullptr;
    const uint32_t *re = r_exps ? r_exps + item * EXP_REC_WORDS : me;
    if (!me) me = re;
    QForm x[2];
    bool trivial[2];
    CF_UNROLL for (int k = 0; k < 2; k++) {
        const CombSel sel = comb_select(s, h, (uint32_t)(2 * pair + k), re, me);
        const uint32_t *src = one_rec;
        if (sel.table == 3) src = leaf + (s.c2_only ? 2 * col + 1 : col) * REC_WORDS;
        else if (sel.table >= 0) src = (sel.table == 0 ? tab0 : sel.table == 1 ? tab1 : tabf) + (uint64_t)comb_entry(s, sel) * REC_WORDS;
        qf_load(c, x[k], src);
        if (sel.table == 3 ? s.leaf_inv != 0 : (sel.table >= 0 && sel.digit < 0)) qf_inverse(c, x[k]);
        trivial[k] = sel.table < 0;
    }
    // a principal operand leaves the other one as it is: a workgroup in which every group has one skips the round
    if (!__syncthreads_or((trivial[0] || trivial[1]) ? 0 : 1)) {
        if (g0 < total) qf_store(c, trivial[0] ? x[1] : x[0], out + g * REC_WORDS);
        return;
    }
    QForm r;
    qf_compose<true, false, false>(c, r, x[0], x[1], dd);
    if (g0 < total) qf_store(c, r, out + g * REC_WORDS);
}

}  // namespace cofhe_k
