// Host build of the difference kernels' body (cofhe_amd/csrc/affine.hpp) on the simulated workgroup of sim.cpp, and of the
// comb's slot map with the plaintext-addend fields of its shape (comb.hpp).  TEST INFRASTRUCTURE ONLY; not linked into the
// product library.
#include "sim.cpp"       // the lane-group / workgroup simulator (run_workgroup) and COFHE_HOSTSIM

#include "../../cofhe_amd/csrc/affine.hpp"
#include "../../cofhe_amd/csrc/comb.hpp"

extern "C" {
// out[i] = a[i] o b[i]^-1 as k_sub_ct runs it: one workgroup, group gi takes pair min(gi, count - 1), count <= WG_GROUPS
void affine_sim_sub_wg(const uint32_t *a, const uint32_t *b, uint32_t *out, int count, int half_dbits, const uint32_t *absdelta) {
    const QDisc dd{absdelta, half_dbits};
    run_workgroup([&](Ctx &c) {
        const int i = c.gi < count ? c.gi : count - 1;
        QForm r;
        qf_sub_records(c, r, a + (size_t)REC_WORDS * i, b + (size_t)REC_WORDS * i, dd);
        if (c.gi < count) qf_store(c, r, out + (size_t)REC_WORDS * i);
    });
}
// out[i] = in[i]^-1 as k_invert_records runs it (in == out allowed)
void affine_sim_invert(const uint32_t *in, uint32_t *out, int count) {
    run_group([&](Ctx &c) {
        for (int i = 0; i < count; i++) qf_invert_record(c, in + (size_t)REC_WORDS * i, out + (size_t)REC_WORDS * i);
    });
}
// every slot of a column under a shape given field by field, the addend's three included:
// sel[4 s .. 4 s + 3] = table, position, signed digit, entry record (tables only, else 0)
void affine_sim_slots(const uint32_t *shape9, uint32_t h, const uint32_t *r_exp, const uint32_t *m_exp, int32_t *sel, uint32_t *n_slots) {
    CombShape s{};
    s.w = shape9[0];
    s.npos_r = shape9[1];
    s.npos_m = shape9[2];
    s.leaf = shape9[3];
    s.halves = shape9[4];
    s.kbits = shape9[5];
    s.c2_only = shape9[6];
    s.m_neg = shape9[7];
    s.leaf_inv = shape9[8];
    *n_slots = comb_slots(s);
    for (uint32_t k = 0; k < comb_slots(s); k++) {
        const CombSel c = comb_select(s, h, k, r_exp, m_exp);
        sel[4 * k + 0] = c.table;
        sel[4 * k + 1] = c.pos;
        sel[4 * k + 2] = c.digit;
        sel[4 * k + 3] = (c.table >= 0 && c.table <= 2) ? (int32_t)comb_entry(s, c) : 0;
    }
}
}
