// Host build of the grouped and dilated convolution's geometry and level-0 body (cofhe_amd/csrc/conv.hpp) on the simulated
// workgroup of sim.cpp.  TEST INFRASTRUCTURE ONLY; not linked into the product library.
#include "sim.cpp"       // the lane-group / workgroup simulator (run_workgroup) and COFHE_HOSTSIM

#include "../../cofhe_amd/csrc/conv.hpp"

// shape14 = B, H, W, C, kh, kw, Co, sh, sw, ph, pw, dh, dw, groups
static ConvShape shape_of(const uint32_t *a) {
    return ConvShape{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], a[9], a[10], 0u, 0u, a[11], a[12], a[13]};
}

extern "C" {
// Returns 0 and Ho, Wo, or 1 for a refused shape
int convg_sim_shape(const uint32_t *shape14, uint32_t *Ho, uint32_t *Wo) {
    ConvShape s = shape_of(shape14);
    if (conv_shape_check(s)) return 1;
    *Ho = s.Ho;
    *Wo = s.Wo;
    return 0;
}
// leaf[(row * m + j) * Co + col] = conv_leaf(row, j, col) for every row < n = B Ho Wo, j < m = kh kw C / groups and col < Co;
// leaf0[row * m + j] = the three-argument conv_leaf(row, j)
int convg_sim_leaves(const uint32_t *shape14, int64_t *leaf, int64_t *leaf0) {
    ConvShape s = shape_of(shape14);
    if (conv_shape_check(s)) return 1;
    const uint32_t n = conv_rows(s), m = conv_inner(s);
    for (uint32_t row = 0; row < n; row++)
        for (uint32_t j = 0; j < m; j++) {
            leaf0[(size_t)row * m + j] = conv_leaf(s, row, j);
            for (uint32_t col = 0; col < s.Co; col++) leaf[((size_t)row * m + j) * s.Co + col] = conv_leaf(s, row, j, col);
        }
    return 0;
}
// workgroup `wg` of a k_conv_level0 launch, as the kernel runs it
int convg_sim_level0(const uint32_t *shape14, uint32_t wg, const uint32_t *table, const uint32_t *one_rec, const uint32_t *ent0,
                     const uint32_t *off_cur, const uint32_t *off_next, const uint32_t *map_next, uint32_t n_next, uint32_t row0, uint32_t rows,
                     uint32_t tw, uint32_t *dst, int half_dbits, const uint32_t *absdelta) {
    ConvShape s = shape_of(shape14);
    if (conv_shape_check(s)) return 1;
    const QDisc dd{absdelta, half_dbits};
    run_workgroup([&](Ctx &c) { conv_level0_body(c, wg, s, table, one_rec, ent0, off_cur, off_next, map_next, n_next, row0, rows, tw, dst, dd); });
    return 0;
}
}
