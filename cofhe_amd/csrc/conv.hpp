// conv.hpp -- the 2-D convolution of a ciphertext image with plaintext filters (conv.hip), in a header so that the host
// simulator of the CPU tests (tests/hostsim/conv_sim.cpp) compiles the very code the kernels run.
//
// Channels last, so that no operand is rearranged and a layer's output is the next layer's input:
//   image   [B, H, W, C] ciphertexts        filters [kh, kw, C/G, Co] exponent records      output [B, Ho, Wo, Co]
//   out[b,oy,ox,co] = zero o prod_{dy,dx,ci<Cg} image[b, oy sh + dy dh - ph, ox sw + dx dw - pw, g(co) Cg + ci] ^ w[dy,dx,ci,co]
// with G = groups, Cg = C / G, Cog = Co / G, g(co) = co / Cog, and the factors outside the image left out.  Read as matrices
// this is the n x m . m x p product of cofhe_hip_scal_matmul_records with rows (b, oy, ox), n = B Ho Wo, inner index
// j = (dy kw + dx) Cg + ci, m = kh kw Cg, and p = Co -- except that the n x m left operand (the patch matrix, im2col) is never
// written, and with groups is not one matrix at all (element (row, j) is a different pixel for columns of different groups):
// conv_leaf says which image pixel element (row, j) is for column col, the table of odd powers is built ONCE over the image,
// and level 0 of the product tree reads its leaves through conv_leaf (conv_level0_body: k_tree_level with from_table = 1 and
// the leaf address replaced; a segment of the tree belongs to one column, so the column costs one modulo).
// A leaf in the padding is the principal form, which contributes nothing; a dilated window may lie wholly in the padding and
// then gives zero.  G = C = Co is a depthwise convolution, with all-ones filters sum pooling (cofhe_hip_sum_pool2d_records),
// with kh = kw = 1 a per-channel scale.
//
// Not here: a per-channel bias (cofhe_hip_add_plain_records on the result) and max pooling.  Ciphertext filters over a
// plaintext image, and the plaintext convolution of their Beaver triplet: plain_conv.hpp, on this geometry.
#pragma once
#include "form_io.hpp"

namespace cofhe {

struct ConvShape {
    uint32_t B, H, W, C;          // the image
    uint32_t kh, kw, Co;          // the filters: kh x kw x C / groups x Co
    uint32_t sh, sw, ph, pw;      // strides and zero padding (rows, columns)
    uint32_t Ho, Wo;              // the output extents, filled by conv_shape_check
    uint32_t dh = 1, dw = 1;      // dilation: filter tap (dy, dx) sits dy dh rows and dx dw columns into the window
    uint32_t groups = 1;          // output column co reads channels (co / (Co / groups)) C / groups + ci, ci < C / groups
};

constexpr uint64_t CONV_PIXEL_LIMIT = 0x7FFFFFFFull;       // B H W C: a pixel index is a non-negative 32-bit number
constexpr uint64_t CONV_PATCH_LIMIT = 1ull << 40;          // n m: the patch matrix of the gather route is a tensor (formats' bound)

// validates a shape and fills Ho, Wo; returns null, or what is wrong with it (host)
inline const char *conv_shape_check(ConvShape &s) {
    s.Ho = s.Wo = 0;
    if (s.sh == 0 || s.sw == 0) return "conv2d: a stride is zero";
    if (s.dh == 0 || s.dw == 0) return "conv2d: a dilation is zero";
    if (s.groups == 0) return "conv2d: groups is zero";
    if (s.C % s.groups || s.Co % s.groups) return "conv2d: groups must divide the channels of the image and of the output";
    // the extent a dilated filter covers, (k - 1) d + 1: below 2^64, as both factors are below 2^32
    const uint64_t keh = s.kh ? (uint64_t)(s.kh - 1) * s.dh + 1 : 0, kew = s.kw ? (uint64_t)(s.kw - 1) * s.dw + 1 : 0;
    if (s.ph >= keh || s.pw >= kew) return "conv2d: padding must be smaller than the filter";
    const uint64_t Hp = (uint64_t)s.H + 2ull * s.ph, Wp = (uint64_t)s.W + 2ull * s.pw;
    if (keh > Hp || kew > Wp) return "conv2d: the filter is larger than the padded image";
    if (Hp > CONV_PIXEL_LIMIT || Wp > CONV_PIXEL_LIMIT) return "conv2d: image extent out of range";
    const uint64_t m = (uint64_t)s.kh * s.kw * (s.C / s.groups);      // kh <= Hp, kw <= Wp < 2^31, then < 2^62 2^32: checked stepwise
    if ((uint64_t)s.kh * s.kw >= (1ull << 21) || m >= (1ull << 21)) return "conv2d: inner dimension kh kw C / groups beyond 2^21";
    uint64_t pix = (uint64_t)s.B * s.H;
    if (pix <= CONV_PIXEL_LIMIT) pix *= s.W;
    if (pix <= CONV_PIXEL_LIMIT) pix *= s.C;
    if (pix > CONV_PIXEL_LIMIT) return "conv2d: the image has more than 2^31 - 1 pixels";
    const uint64_t Ho = (Hp - keh) / s.sh + 1, Wo = (Wp - kew) / s.sw + 1;
    uint64_t n = (uint64_t)s.B * Ho;                        // < 2^63
    if (n <= 0xFFFFFFFFull) n *= Wo;
    if (n > 0xFFFFFFFFull) return "conv2d: more than 2^32 - 1 output positions";
    if (n * m > CONV_PATCH_LIMIT) return "conv2d: the patch matrix n m is too large";
    if (n * s.Co > 0x7FFFFFFFull * (uint64_t)(WG_GROUPS / 2)) return "conv2d: work size out of range";       // 2 n p records, one group each
    s.Ho = (uint32_t)Ho;
    s.Wo = (uint32_t)Wo;
    return nullptr;
}
constexpr uint32_t conv_rows(const ConvShape &s) { return s.B * s.Ho * s.Wo; }
constexpr uint32_t conv_inner(const ConvShape &s) { return s.kh * s.kw * (s.C / s.groups); }
// the same geometry without its groups: what the gather route, whose patch matrix is dense over C, runs (Ho, Wo are kept)
inline ConvShape conv_dense(ConvShape s) {
    s.groups = 1;
    return s;
}

// THE geometry: element (row, j) of the patch matrix of output column col is image pixel ((b H + y) W + x) C + c, or -1 in
// the padding.  row = (b Ho + oy) Wo + ox, j = (dy kw + dx) Cg + ci, c = (col / Cog) Cg + ci.  Nine 32-bit divisions by runtime
// values, three of them the same for every thread: nothing next to a composition.
CF_DEV int64_t conv_leaf(const ConvShape &s, uint32_t row, uint32_t j, uint32_t col) {
    const uint32_t Cg = s.C / s.groups, Cog = s.Co / s.groups;
    const uint32_t ox = row % s.Wo, t = row / s.Wo, oy = t % s.Ho, b = t / s.Ho;
    const uint32_t ci = j % Cg, u = j / Cg, dx = u % s.kw, dy = u / s.kw;
    const uint32_t y = oy * s.sh + dy * s.dh, x = ox * s.sw + dx * s.dw;      // in the padded image: < H + 2 ph, W + 2 pw < 2^31
    if (y < s.ph || y - s.ph >= s.H || x < s.pw || x - s.pw >= s.W) return -1;
    return (((int64_t)b * s.H + (y - s.ph)) * s.W + (x - s.pw)) * s.C + (col / Cog) * Cg + ci;
}
// column 0: the whole geometry when groups = 1, where every column reads the same pixel
CF_DEV int64_t conv_leaf(const ConvShape &s, uint32_t row, uint32_t j) { return conv_leaf(s, row, j, 0); }

// "does any thread of the workgroup say so": __syncthreads_or, and its counterpart on the simulated workgroup
#if defined(COFHE_HOSTSIM)
inline std::atomic<unsigned> g_conv_vote{0};
inline bool conv_wg_any(Ctx &c, bool p) {
    if (p) g_conv_vote.fetch_or(1u);
    CF_WG_BARRIER(c);
    const bool any = g_conv_vote.load() != 0;
    CF_WG_BARRIER(c);
    if (c.tid == 0) g_conv_vote.store(0);
    CF_WG_BARRIER(c);
    return any;
}
#else
CF_DEV bool conv_wg_any(Ctx &, bool p) { return __syncthreads_or(p ? 1 : 0) != 0; }
#endif

// Level 0 -> 1 of the product trees of the chunk of `rows` rows that starts at row0, for workgroup `wg` of the launch
// (every thread of it calls this).  k_tree_level (cofhe_hip.hip) with from_table = 1, word for word, but for the leaf:
// work item g = (u, i, h), u slowest; element u of level 1 (segment sgm = map_next[u], q = u - off_next[sgm]) is the product
// of leaves 2 q and 2 q + 1 of the segment, or a copy of leaf 2 q when that is its last.  Leaf e is the word ent0[e] =
// j << 8 | negative << 7 | |digit| >> 1: entry idx = |digit| >> 1 of the table of pixel conv_leaf(row0 + i, j), half h --
// table[(leaf 2 + h) tw + idx] -- inverted when negative, or the principal form when the leaf is padding.  The rows of a
// chunk share the ONE table of the image, so the chunk is named by row0 and not by an offset into the table.  Segment
// sgm = t Co + col is bit position t of output column col, which names the group the leaf's channel lies in: the eight lanes
// of a limb group share g and so sgm, and the modulo is uniform within the group like everything before it.
CF_DEV void conv_level0_body(Ctx &c, uint64_t wg, const ConvShape &s, const uint32_t *__restrict__ table, const uint32_t *__restrict__ one_rec,
                             const uint32_t *__restrict__ ent0, const uint32_t *__restrict__ off_cur, const uint32_t *__restrict__ off_next,
                             const uint32_t *__restrict__ map_next, uint32_t n_next, uint32_t row0, uint32_t rows, uint32_t tw,
                             uint32_t *__restrict__ dst, const QDisc &dd) {
    const uint64_t total = (uint64_t)n_next * rows * 2;
    const uint64_t g0 = wg * WG_GROUPS + (uint32_t)c.gi;
    const uint64_t g = g0 < total ? g0 : total - 1;              // beyond the work: recompute the last item, store nothing
    const uint32_t ih = (uint32_t)(g % ((uint64_t)rows * 2)), u = (uint32_t)(g / ((uint64_t)rows * 2));
    const uint32_t i = ih >> 1, h = ih & 1u;
    const uint32_t sgm = map_next[u], q = u - off_next[sgm];
    const uint32_t base = off_cur[sgm], cnt = off_cur[sgm + 1] - base;
    const uint32_t col = sgm % s.Co;
    const bool paired = 2 * q + 1 < cnt;
    QForm a, b, r;
    auto element = [&](QForm &f, uint32_t e) {
        const uint32_t w = ent0[e];
        const int64_t leaf = conv_leaf(s, row0 + i, w >> 8, col);
        qf_load(c, f, leaf < 0 ? one_rec : table + (((uint64_t)leaf * 2 + h) * tw + (w & 0x7Fu)) * REC_WORDS);
        if (w & 0x80u) qf_inverse(c, f);
    };
    element(a, base + 2 * q);
    uint32_t *out = dst + (((uint64_t)i * n_next + u) * 2 + h) * REC_WORDS;
    if (!conv_wg_any(c, paired)) {                               // a workgroup of copies
        if (g0 < total) qf_store(c, a, out);
        return;
    }
    if (paired) element(b, base + 2 * q + 1); else b = a;
    qf_compose<true, false, false>(c, r, a, b, dd);
    if (g0 < total) qf_store(c, paired ? r : a, out);
}

}  // namespace cofhe
