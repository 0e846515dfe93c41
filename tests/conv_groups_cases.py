"""The grouped and dilated convolution's geometry in numpy, shared by tests/test_conv_groups_cpu.py and
tests/test_gpu_conv_groups.py: per output column, the patch matrix (im2col) of pixel indices, written independently of
cofhe_amd/csrc/conv.hpp.  TEST INFRASTRUCTURE."""
import numpy as np

# id: (image [B, H, W, C], kernel (kh, kw), stride, pad, dilation, groups, Co).  Extents are distinct everywhere, Cg != Cog != G:
# A depthwise; B Cg = 2, Cog = 3 (n = 9, m = 12); C channel multiplier 2 (Cg = 1); D dilation only (Ho = Wo = 6); E the single
# output row's window lies wholly in the padding; F a per-channel scale (m = 1)
CASES = {
    "A": ((2, 5, 4, 3), (3, 2), (2, 1), (1, 0), (1, 1), 3, 3),
    "B": ((1, 4, 5, 4), (2, 3), (1, 2), (0, 1), (1, 1), 2, 6),
    "C": ((1, 3, 3, 2), (2, 2), (1, 1), (1, 1), (1, 1), 2, 4),
    "D": ((2, 6, 5, 2), (2, 2), (1, 1), (1, 2), (2, 3), 1, 2),
    "E": ((1, 1, 3, 2), (2, 1), (1, 1), (2, 0), (4, 1), 2, 2),
    "F": ((1, 4, 4, 3), (1, 1), (1, 1), (0, 0), (1, 1), 3, 3),
}


def out_extents(image, kernel, stride, pad, dilation):
    ke = [(k - 1) * d + 1 for k, d in zip(kernel, dilation)]
    return tuple((image[1 + a] + 2 * pad[a] - ke[a]) // stride[a] + 1 for a in (0, 1))


def sizes(case):
    """n, m, p, Ho, Wo"""
    image, kernel, stride, pad, dilation, groups, co = case
    ho, wo = out_extents(image, kernel, stride, pad, dilation)
    return image[0] * ho * wo, kernel[0] * kernel[1] * (image[3] // groups), co, ho, wo


def group_im2col(case):
    """int64 [G, n, m]: the flat pixel index ((b H + y) W + x) C + g Cg + ci of element (row, j) of group g's patch matrix, -1 in
    the padding; row = (b Ho + oy) Wo + ox, j = (dy kw + dx) Cg + ci"""
    (B, H, W, C), (kh, kw), (sh, sw), (ph, pw), (dh, dw), G, _ = case
    Cg = C // G
    Ho, Wo = out_extents(case[0], case[1], case[2], case[3], case[4])
    padded = np.full((B, H + 2 * ph, W + 2 * pw, C), -1, dtype=np.int64)
    padded[:, ph:ph + H, pw:pw + W, :] = np.arange(B * H * W * C, dtype=np.int64).reshape(B, H, W, C)
    patches = np.empty((G, B, Ho, Wo, kh, kw, Cg), dtype=np.int64)
    for g in range(G):
        for dy in range(kh):
            for dx in range(kw):
                y0, x0 = dy * dh, dx * dw
                patches[g, :, :, :, dy, dx, :] = padded[:, y0:y0 + (Ho - 1) * sh + 1:sh, x0:x0 + (Wo - 1) * sw + 1:sw, g * Cg:(g + 1) * Cg]
    return patches.reshape(G, B * Ho * Wo, kh * kw * Cg)


def column_im2col(case):
    """int64 [n, m, Co]: group_im2col by output column, column co in group co // (Co / G)"""
    G, co = case[5], case[6]
    per_group = group_im2col(case)
    return np.stack([per_group[c // (co // G)] for c in range(co)], axis=2)


def shape14(case, co=None):
    image, kernel, stride, pad, dilation, groups, c_o = case
    return [*image, kernel[0], kernel[1], c_o if co is None else co, *stride, *pad, *dilation, groups]


def filters_of(case):
    image, kernel, _, _, _, groups, co = case
    return (kernel[0], kernel[1], image[3] // groups, co)


def dense_filter(case, w):
    """the block-diagonal dense [kh, kw, C, Co] filter (flat list) of the grouped [kh, kw, Cg, Co] filter w (flat list)"""
    image, kernel, _, _, _, G, co = case
    C = image[3]
    Cg, Cog = C // G, co // G
    out = []
    for t in range(kernel[0] * kernel[1]):
        for c in range(C):
            for o in range(co):
                out.append(w[(t * Cg + c % Cg) * co + o] if c // Cg == o // Cog else 0)
    return out
