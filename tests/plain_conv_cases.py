"""Cases of the plaintext convolution mod 2^k and of the transposed patch matrix of a plaintext image, shared by the CPU tier
(plain_conv.hpp on the host) and the GPU tier (k_plain_conv2d, k_gather_patch_exponents): geometries with groups = 1, operands
as exponent records, the expected values from Python integers on the numpy patch matrix of conv_groups_cases (written
independently of cofhe_amd/csrc/conv.hpp).  TEST INFRASTRUCTURE."""
import random

import numpy as np

import conv_groups_cases as CG
import plain_mm_cases as PM

KBITS = PM.KBITS
# id: (image [B, H, W, C], kernel (kh, kw), stride, pad, dilation, Co)
#   n15/n16/n17  n = B Ho Wo one below / at / one above the tile under 1 x 1 filters, Co one above / at / one below it
#   inner33      m = kh kw C = 33: two full steps of 16 and one element
#   distinct     distinct extents everywhere, a stride per axis, padding on one axis (n = 18, m = 18)
#   pad2         ph = 2 under kw C = 8: in the output rows with oy = 0 the first 16 patch columns -- a whole row of the first
#                left tile -- are padding (n = 24, m = 24)
#   dilated      dilation (2, 1) (n = 15, m = 8)
#   all_padding  both taps of the one dilated window lie in the padding: every output is zero
GEOMETRIES = {
    "n15": ((1, 5, 3, 1), (1, 1), (1, 1), (0, 0), (1, 1), 17),
    "n16": ((1, 4, 4, 1), (1, 1), (1, 1), (0, 0), (1, 1), 16),
    "n17": ((1, 17, 1, 1), (1, 1), (1, 1), (0, 0), (1, 1), 15),
    "inner33": ((1, 5, 2, 11), (3, 1), (1, 1), (0, 0), (1, 1), 3),
    "distinct": ((2, 5, 4, 3), (3, 2), (2, 1), (1, 0), (1, 1), 2),
    "pad2": ((1, 4, 3, 4), (3, 2), (1, 1), (2, 1), (1, 1), 3),
    "dilated": ((1, 5, 4, 2), (2, 2), (1, 1), (1, 0), (2, 1), 3),
    "all_padding": ((1, 1, 3, 2), (2, 1), (1, 1), (2, 0), (4, 1), 2),
}


def grouped_case(geo):
    """the geometry as a case of conv_groups_cases, groups = 1"""
    image, kernel, stride, pad, dilation, co = geo
    return (image, kernel, stride, pad, dilation, 1, co)


def sizes(geo):
    """n, m, p, Ho, Wo"""
    return CG.sizes(grouped_case(geo))


def shape14(geo, groups=1):
    image, kernel, stride, pad, dilation, co = geo
    return [*image, kernel[0], kernel[1], co, *stride, *pad, *dilation, groups]


def im2col(geo):
    """int64 [n, m]: the pixel index of element (row, j) of the patch matrix, -1 in the padding"""
    return CG.group_im2col(grouped_case(geo))[0]


def patch_values(geo, img):
    """the n x m patch matrix of the values img (flat list), 0 in the padding, row-major"""
    return [img[i] if i >= 0 else 0 for i in im2col(geo).reshape(-1)]


def expected(geo, img, w, k):
    n, m, p, _, _ = sizes(geo)
    return PM.product(patch_values(geo, img), w, n, m, p, k)


def cases(k):
    """[(name, geometry id, img, w)]: every geometry with the mixed operand family of plain_mm_cases (0, +-1, 2^k - 1, magnitudes of
    2^k and above, both signs), and 2^k - 1 / -1 everywhere (the longest carries) at two geometries"""
    rng = random.Random(2000 + k)
    out = []
    for gid, geo in GEOMETRIES.items():
        n_img = int(np.prod(geo[0]))
        n_w = geo[1][0] * geo[1][1] * geo[0][3] * geo[5]
        out.append(("mixed", gid, PM.operand(n_img, k, rng), PM.operand(n_w, k, rng)))
    top = (1 << k) - 1
    for gid in ("distinct", "pad2"):
        geo = GEOMETRIES[gid]
        n_img = int(np.prod(geo[0]))
        n_w = geo[1][0] * geo[1][1] * geo[0][3] * geo[5]
        out.append(("all_top", gid, [top] * n_img, [top] * n_w))
        out.append(("all_minus_one", gid, [-1] * n_img, [top] * n_w))
    return out
