"""The convolution's geometry in numpy, shared by tests/test_conv_cpu.py and tests/test_gpu_conv.py: the patch matrix (im2col)
of pixel indices, written independently of cofhe_amd/csrc/conv.hpp.  TEST INFRASTRUCTURE."""
import numpy as np

# (image [B, H, W, C], filter extents (kh, kw), stride, pad): one pixel; distinct extents, a stride per axis, padding on one
# axis; padding on all four sides (ph = kh - 1, pw = kw - 1); a stride larger than the filter; a filter equal to the padded image
GEOMETRIES = [
    ((1, 1, 1, 1), (1, 1), (1, 1), (0, 0)),
    ((2, 5, 4, 3), (3, 2), (2, 1), (1, 0)),
    ((2, 5, 4, 3), (3, 2), (1, 1), (2, 1)),
    ((1, 7, 6, 2), (2, 1), (3, 4), (0, 0)),
    ((2, 3, 2, 2), (5, 4), (1, 1), (1, 1)),
]


def out_extents(image, kernel, stride, pad):
    (_, H, W, _), (kh, kw) = image, kernel
    return (H + 2 * pad[0] - kh) // stride[0] + 1, (W + 2 * pad[1] - kw) // stride[1] + 1


def im2col(image, kernel, stride, pad):
    """int64 [n, m]: the flat pixel index ((b H + y) W + x) C + ci of element (row, j) of the patch matrix, -1 in the padding;
    row = (b Ho + oy) Wo + ox, j = (dy kw + dx) C + ci"""
    (B, H, W, C), (kh, kw), (sh, sw), (ph, pw) = image, kernel, stride, pad
    Ho, Wo = out_extents(image, kernel, stride, pad)
    padded = np.full((B, H + 2 * ph, W + 2 * pw, C), -1, dtype=np.int64)
    padded[:, ph:ph + H, pw:pw + W, :] = np.arange(B * H * W * C, dtype=np.int64).reshape(B, H, W, C)
    patches = np.empty((B, Ho, Wo, kh, kw, C), dtype=np.int64)
    for dy in range(kh):
        for dx in range(kw):
            patches[:, :, :, dy, dx, :] = padded[:, dy:dy + (Ho - 1) * sh + 1:sh, dx:dx + (Wo - 1) * sw + 1:sw, :]
    return patches.reshape(B * Ho * Wo, kh * kw * C)


def shape11(image, kernel, Co, stride, pad):
    return [*image, kernel[0], kernel[1], Co, stride[0], stride[1], pad[0], pad[1]]
