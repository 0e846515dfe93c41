"""CPU: the convolution without a GPU.  conv_leaf (cofhe_amd/csrc/conv.hpp) against a numpy im2col, the shape check behind
cofhe_hip_conv2d_out_shape and each of its refusals, the body of k_conv_level0 on the host simulator's 32-group workgroup
against the pure-Python model, and how the direct route carves the workspace (cofhe_hip_workspace_plan "conv2d").  No kernel
runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_cases as CC
import simlib as S
from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libconvsim.so")
REC = S.REC_WORDS
REC_BYTES = REC * 4
EINVAL = -1


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def t3(x):
    return (x.a, x.b, x.c)


def u32(vals):
    return np.array(vals, dtype=np.uint32)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "conv_sim.cpp")
    deps = [src, os.path.join(HERE, "hostsim", "sim.cpp")] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in
                                                              ("conv.hpp", "qf.hpp", "mp.hpp", "lane.hpp", "form_io.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        # the kernels' workgroup geometry: 32 groups = 256 host threads = four wavefronts
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-DCOFHE_WG_GROUPS=32", "-o", _SO, src])
    L = C.CDLL(_SO)
    assert L.sim_wg_groups() == 32
    return L


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from cofhe_amd import load_library
    return load_library()


@pytest.mark.parametrize("image,kernel,stride,pad", CC.GEOMETRIES)
def test_conv_leaf_is_the_numpy_im2col(sim, image, kernel, stride, pad):
    """every (row, j) of the five geometries: the pixel index, or -1 in the padding; and the extents the shape check fills"""
    want = CC.im2col(image, kernel, stride, pad)
    sh = u32(CC.shape11(image, kernel, 1, stride, pad))
    ho, wo = C.c_uint32(), C.c_uint32()
    assert sim.conv_sim_shape(S.P(sh), C.byref(ho), C.byref(wo)) == 0
    assert (ho.value, wo.value) == CC.out_extents(image, kernel, stride, pad)
    got = np.full(want.shape, -7, dtype=np.int64)
    assert sim.conv_sim_leaves(S.P(sh), got.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(got, want)
    if pad != (0, 0):
        assert (want < 0).any()
    assert (want >= 0).any(axis=1).all()                 # every window holds a real pixel


def test_geometries_are_what_the_docstring_says():
    g = CC.GEOMETRIES
    assert CC.out_extents(*g[1][:2], g[1][2], g[1][3]) == (3, 3)
    assert g[2][3] == (g[2][1][0] - 1, g[2][1][1] - 1)                                          # padding on all four sides
    assert g[3][2][0] > g[3][1][0] and g[3][2][1] > g[3][1][1]                                  # stride larger than the filter
    assert CC.out_extents(*g[4][:2], g[4][2], g[4][3]) == (1, 1)                                # the filter is the padded image


REFUSALS = {
    "sh = 0": ((1, 4, 4, 1), (2, 2), 1, (0, 1), (0, 0)),
    "sw = 0": ((1, 4, 4, 1), (2, 2), 1, (1, 0), (0, 0)),
    "ph >= kh": ((1, 4, 4, 1), (2, 2), 1, (1, 1), (2, 0)),
    "pw >= kw": ((1, 4, 4, 1), (2, 3), 1, (1, 1), (0, 3)),
    "kh > H + 2 ph": ((1, 2, 4, 1), (5, 2), 1, (1, 1), (1, 0)),
    "kw > W + 2 pw": ((1, 4, 2, 1), (2, 3), 1, (1, 1), (0, 0)),
    "m = 2^21": ((1, 2048, 2048, 2), (1024, 1024), 1, (1, 1), (0, 0)),
    "B H W C = 2^31": ((1 << 16, 1 << 15, 1, 1), (1, 1), 1, (1, 1), (0, 0)),
    "n = 2^33": (((1 << 31) - 1, 1, 1, 1), (2, 2), 1, (1, 1), (1, 1)),
    "n m > 2^40": ((1, 1 << 15, 1 << 15, 1), (1024, 1024), 1, (1, 1), (0, 0)),
    "2 n p beyond the launch limit": ((1, 1 << 15, 1 << 15, 1), (1, 1), 64, (1, 1), (0, 0)),
}


def test_out_shape_and_each_refusal(lib):
    """cofhe_hip_conv2d_out_shape: Ho = (H + 2 ph - kh) / sh + 1 rounded down on the five geometries, COFHE_HIP_EINVAL with the
    outputs untouched for each refusal, and the largest shapes on the right side of each bound accepted"""
    from cofhe_amd import CofheHipError, engine
    for image, kernel, stride, pad in CC.GEOMETRIES:
        assert engine.conv2d_out_shape(image, (*kernel, image[3], 2), stride, pad) == CC.out_extents(image, kernel, stride, pad)
    for why, (image, kernel, co, stride, pad) in REFUSALS.items():
        with pytest.raises(CofheHipError) as ei:
            engine.conv2d_out_shape(image, (*kernel, image[3], co), stride, pad)
        assert ei.value.code == EINVAL, why
        # the records entry refuses the same before it looks at its context or its pointers
        shp = engine._conv_shape(image, (*kernel, image[3], co), stride, pad)
        assert lib.cofhe_hip_conv2d_plain_ct_records(None, None, None, None, None, C.byref(shp), None) == EINVAL, why
    assert engine.conv2d_out_shape((1, 2048, 2048, 1), (1024, 1024, 1, 1), (1024, 1024), (0, 0)) == (2, 2)          # m = 2^20
    assert engine.conv2d_out_shape(((1 << 16) - 1, 1 << 15, 1, 1), (1, 1, 1, 1)) == (1 << 15, 1)                    # B H W C = 2^31 - 2^15
    assert engine.conv2d_out_shape((1, 1 << 15, 1 << 15, 1), (1, 1, 1, 31)) == (1 << 15, 1 << 15)                   # 2 n p = 62 2^30
    with pytest.raises(CofheHipError) as ei:
        engine.conv2d_out_shape((1, 4, 4, 3), (2, 2, 2, 1))
    assert ei.value.code == -2                                                                                     # channels differ: ESHAPE


# ---- the level-0 body --------------------------------------------------------------------------------------------------------

IMAGE, KERNEL, STRIDE, PAD = (1, 3, 3, 2), (2, 2), (1, 1), (1, 1)          # n = 16 rows, m = 8; rows 1..4 touch the top and left padding
TW = 8
ROW0, ROWS = 1, 4
COUNTS = [2, 1, 5, 0, 4, 3]            # leaves per segment: level 1 has 1, 1, 3, 0, 2, 2 elements; the last one is a copy


def level0_case():
    """ent0, the offsets and the map of a hand-made level 0; ent0 words j << 8 | negative << 7 | idx"""
    # (j, j') pairs chosen by where they fall for rows 1..3 (oy = 0: dy = 0, j < 4, is padding) and row 4 (oy = 1, ox = 0: dx = 0,
    # j in {0, 1, 4, 5}, is padding): first operand padding, second operand padding, both, neither
    js = [0, 6,   7,   6, 2, 0, 1, 3,   5, 7, 4, 6,   2, 7, 6]
    assert len(js) == sum(COUNTS)
    ent0 = [(j << 8) | ((0 if i % 3 == 1 else 1) << 7) | ((3 * i + 1) % TW) for i, j in enumerate(js)]
    off_cur = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint32)
    nxt = [(c + 1) // 2 for c in COUNTS]
    off_next = np.concatenate([[0], np.cumsum(nxt)]).astype(np.uint32)
    map_next = u32([s for s, c in enumerate(nxt) for _ in range(c)])
    return u32(ent0), off_cur, off_next, map_next


@pytest.mark.parametrize("name", ["tiny_k8", "s128_k128"])
def test_level0_body_on_workgroups_of_32(sim, name):
    """conv_level0_body for every workgroup of a launch over rows 1..4 (row0 = 1) of a padded 3 x 3 x 2 image with a table of
    tw = 8 entries per pixel: 72 work items in workgroups of 32, 32 and a ragged 8.  The first two mix paired elements and
    copies (one composition for all, the copies ride along), the last holds only copies (the shortcut).  Among the pairs: a
    padding leaf as the first operand, as the second, as both; negative digits on table leaves and on padding; entries
    idx > 0.  Expected: the table record of pixel conv_leaf(row, j) -- from the numpy im2col -- inverted where the word says
    so, the principal form in the padding, composed in the model's arithmetic.  Records outside the launch's 72 stay as
    they were; the simulator's status word stays 0"""
    prm = load_json("params_%s.json" % name)
    d = hx(prm["delta"])
    rng = P.SplitMix64(99 + prm["k"])
    pool = [P.random_form(d, rng, 12, 10) for _ in range(20)] if name == "tiny_k8" else [P.random_form(d, rng) for _ in range(20)]
    pixels = int(np.prod(IMAGE))
    table = [pool[rng.below(len(pool))] for _ in range(pixels * 2 * TW)]
    one = P.identity(d)
    ent0, off_cur, off_next, map_next = level0_case()
    n_next = int(off_next[-1])
    cols = CC.im2col(IMAGE, KERNEL, STRIDE, PAD)
    half = ((-d).bit_length() + 1) // 2
    ad = S.to_limbs(-d, 80)
    trec = np.concatenate([S.form_record(*t3(x)) for x in table])
    orec = S.form_record(*t3(one))
    total = n_next * ROWS * 2
    dst = np.full((total + 3) * REC, 0xA5A5A5A5, dtype=np.uint32)
    sh = u32(CC.shape11(IMAGE, KERNEL, 1, STRIDE, PAD))
    for wg in range((total + 31) // 32):
        assert sim.conv_sim_level0(S.P(sh), C.c_uint32(wg), S.P(trec), S.P(orec), S.P(ent0), S.P(off_cur), S.P(off_next), S.P(map_next),
                                   C.c_uint32(n_next), C.c_uint32(ROW0), C.c_uint32(ROWS), C.c_uint32(TW), S.P(dst), half, S.P(ad)) == 0
    assert sim.sim_status() == 0
    assert (dst[total * REC:] == 0xA5A5A5A5).all()

    seen = set()

    def leaf(e, i, h):
        w = int(ent0[e])
        j, neg, idx = w >> 8, (w >> 7) & 1, w & 0x7F
        px = int(cols[ROW0 + i, j])
        f = one if px < 0 else table[(px * 2 + h) * TW + idx]
        seen.add(("pad" if px < 0 else "real", "neg" if neg else "pos", "idx>0" if idx else "idx0"))
        return (P.inverse(f) if neg else f), px < 0

    kinds = {}
    for u in range(n_next):
        s = int(map_next[u])
        q = u - int(off_next[s])
        base, cnt = int(off_cur[s]), int(off_cur[s + 1] - off_cur[s])
        for i in range(ROWS):
            for h in range(2):
                a, pa = leaf(base + 2 * q, i, h)
                if 2 * q + 1 < cnt:
                    b, pb = leaf(base + 2 * q + 1, i, h)
                    want = P.compose(a, b)
                    kinds[(pa, pb)] = kinds.get((pa, pb), 0) + 1
                else:
                    want = a
                    kinds["copy"] = kinds.get("copy", 0) + 1
                g = (u * ROWS + i) * 2 + h
                o = ((i * n_next + u) * 2 + h) * REC
                assert S.record_form(dst[o:o + REC]) == t3(want), (u, i, h, g // 32)
    # the situations the docstring names all occurred
    assert all(kinds.get(k, 0) > 0 for k in [(True, False), (False, True), (True, True), (False, False), "copy"]), kinds
    assert {("pad", "neg", "idx>0"), ("real", "neg", "idx>0"), ("real", "pos", "idx>0")} <= seen
    items = [(int(map_next[g // (2 * ROWS)]), g // (2 * ROWS)) for g in range(total)]
    paired = [2 * (u - int(off_next[s])) + 1 < COUNTS[s] for s, u in items]
    assert any(paired[:32]) and not all(paired[:32]) and not any(paired[64:])             # a mixed workgroup, and one of copies


# ---- the workspace plan ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("image,kernel,stride,pad", CC.GEOMETRIES + [((8, 56, 56, 64), (3, 3), (1, 1), (1, 1))])
def test_workspace_plan_of_the_direct_route(lib, image, kernel, stride, pad, w):
    """"conv2d": the table holds 2^(w-2) records for each of the B H W C 2 image records -- pixels, not patches -- and nothing at
    w = 2, where the image is the table; the other regions are those of "scal_matmul_tree" for n = B Ho Wo, m = kh kw C, p = Co;
    regions are 256-byte aligned, ordered and disjoint.  The total is below the tree plan of the matrix product on the patch
    matrix whenever that matrix is larger than the image (n m > B H W C: every geometry here whose windows overlap), by the
    difference of the two tables"""
    from cofhe_amd import engine
    co, bits = 5, 16
    regs, total = engine.workspace_plan("conv2d", *CC.shape11(image, kernel, co, stride, pad), bits, w)
    ho, wo = CC.out_extents(image, kernel, stride, pad)
    n, m = image[0] * ho * wo, kernel[0] * kernel[1] * image[3]
    pixels = int(np.prod(image))
    tw = 1 << (w - 2)
    r = {name: (off, nbytes) for name, off, nbytes in regs}
    assert r["table"] == (0, pixels * 2 * tw * REC_BYTES if w > 2 else 0)
    end = 0
    for name, off, nbytes in regs:
        assert off % 256 == 0 and off >= end, name
        end = off + nbytes
    assert end == total
    tregs, ttotal = engine.workspace_plan("scal_matmul_tree", n, m, co, bits, w)
    assert [(name, nbytes) for name, _, nbytes in regs[1:]] == [(name, nbytes) for name, _, nbytes in tregs[1:]]
    assert tregs[0][2] == (n * m * 2 * tw * REC_BYTES if w > 2 else 0)
    if w > 2 and n * m > pixels:
        assert total < ttotal and abs((ttotal - total) - (n * m - pixels) * 2 * tw * REC_BYTES) < 256
    if w == 4 and kernel == (3, 3):
        assert n * m == 9 * pixels and 76e9 < tregs[0][2] < 78e9 and 8.5e9 < r["table"][1] < 8.7e9          # the flagship layer at w = 4


def test_workspace_plan_refuses_what_the_entry_point_refuses(lib):
    from cofhe_amd import CofheHipError, engine
    for why, (image, kernel, co, stride, pad) in REFUSALS.items():
        with pytest.raises(CofheHipError):
            engine.workspace_plan("conv2d", *CC.shape11(image, kernel, co, stride, pad), 16, 4)
    for w in (1, 9):
        with pytest.raises(CofheHipError):
            engine.workspace_plan("conv2d", *CC.shape11((2, 5, 4, 3), (3, 2), 2, (2, 1), (1, 0)), 16, w)
