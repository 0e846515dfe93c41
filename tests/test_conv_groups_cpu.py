"""CPU: groups and dilation of the convolution without a GPU.  conv_leaf(s, row, j, col) (cofhe_amd/csrc/conv.hpp) against a
numpy grouped and dilated im2col, the output extents, each new refusal of the shape check behind
cofhe_hip_conv2d_geometry_out_shape, the body of k_conv_level0 with segments of several columns and groups on the host
simulator's 32-group workgroup against the pure-Python model, and cofhe_hip_workspace_plan "conv2d_grouped".  No kernel runs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import conv_cases as CC
import conv_groups_cases as CG
import simlib as S
from conftest import ROOT, load_json

sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libconvgroupssim.so")
REC = S.REC_WORDS
REC_BYTES = REC * 4
EINVAL, ESHAPE = -1, -2


def hx(s):
    return -int(s[1:], 16) if s.startswith("-") else int(s, 16)


def t3(x):
    return (x.a, x.b, x.c)


def u32(vals):
    return np.array(vals, dtype=np.uint32)


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "conv_groups_sim.cpp")
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


def test_the_cases_are_what_the_table_says():
    for name, case in CG.CASES.items():
        image, kernel, stride, pad, dilation, G, co = case
        assert image[3] % G == 0 and co % G == 0, name
    assert CG.sizes(CG.CASES["B"])[:3] == (9, 12, 6)
    assert CG.sizes(CG.CASES["D"])[3:] == (6, 6)
    assert CG.sizes(CG.CASES["E"])[3:] == (1, 3) and (CG.group_im2col(CG.CASES["E"]) < 0).all()          # nothing but padding
    assert CG.sizes(CG.CASES["F"])[1] == 1
    for name in "ABC":                                      # every other case has a window with a real pixel everywhere
        assert (CG.group_im2col(CG.CASES[name]) >= 0).any(axis=2).all(), name


@pytest.mark.parametrize("name", sorted(CG.CASES))
def test_conv_leaf_is_the_numpy_grouped_im2col(sim, name):
    """every (row, j, col) of the six cases: the pixel index, or -1 in the padding; the extents the shape check fills; and the
    three-argument conv_leaf is column 0"""
    case = CG.CASES[name]
    want = CG.column_im2col(case)
    n, m, p, ho, wo = CG.sizes(case)
    assert want.shape == (n, m, p)
    sh = u32(CG.shape14(case))
    got_ho, got_wo = C.c_uint32(), C.c_uint32()
    assert sim.convg_sim_shape(S.P(sh), C.byref(got_ho), C.byref(got_wo)) == 0
    assert (got_ho.value, got_wo.value) == (ho, wo)
    got = np.full(want.shape, -7, dtype=np.int64)
    got0 = np.full((n, m), -7, dtype=np.int64)
    assert sim.convg_sim_leaves(S.P(sh), got.ctypes.data_as(C.c_void_p), got0.ctypes.data_as(C.c_void_p)) == 0
    assert np.array_equal(got, want)
    assert np.array_equal(got0, want[:, :, 0])
    if case[5] > 1 and name != "E":
        assert not np.array_equal(want[:, :, 0], want[:, :, p - 1])              # the groups read different pixels


def test_ungrouped_undilated_geometry_is_the_old_one(sim):
    """dh = dw = groups = 1 through the new arguments: the im2col of tests/conv_cases.py in every column"""
    for image, kernel, stride, pad in CC.GEOMETRIES:
        case = (image, kernel, stride, pad, (1, 1), 1, 2)
        want = CC.im2col(image, kernel, stride, pad)
        got = np.full((*want.shape, 2), -7, dtype=np.int64)
        got0 = np.full(want.shape, -7, dtype=np.int64)
        assert sim.convg_sim_leaves(S.P(u32(CG.shape14(case))), got.ctypes.data_as(C.c_void_p), got0.ctypes.data_as(C.c_void_p)) == 0
        assert np.array_equal(got[:, :, 0], want) and np.array_equal(got[:, :, 1], want) and np.array_equal(got0, want)


# why: (image, kernel, Co, stride, pad, dilation, groups)
REFUSALS = {
    "dh = 0": ((1, 4, 4, 2), (2, 2), 2, (1, 1), (0, 0), (0, 1), 1),
    "dw = 0": ((1, 4, 4, 2), (2, 2), 2, (1, 1), (0, 0), (1, 0), 1),
    "groups = 0": ((1, 4, 4, 2), (2, 2), 2, (1, 1), (0, 0), (1, 1), 0),
    "C % groups": ((1, 4, 4, 3), (2, 2), 2, (1, 1), (0, 0), (1, 1), 2),
    "Co % groups": ((1, 4, 4, 2), (2, 2), 3, (1, 1), (0, 0), (1, 1), 2),
    "ph >= keff_h": ((1, 4, 4, 2), (2, 2), 2, (1, 1), (3, 0), (2, 1), 2),
    "pw >= keff_w": ((1, 4, 4, 2), (2, 2), 2, (1, 1), (0, 4), (1, 3), 2),
    "keff_h > H + 2 ph": ((1, 4, 4, 2), (3, 2), 2, (1, 1), (0, 0), (2, 1), 2),
    "keff_w > W + 2 pw": ((1, 4, 4, 2), (2, 3), 2, (1, 1), (0, 1), (1, 3), 2),
    "keff_h beyond 32 bits": ((1, 4, 4, 2), (3, 1), 2, (1, 1), (0, 0), (0xFFFFFFFF, 1), 2),
    "grouped m = 2^21": ((1, 2048, 2048, 4), (1024, 1024), 2, (1024, 1024), (0, 0), (1, 1), 2),
}


def geometry(image, kernel, co, stride, pad, dilation, groups):
    from cofhe_amd import engine
    return engine._ConvGeometry(*image, kernel[0], kernel[1], co, *stride, *pad, *dilation, groups)


def test_geometry_out_shape_and_each_new_refusal(lib):
    """cofhe_hip_conv2d_geometry_out_shape: the extents of A-F, COFHE_HIP_EINVAL for each new refusal, from the records entry
    too, which refuses before it looks at its context or its pointers; the shapes next to each bound accepted; the limits
    charged on the grouped inner dimension"""
    from cofhe_amd import CofheHipError, engine
    for name, case in CG.CASES.items():
        image, kernel, stride, pad, dilation, G, co = case
        assert engine.conv2d_out_shape(image, CG.filters_of(case), stride, pad, dilation, G) == CG.sizes(case)[3:], name
    for why, (image, kernel, co, stride, pad, dilation, G) in REFUSALS.items():
        geo = geometry(image, kernel, co, stride, pad, dilation, G)
        ho, wo = C.c_uint32(77), C.c_uint32(78)
        assert lib.cofhe_hip_conv2d_geometry_out_shape(C.byref(geo), C.byref(ho), C.byref(wo)) == EINVAL, why
        assert (ho.value, wo.value) == (77, 78), why
        assert lib.cofhe_hip_conv2d_grouped_plain_ct_records(None, None, None, None, None, C.byref(geo), None) == EINVAL, why
        if "groups" not in why and "grouped" not in why:           # pooling takes Co and groups from C
            assert lib.cofhe_hip_sum_pool2d_records(None, None, None, None, C.byref(geo), None) == EINVAL, why
        if G > 0 and image[3] % G == 0:
            with pytest.raises(CofheHipError) as ei:
                engine.conv2d_out_shape(image, (*kernel, image[3] // G, co), stride, pad, dilation, G)
            assert ei.value.code == EINVAL, why
    # padding up to keff - 1 is legal with a dilated filter, where it was not with a dense one
    assert engine.conv2d_out_shape((1, 4, 4, 2), (2, 2, 1, 2), (1, 1), (2, 0), (2, 1), 2) == (6, 3)
    with pytest.raises(CofheHipError):
        engine.conv2d_out_shape((1, 4, 4, 2), (2, 2, 2, 2), (1, 1), (2, 0))
    assert engine.conv2d_out_shape((1, 5, 4, 2), (3, 2, 1, 2), (1, 1), (0, 0), (2, 1), 2) == (1, 3)                  # keff_h = H
    # the dense filter of this depthwise layer would have m = 2^21: refused ungrouped, accepted with two groups (m = 2^20)
    big = ((1, 2048, 2048, 2), (1024, 1024), (1024, 1024), (0, 0))
    with pytest.raises(CofheHipError):
        engine.conv2d_out_shape(big[0], (1024, 1024, 2, 2), big[2], big[3])
    assert engine.conv2d_out_shape(big[0], (1024, 1024, 1, 2), big[2], big[3], (1, 1), 2) == (2, 2)
    # the third filter extent is C / groups: ESHAPE from Python
    for filters, G in (((2, 2, 4, 6), 2), ((2, 2, 1, 6), 2), ((2, 2, 2, 6), 1)):
        with pytest.raises(CofheHipError) as ei:
            engine.conv2d_out_shape((1, 4, 5, 4), filters, (1, 1), (0, 0), (1, 1), G)
        assert ei.value.code == ESHAPE


# ---- the level-0 body --------------------------------------------------------------------------------------------------------

CASE_B = CG.CASES["B"]                 # n = 9 rows (Ho = Wo = 3), m = 12, Co = 6 in two groups: columns 0..2 read channels 0, 1; 3..5 channels 2, 3
TW = 8
ROW0, ROWS = 1, 5                      # rows 1..5: ox = 1, 2, 0, 1, 2 -- ox = 0 has dx = 0 in the padding, ox = 2 has dx = 2
# leaves per segment, segment = bit position * Co + column: two bit positions, so that segments 6..11 (sgm >= Co) occur;
# level 1 has 1, 1, 2, 0, 2, 1, 1, 2, 1, 1, 1, 1 elements, the last four of them copies
COUNTS = [2, 1, 4, 0, 3, 2, 2, 4, 1, 1, 1, 1]


def level0_case():
    """ent0, the offsets and the map of a hand-made level 0; ent0 words j << 8 | negative << 7 | idx.  j = (dy 3 + dx) 2 + ci:
    dx = 0 is j in {0, 1, 6, 7}, dx = 2 is j in {4, 5, 10, 11}, dx = 1 (never padding) the rest"""
    js = [0, 2,   6,   2, 0, 0, 6,   2, 3, 7,   4, 10,   3, 8,   1, 9, 5, 11,   2,   0,   11,   8]
    assert len(js) == sum(COUNTS)
    ent0 = [(j << 8) | ((0 if i % 3 == 1 else 1) << 7) | ((3 * i + 1) % TW) for i, j in enumerate(js)]
    off_cur = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.uint32)
    nxt = [(c + 1) // 2 for c in COUNTS]
    off_next = np.concatenate([[0], np.cumsum(nxt)]).astype(np.uint32)
    map_next = u32([s for s, c in enumerate(nxt) for _ in range(c)])
    return u32(ent0), off_cur, off_next, map_next


@pytest.mark.parametrize("name", ["tiny_k8", "s128_k128"])
def test_level0_body_reads_each_columns_group(sim, name):
    """conv_level0_body for every workgroup of a launch over rows 1..5 of case B with a table of tw = 8 entries per pixel and
    twelve segments over two bit positions: 140 work items in workgroups of 32, 32, 32, 32 and a ragged 12.  Segment sgm is
    column sgm % 6, in group (sgm % 6) / 3: the leaf of (row, j) is a different pixel for columns of different groups.  Among the
    pairs: a padding leaf as the first operand, as the second, as both, as neither; negative digits; entries idx > 0; a mixed
    workgroup; a workgroup of copies.  Expected: the table record of the pixel the numpy grouped im2col names, inverted where
    the word says so, the principal form in the padding, composed in the model's arithmetic.  Records beyond the launch stay as
    they were; the simulator's status word stays 0"""
    prm = load_json("params_%s.json" % name)
    d = hx(prm["delta"])
    rng = P.SplitMix64(199 + prm["k"])
    pool = [P.random_form(d, rng, 12, 10) for _ in range(20)] if name == "tiny_k8" else [P.random_form(d, rng) for _ in range(20)]
    image, co = CASE_B[0], CASE_B[6]
    pixels = int(np.prod(image))
    table = [pool[rng.below(len(pool))] for _ in range(pixels * 2 * TW)]
    one = P.identity(d)
    ent0, off_cur, off_next, map_next = level0_case()
    n_next = int(off_next[-1])
    cols = CG.column_im2col(CASE_B)
    half = ((-d).bit_length() + 1) // 2
    ad = S.to_limbs(-d, 80)
    trec = np.concatenate([S.form_record(*t3(x)) for x in table])
    orec = S.form_record(*t3(one))
    total = n_next * ROWS * 2
    assert total == 140
    dst = np.full((total + 3) * REC, 0xA5A5A5A5, dtype=np.uint32)
    sh = u32(CG.shape14(CASE_B))
    for wg in range((total + 31) // 32):
        assert sim.convg_sim_level0(S.P(sh), C.c_uint32(wg), S.P(trec), S.P(orec), S.P(ent0), S.P(off_cur), S.P(off_next), S.P(map_next),
                                    C.c_uint32(n_next), C.c_uint32(ROW0), C.c_uint32(ROWS), C.c_uint32(TW), S.P(dst), half, S.P(ad)) == 0
    assert sim.sim_status() == 0
    assert (dst[total * REC:] == 0xA5A5A5A5).all()

    seen, groups_read = set(), set()

    def leaf(e, i, h, col):
        w = int(ent0[e])
        j, neg, idx = w >> 8, (w >> 7) & 1, w & 0x7F
        px = int(cols[ROW0 + i, j, col])
        f = one if px < 0 else table[(px * 2 + h) * TW + idx]
        seen.add(("pad" if px < 0 else "real", "neg" if neg else "pos", "idx>0" if idx else "idx0"))
        if px >= 0:
            groups_read.add((col // 3, (px % image[3]) // 2))
        return (P.inverse(f) if neg else f), px < 0

    kinds = {}
    for u in range(n_next):
        s = int(map_next[u])
        q = u - int(off_next[s])
        base, cnt = int(off_cur[s]), int(off_cur[s + 1] - off_cur[s])
        for i in range(ROWS):
            for h in range(2):
                a, pa = leaf(base + 2 * q, i, h, s % co)
                if 2 * q + 1 < cnt:
                    b, pb = leaf(base + 2 * q + 1, i, h, s % co)
                    want = P.compose(a, b)
                    kinds[(pa, pb)] = kinds.get((pa, pb), 0) + 1
                else:
                    want = a
                    kinds["copy"] = kinds.get("copy", 0) + 1
                o = ((i * n_next + u) * 2 + h) * REC
                assert S.record_form(dst[o:o + REC]) == t3(want), (u, i, h, s)
    # the situations the docstring names all occurred
    assert all(kinds.get(k, 0) > 0 for k in [(True, False), (False, True), (True, True), (False, False), "copy"]), kinds
    assert {("pad", "neg", "idx>0"), ("real", "neg", "idx>0"), ("real", "pos", "idx>0")} <= seen
    assert groups_read == {(0, 0), (1, 1)}                                  # both groups were read, each from its own channel block
    assert int(map_next.max()) >= co                                        # sgm >= Co
    items = [(int(map_next[g // (2 * ROWS)]), g // (2 * ROWS)) for g in range(total)]
    paired = [2 * (u - int(off_next[s])) + 1 < COUNTS[s] for s, u in items]
    assert any(paired[96:128]) and not all(paired[96:128]) and not any(paired[128:])          # a mixed workgroup, and one of copies


# ---- the workspace plan ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [2, 4, 8])
@pytest.mark.parametrize("name", sorted(CG.CASES))
def test_workspace_plan_of_the_grouped_direct_route(lib, name, w):
    """"conv2d_grouped": the table region of "conv2d" (the image's records, whatever the groups), the other regions those of
    "scal_matmul_tree" at m = kh kw C / G"""
    from cofhe_amd import engine
    case = CG.CASES[name]
    image, kernel, stride, pad, dilation, G, co = case
    bits = 16
    n, m, p, ho, wo = CG.sizes(case)
    regs, total = engine.workspace_plan("conv2d_grouped", *CG.shape14(case), bits, w)
    pixels = int(np.prod(image))
    tw = 1 << (w - 2)
    assert regs[0] == ("table", 0, pixels * 2 * tw * REC_BYTES if w > 2 else 0)
    tregs, _ = engine.workspace_plan("scal_matmul_tree", n, m, p, bits, w)
    assert [(nm, nbytes) for nm, _, nbytes in regs[1:]] == [(nm, nbytes) for nm, _, nbytes in tregs[1:]]
    end = 0
    for nm, off, nbytes in regs:
        assert off % 256 == 0 and off >= end, nm
        end = off + nbytes
    assert end == total
    if dilation == (1, 1):
        # the same table as the ungrouped plan over the same image; its digits are G times as many
        cregs, _ = engine.workspace_plan("conv2d", *CC.shape11(image, kernel, co, stride, pad), bits, w)
        assert cregs[0] == regs[0]
        digits, cdigits = dict((nm, b) for nm, _, b in regs)["digits"], dict((nm, b) for nm, _, b in cregs)["digits"]
        assert cdigits == G * digits


@pytest.mark.parametrize("w", [2, 5])
def test_grouped_plan_without_groups_is_the_conv2d_plan(lib, w):
    from cofhe_amd import engine
    for image, kernel, stride, pad in CC.GEOMETRIES:
        a = engine.workspace_plan("conv2d_grouped", *CC.shape11(image, kernel, 5, stride, pad), 1, 1, 1, 16, w)
        assert a == engine.workspace_plan("conv2d", *CC.shape11(image, kernel, 5, stride, pad), 16, w)


def test_grouped_plan_refuses_what_the_entry_point_refuses(lib):
    from cofhe_amd import CofheHipError, engine
    for why, (image, kernel, co, stride, pad, dilation, G) in REFUSALS.items():
        with pytest.raises(CofheHipError):
            engine.workspace_plan("conv2d_grouped", *image, *kernel, co, *stride, *pad, *dilation, G, 16, 4)
    for w in (1, 9):
        with pytest.raises(CofheHipError):
            engine.workspace_plan("conv2d_grouped", *CG.shape14(CG.CASES["A"]), 16, w)
    with pytest.raises(CofheHipError):
        engine.workspace_plan("conv2d_grouped", *CG.shape14(CG.CASES["A"]), 16)          # the argument count of "conv2d" + 2
