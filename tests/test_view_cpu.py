"""CPU: the index arithmetic of the affine views (cofhe_amd/csrc/view.hpp compiled with g++, tests/hostsim/view_sim.cpp) against
the Python reference of tests/view_cases.py, and the host-only entries of the C ABI (the validator and the descriptor builders)
against numpy on index arrays.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import view_cases as VC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libviewsim.so")
EINVAL = -1


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "view_sim.cpp")
    deps = [src, os.path.join(ROOT, "cofhe_amd", "csrc", "view.hpp"), os.path.join(ROOT, "include", "cofhe_hip.h")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def E():
    import __graft_entry__ as g
    g.build()
    from cofhe_amd import engine
    engine.load_library()
    return engine


def to_c(E, v):
    """a view_cases.View as the C descriptor"""
    assert E.View is type(VC.to_c(v))
    return VC.to_c(v)


def from_c(c):
    return VC.View([int(c.out_extent[d]) for d in range(c.out_ndim)], [int(c.src_extent[a]) for a in range(c.src_ndim)],
                   [int(c.start[a]) for a in range(c.src_ndim)], [[int(c.map[a][d]) for d in range(c.out_ndim)] for a in range(c.src_ndim)],
                   [int(c.dst_extent[d]) for d in range(c.out_ndim)], [int(c.dst_start[d]) for d in range(c.out_ndim)])


def through(view, index_array):
    """the view applied to a numpy array of distinct indices, -1 as the fill: an array of the view's destination shape"""
    dst = VC.apply(view, [int(x) for x in index_array.reshape(-1)], -1, [-7] * VC.count(view.dst_extent))
    return np.array(dst, dtype=np.int64).reshape(view.dst_extent)


def test_the_reference_by_hand():
    """a 2 x 3 transpose and a pad by one, the expected lists written out"""
    assert VC.apply(VC.permute([2, 3], [1, 0]), ["a", "b", "c", "d", "e", "f"], "-", [None] * 6) == ["a", "d", "b", "e", "c", "f"]
    assert VC.apply(VC.pad([2], [1], [1]), ["a", "b"], "-", [None] * 4) == ["-", "a", "b", "-"]
    assert VC.apply(VC.pad([1, 2], [1, 0], [0, 1]), ["a", "b"], "-", [None] * 6) == ["-", "-", "-", "a", "b", "-"]
    # a box inside a larger destination leaves the rest alone
    assert VC.apply(VC.into(VC.identity([2]), [4], [1]), ["a", "b"], "-", ["w", "x", "y", "z"]) == ["w", "a", "b", "z"]
    assert VC.indices(VC.slice_([7], [5], [0], [-2])) == [(5, 0), (3, 1), (1, 2)]
    assert VC.gather(["a", "b"], [1, VC.GATHER_KEEP, VC.GATHER_FILL, 2, 0], "-", ["v", "w", "x", "y", "z"]) == (["b", "w", "-", "-", "a"], True)


def test_the_descriptor_is_the_same_struct_everywhere(sim, E):
    assert sim.view_sim_descriptor_bytes() == C.sizeof(E.View) == 8 + 8 * (16 + 8 + 16) + 4 * 64


@pytest.mark.parametrize("name,views", VC.CASES, ids=VC.CASE_IDS)
def test_view_source_and_view_dest_agree_with_the_reference(sim, E, name, views):
    for v in views:
        want = VC.indices(v)
        n = len(want)
        assert n == VC.count(v.out_extent)
        src = np.full(max(n, 1), -99, dtype=np.int64)
        dst = np.full(max(n, 1), 2 ** 63, dtype=np.uint64)
        c = to_c(E, v)
        sim.view_sim_indices(C.byref(c), C.c_uint64(n), src.ctypes.data_as(C.c_void_p), dst.ctypes.data_as(C.c_void_p))
        assert [(int(s), int(d)) for s, d in zip(src[:n], dst[:n])] == want
        # the validator of the header and the library's are one function: the same counts from both
        counts = (VC.count(v.src_extent), n, VC.count(v.dst_extent), VC.needs_fill(v))
        assert E.view_check(c) == counts
        ns, nb, nd, nf = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_int()
        assert sim.view_sim_check(C.byref(c), C.byref(ns), C.byref(nb), C.byref(nd), C.byref(nf)) == 0
        assert (ns.value, nb.value, nd.value, bool(nf.value)) == counts


def test_the_case_list_covers_fill_and_no_fill():
    flags = {name: [VC.needs_fill(v) for v in views] for name, views in VC.CASES}
    assert flags["pad"] == [True] and flags["window_taps"] == [True] and flags["all_fill"] == [True]
    assert flags["transpose"] == [False] and flags["dst_box"] == [False, False] and flags["empty"] == [False]
    assert all(s < 0 for s, _ in VC.indices(dict(VC.CASES)["all_fill"][0]))
    # window taps: some taps lie in the padding, on both image axes
    taps = VC.indices(dict(VC.CASES)["window_taps"][0])
    assert 0 < sum(s < 0 for s, _ in taps) < len(taps)


def test_the_builders_agree_with_numpy(E):
    rng = np.random.default_rng(5)
    for shape, perm in (([3, 5], [1, 0]), ([2, 3, 4, 5], [3, 1, 0, 2]), ([4], [0]), ([2, 1, 3], [2, 0, 1])):
        x = np.arange(int(np.prod(shape))).reshape(shape)
        c = E.view_permute(shape, perm)
        assert np.array_equal(through(from_c(c), x), np.transpose(x, perm))
        assert from_c(c).__dict__ == VC.permute(shape, perm).__dict__
    x = np.arange(60).reshape(3, 4, 5)
    for start, stop, step in (([0, 0, 0], [3, 4, 5], [1, 1, 1]), ([1, 0, 2], [3, 4, 5], [1, 2, 3]), ([2, 3, 4], [0, -1, 1], [-1, -2, -3]),
                              ([0, 1, 0], [3, 4, 5], [1, 2, 1]), ([1, 2, 3], [1, 4, 5], [1, 1, 1]), ([2, 3, 4], [-1, -1, -1], [-1, -1, -1])):
        c = E.view_slice([3, 4, 5], start, stop, step)
        sl = tuple(slice(a, None if (s < 0 and b == -1) else b, s) for a, b, s in zip(start, stop, step))
        assert np.array_equal(through(from_c(c), x), x[sl]), (start, stop, step)
        assert from_c(c).__dict__ == VC.slice_([3, 4, 5], start, stop, step).__dict__
    y = np.arange(7)
    assert np.array_equal(through(from_c(E.view_slice([7], [1], [6], [2])), y), y[1:6:2])
    assert np.array_equal(through(from_c(E.view_slice([7], [5], [0], [-2])), y), y[5:0:-2])
    for axis in (0, 1, 2):                                                # a flip is a slice with step -1 down to element 0
        shape = [3, 4, 5]
        c = E.view_slice(shape, [shape[a] - 1 if a == axis else 0 for a in range(3)], [-1 if a == axis else shape[a] for a in range(3)],
                         [-1 if a == axis else 1 for a in range(3)])
        assert np.array_equal(through(from_c(c), x), np.flip(x, axis))
        assert from_c(c).__dict__ == VC.flip(shape, axis).__dict__
    for shape, lo, hi in (([3, 4], [1, 2], [1, 1]), ([3, 4], [0, 0], [0, 0]), ([5], [0], [3])):
        x2 = np.arange(int(np.prod(shape))).reshape(shape)
        c = E.view_pad(shape, lo, hi)
        assert np.array_equal(through(from_c(c), x2), np.pad(x2, list(zip(lo, hi)), constant_values=-1))
    for shape, out in (([3], [4, 3]), ([2, 1, 3], [2, 5, 3]), ([1], [6]), ([2, 3], [2, 3]), ([], [2, 2])):
        x2 = np.arange(int(np.prod(shape))).reshape(shape)
        c = E.view_broadcast(shape, out)
        assert np.array_equal(through(from_c(c), x2), np.broadcast_to(x2, out))
    from numpy.lib.stride_tricks import sliding_window_view
    for (B, H, W, Ch), (kh, kw), (sh, sw), (ph, pw), (dh, dw) in (((1, 5, 4, 2), (3, 2), (2, 1), (1, 1), (2, 1)), ((2, 4, 4, 3), (2, 2), (2, 2), (0, 0), (1, 1)),
                                                                    ((1, 6, 7, 1), (3, 3), (1, 2), (2, 1), (1, 2)), ((2, 3, 3, 2), (1, 1), (1, 1), (0, 0), (1, 1))):
        x4 = np.arange(B * H * W * Ch).reshape(B, H, W, Ch)
        c = E.view_window_taps((B, H, W, Ch), (kh, kw), (sh, sw), (ph, pw), (dh, dw))
        padded = np.pad(x4, ((0, 0), (ph, ph), (pw, pw), (0, 0)), constant_values=-1)
        win = sliding_window_view(padded, ((kh - 1) * dh + 1, (kw - 1) * dw + 1), axis=(1, 2))       # [B, Ho', Wo', C, keh, kew]
        win = win[:, ::sh, ::sw, :, ::dh, ::dw]                                                       # [B, Ho, Wo, C, kh, kw]
        assert np.array_equal(through(from_c(c), x4), np.transpose(win, (4, 5, 0, 1, 2, 3)))
        assert from_c(c).__dict__ == VC.window_taps(B, H, W, Ch, kh, kw, sh, sw, ph, pw, dh, dw).__dict__
        assert tuple(c.out_shape[3:5]) == E.conv2d_out_shape((B, H, W, Ch), (kh, kw, 1, Ch), (sh, sw), (ph, pw), (dh, dw), Ch)
    # concatenation along axis 1: two boxes of one destination
    a, b = np.arange(4).reshape(2, 2), 10 + np.arange(6).reshape(2, 3)
    va, vb = E.view_into(E.view_permute([2, 2], [0, 1]), [2, 5], [0, 0]), E.view_into(E.view_permute([2, 3], [0, 1]), [2, 5], [0, 2])
    dst = [-7] * 10
    VC.apply(from_c(va), [int(v) for v in a.reshape(-1)], -1, dst)
    VC.apply(from_c(vb), [int(v) for v in b.reshape(-1)], -1, dst)
    assert np.array_equal(np.array(dst).reshape(2, 5), np.concatenate([a, b], axis=1))
    del rng


def test_the_builders_refuse(E):
    for call in (lambda: E.view_permute([2, 3], [0, 0]), lambda: E.view_permute([2, 3], [0, 2]), lambda: E.view_permute([2] * 9, list(range(9))),
                 lambda: E.view_slice([7], [0], [7], [0]), lambda: E.view_slice([7], [0], [8], [1]), lambda: E.view_slice([7], [7], [0], [-1]),
                 lambda: E.view_slice([7], [-1], [3], [1]), lambda: E.view_slice([7], [3], [-2], [-1]),
                 lambda: E.view_broadcast([2], [3]), lambda: E.view_broadcast([2, 2], [2]), lambda: E.view_pad([2] * 9, [0] * 9, [0] * 9),
                 lambda: E.view_window_taps((1, 4, 4, 1), (2, 2), (0, 1)), lambda: E.view_window_taps((1, 4, 4, 1), (2, 2), (1, 1), (2, 0)),
                 lambda: E.view_window_taps((1, 2, 2, 1), (3, 3)),
                 lambda: E.view_into(E.view_permute([2, 2], [0, 1]), [2, 3], [0, 2]), lambda: E.view_into(E.view_permute([2, 2], [0, 1]), [1, 5], [0, 0])):
        with pytest.raises(E.CofheHipError) as err:
            call()
        assert err.value.code == EINVAL


def test_needs_fill_is_exact_at_the_edges(E):
    assert E.view_check(E.view_slice([7], [2], [7], [2])) == (7, 3, 3, False)          # 2, 4, 6: ends on the last element
    v = E.view_slice([7], [2], [7], [2])
    v.out_extent[0] = v.dst_extent[0] = 4                                              # one step further: 8
    assert E.view_check(v) == (7, 4, 4, True)
    assert E.view_check(E.view_slice([7], [6], [-1], [-3])) == (7, 3, 3, False)        # 6, 3, 0: ends on the first element
    v = E.view_slice([7], [6], [-1], [-3])
    v.out_extent[0] = v.dst_extent[0] = 4                                              # -3
    assert E.view_check(v) == (7, 4, 4, True)
    assert E.view_check(E.view_pad([3, 4], [0, 0], [0, 0])) == (12, 12, 12, False)
    assert E.view_check(E.view_pad([3, 4], [0, 1], [0, 0])) == (12, 15, 15, True)
    assert E.view_check(E.view_pad([3, 4], [0, 0], [1, 0])) == (12, 16, 16, True)
    # two output axes on one source axis: 2 o_0 + o_1 reaches 2 * 2 + 1 = 5, the last element of 6
    v = E.View()
    v.out_ndim, v.src_ndim = 2, 1
    v.out_extent[0], v.out_extent[1], v.dst_extent[0], v.dst_extent[1], v.src_extent[0] = 3, 2, 3, 2, 6
    v.map[0][0], v.map[0][1] = 2, 1
    assert E.view_check(v) == (6, 6, 6, False)
    v.src_extent[0] = 5
    assert E.view_check(v) == (5, 6, 6, True)
    # a zero extent: an empty box is legal, needs nothing, whatever the map says
    v.out_extent[1] = v.dst_extent[1] = 0
    v.start[0] = -100
    assert E.view_check(v) == (5, 0, 0, False)


def test_view_check_refuses(E):
    def refused(v):
        with pytest.raises(E.CofheHipError) as err:
            E.view_check(v)
        return err.value.code == EINVAL

    v = E.view_permute([2, 2], [1, 0])
    v.out_ndim = 9
    assert refused(v)
    v = E.view_permute([2, 2], [1, 0])
    v.src_ndim = 9
    assert refused(v)
    v = E.view_permute([2, 2], [1, 0])                                                # a box that sticks out of dst_extent
    v.dst_start[1] = 1
    assert refused(v)
    v.dst_extent[1] = 3
    assert E.view_check(v) == (4, 4, 6, False)
    v.dst_start[1] = 2 ** 64 - 1                                                        # ... and whose end wraps
    assert refused(v)
    # start = 2^62, map = 2^31 - 1, extent 2^32: c reaches 2^62 + (2^31 - 1)(2^32 - 1) > 2^63 -- an overflow refusal, not a wrapped acceptance
    v = E.View()
    v.out_ndim, v.src_ndim = 1, 1
    v.out_extent[0] = v.dst_extent[0] = 2 ** 32
    v.src_extent[0] = 2 ** 40
    v.start[0] = 2 ** 62
    v.map[0][0] = 2 ** 31 - 1
    assert 2 ** 62 + (2 ** 31 - 1) * (2 ** 32 - 1) > 2 ** 63 - 1
    assert refused(v)
    from cofhe_amd import load_library
    assert b"64 bits" in load_library().cofhe_hip_last_error()
    v.map[0][0] = 2 ** 30                                                               # 2^62 + 2^30 (2^32 - 1) < 2^63: in range, outside the source
    assert E.view_check(v) == (2 ** 40, 2 ** 32, 2 ** 32, True)
    v.start[0] = -(2 ** 63)                                                             # the low end: -2^63 - 2^31 (2^32 - 1)
    v.map[0][0] = -(2 ** 31)
    assert refused(v)
