"""CPU: what ciphertext filters add to the convolution, without a GPU -- the bodies of k_plain_conv2d and
k_gather_patch_exponents (cofhe_amd/csrc/plain_conv.hpp) compiled for the host and run as the kernels run them, against Python
integers on a numpy patch matrix; the refusals of the two records entries that need no context; the new entry points among the
library's symbols; the host harness with its new mode.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plain_conv_cases as PC
import plain_mm_cases as PM
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libplainconvsim.so")
EINVAL = -1
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "plain_conv_sim.cpp")
    deps = [src, os.path.join(HERE, "hostsim", "sim.cpp")] + [os.path.join(ROOT, "cofhe_amd", "csrc", f) for f in
                                                              ("plain_conv.hpp", "plain_mm.hpp", "conv.hpp", "form_io.hpp", "layout.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-pthread", "-DCOFHE_WG_GROUPS=32", "-o", _SO, src])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return g


def u32(vals):
    return np.array(vals, dtype=np.uint32)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def run_conv(sim, geo, img, w, k):
    n, _, p, _, _ = PC.sizes(geo)
    ri, rw, sh = PM.exp_records(img), PM.exp_records(w), u32(PC.shape14(geo))
    out = np.full(n * p * 32, FILL, dtype=np.uint32)               # the kernel must write every word of every record
    assert sim.plain_conv_sim(ptr(sh), ptr(ri), ptr(rw), ptr(out), C.c_uint32(k)) == 0
    return out


def test_geometries_sit_where_the_docstring_says(sim):
    """the grid is written for the tile the kernel really has: n and Co at 15, 16, 17, an inner dimension of two steps and one
    element, a tile row of padding, a window wholly in the padding"""
    T = PM.TILE
    assert sim.plain_conv_sim_tile() == T
    G = PC.GEOMETRIES
    assert [PC.sizes(G[g])[0] for g in ("n15", "n16", "n17")] == [T - 1, T, T + 1]
    assert [PC.sizes(G[g])[2] for g in ("n15", "n16", "n17")] == [T + 1, T, T - 1]
    assert PC.sizes(G["inner33"])[1] == 2 * T + 1
    assert PC.sizes(G["distinct"])[:3] == (18, 18, 2) and PC.sizes(G["dilated"])[:3] == (15, 8, 3)
    assert (PC.im2col(G["pad2"])[:, :T] < 0).all(axis=1).any()                       # a whole row of the first left tile
    assert (PC.im2col(G["all_padding"]) < 0).all()
    assert G["dilated"][4] == (2, 1) and G["pad2"][3][0] == 2


@pytest.mark.parametrize("k", PC.KBITS)
def test_plain_conv_body_matches_python_integers(sim, k):
    """exact, for every geometry and operand family; every word overwritten, sign word 0, nothing at or above bit k"""
    for name, gid, img, w in PC.cases(k):
        geo = PC.GEOMETRIES[gid]
        out = run_conv(sim, geo, img, w, k)
        PM.check_output(out, PC.expected(geo, img, w, k), k)
        assert not (out == FILL).any(), (name, gid)                 # (the cases are seeded: no sum holds the pattern by chance)
    n, _, p, _, _ = PC.sizes(PC.GEOMETRIES["all_padding"])
    img, w = [(1 << k) - 1] * 6, [3] * 4
    assert PM.record_values(run_conv(sim, PC.GEOMETRIES["all_padding"], img, w, k)) == [(0, 0)] * (n * p)


def test_plain_conv_sim_refuses_what_the_launcher_refuses(sim):
    geo = PC.GEOMETRIES["distinct"]
    z = PM.exp_records([1] * 120)
    out = np.zeros(18 * 2 * 32, dtype=np.uint32)
    for k, want in ((0, -1), (641, -1), (640, 0)):
        assert sim.plain_conv_sim(ptr(u32(PC.shape14(geo))), ptr(z), ptr(z), ptr(out), C.c_uint32(k)) == want
    assert sim.plain_conv_sim(ptr(u32(PC.shape14(geo, groups=3))), ptr(z), ptr(z), ptr(out), C.c_uint32(128)) == 1


@pytest.mark.parametrize("gid", sorted(PC.GEOMETRIES))
@pytest.mark.parametrize("offset", (0, 1))
def test_gather_body_is_the_transposed_im2col(sim, gid, offset):
    """S^T[j n + row] = img[conv_leaf(row, j)] word for word, zero records in the padding: 16-byte pieces from aligned pointers,
    4-byte pieces when a pointer is offset by one word"""
    geo = PC.GEOMETRIES[gid]
    n, m, _, _, _ = PC.sizes(geo)
    n_img = int(np.prod(geo[0]))
    rng = np.random.default_rng(7)
    base = np.zeros(n_img * 32 + 4, dtype=np.uint32)
    img = base[offset:offset + n_img * 32]
    img[:] = rng.integers(1, 1 << 32, size=n_img * 32, dtype=np.uint64).astype(np.uint32)      # no zero word: padding is told apart
    obase = np.full(n * m * 32 + 4, FILL, dtype=np.uint32)
    out = obase[:n * m * 32]
    assert base.ctypes.data % 16 == 0 and obase.ctypes.data % 16 == 0
    piece = sim.plain_conv_sim_gather(ptr(u32(PC.shape14(geo))), C.c_void_p(img.ctypes.data), C.c_void_p(out.ctypes.data), C.c_uint32(37))
    assert piece == (4 if offset else 16)
    idx = PC.im2col(geo).T.reshape(-1)                                                         # [m, n]
    recs = img.reshape(n_img, 32)
    want = np.where((idx >= 0)[:, None], recs[np.maximum(idx, 0)], 0).astype(np.uint32)
    assert np.array_equal(out.reshape(n * m, 32), want)
    assert (obase[n * m * 32:] == FILL).all()                                                  # and not a word beyond


def geometry(geo, groups=1, stride=None):
    from cofhe_amd.engine import _ConvGeometry
    v = PC.shape14(geo, groups)
    if stride is not None:
        v[7], v[8] = stride
    return _ConvGeometry(*v)


def test_records_entries_refuse_without_a_context(built):
    """COFHE_HIP_EINVAL before the context or a pointer is looked at: groups = 2, a zero stride, kbits 0 and 640"""
    from cofhe_amd import load_library
    lib = load_library()
    ok = PC.GEOMETRIES["distinct"]
    two = ((1, 4, 4, 2), (1, 1), (1, 1), (0, 0), (1, 1), 2)                  # C = Co = 2: groups = 2 is a legal grouped geometry
    for geo, why in ((geometry(two, groups=2), "groups"), (geometry(ok, stride=(0, 1)), "stride"), (geometry(ok, stride=(2, 0)), "stride")):
        assert lib.cofhe_hip_conv2d_plain_plain_records(None, None, None, None, C.byref(geo), C.c_uint32(128), None) == EINVAL, why
        assert lib.cofhe_hip_conv2d_ct_filters_records(None, None, None, None, None, C.byref(geo), None) == EINVAL, why
    ho, wo = C.c_uint32(), C.c_uint32()
    assert lib.cofhe_hip_conv2d_geometry_out_shape(C.byref(geometry(two, groups=2)), C.byref(ho), C.byref(wo)) == 0      # refused for its groups alone
    for k in (0, 640):
        assert lib.cofhe_hip_conv2d_plain_plain_records(None, None, None, None, C.byref(geometry(ok)), C.c_uint32(k), None) == EINVAL, k
    assert lib.cofhe_hip_conv2d_plain_plain_records(None, None, None, None, None, C.c_uint32(128), None) == EINVAL
    assert lib.cofhe_hip_conv2d_ct_filters_records(None, None, None, None, None, None, None) == EINVAL


def test_new_entry_points_are_exported(built):
    """fails without the feature: the two symbols of the convolution with ciphertext filters and the Engine methods (the one on
    serialised tensors is composed in the Engine: the library has no *_tensors_bytes entry point for it)"""
    from cofhe_amd import lib_path
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path()], text=True)
    for name in ("cofhe_hip_conv2d_plain_plain_records", "cofhe_hip_conv2d_ct_filters_records"):
        assert (" T " + name + "\n") in syms, name
    from cofhe_amd import Engine
    for name in ("conv2d_plain_plain_records", "conv2d_ct_filters_records", "conv2d_ct_filters_tensors"):
        assert callable(getattr(Engine, name))


def test_local_bench_lists_the_new_mode(built):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1
    assert "conv2d_ciphertext" in r.stderr
