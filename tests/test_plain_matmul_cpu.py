"""CPU: the plaintext matrix product mod 2^k of the matrix Beaver triplets -- the body of k_plain_matmul
(cofhe_amd/csrc/plain_mm.hpp) compiled for the host and run tile by tile as the kernel runs it, against Python integers;
the new entry points among the library's symbols; the host harness with its two new modes.  No kernel runs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import plain_mm_cases as PM
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(HERE, "hostsim", "libplainmmsim.so")


@pytest.fixture(scope="module")
def sim():
    src = os.path.join(HERE, "hostsim", "plain_mm_sim.cpp")
    deps = [src, os.path.join(ROOT, "cofhe_amd", "csrc", "plain_mm.hpp")]
    if not os.path.exists(_SO) or any(os.path.getmtime(d) > os.path.getmtime(_SO) for d in deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", _SO, src])
    return C.CDLL(_SO)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    return g


def run_sim(sim, a, b, n, m, p, k):
    ra, rb = PM.exp_records(a), PM.exp_records(b)
    out = np.full(n * p * 32, 0xA5A5A5A5, dtype=np.uint32)         # the kernel must write every word of every record
    rc = sim.plain_mm_sim(ra.ctypes.data_as(C.c_void_p), rb.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p),
                          C.c_uint32(n), C.c_uint32(m), C.c_uint32(p), C.c_uint32(k))
    assert rc == 0
    return out


def test_case_shapes_sit_either_side_of_the_tile(sim):
    """the shape grid is written for the tile the kernel really has"""
    assert sim.plain_mm_sim_tile() == PM.TILE
    for d in (PM.TILE - 1, PM.TILE, PM.TILE + 1):
        assert any(d in (n, p) for n, _, p in PM.SHAPES)
    assert any(m > 2 * PM.TILE and m % PM.TILE for _, m, _ in PM.SHAPES)


@pytest.mark.parametrize("k", PM.KBITS)
def test_plain_mm_body_matches_python_integers(sim, k):
    """exact, for every shape and operand family; outputs have sign word 0 and nothing at or above bit k"""
    for name, n, m, p, a, b in PM.cases(k):
        out = run_sim(sim, a, b, n, m, p, k)
        PM.check_output(out, PM.product(a, b, n, m, p, k), k)


def test_plain_mm_empty_inner_dimension_is_zero(sim):
    out = run_sim(sim, [], [], 3, 0, 2, 128)
    PM.check_output(out, [0] * 6, 128)


def test_plain_mm_refuses_k_beyond_the_tile_buffers(sim):
    z = PM.exp_records([1])
    out = np.zeros(32, dtype=np.uint32)
    args = (z.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p), C.c_uint32(1), C.c_uint32(1), C.c_uint32(1))
    assert sim.plain_mm_sim(*args, C.c_uint32(0)) == -1
    assert sim.plain_mm_sim(*args, C.c_uint32(641)) == -1
    assert sim.plain_mm_sim(*args, C.c_uint32(640)) == 0 and out[0] == 1


def test_new_entry_points_are_exported(built):
    """fails without the feature: the three symbols of the plaintext-left product and the plaintext matrix product"""
    from cofhe_amd import lib_path
    syms = subprocess.check_output(["nm", "-D", "--defined-only", lib_path()], text=True)
    for name in ("cofhe_hip_matmul_plain_ct_records", "cofhe_hip_matmul_plain_plain_records", "cofhe_hip_matmul_plain_ct_tensors_bytes"):
        assert (" T " + name + "\n") in syms, name
    from cofhe_amd import Engine
    for name in ("matmul_plain_ct_records", "matmul_plain_plain_records", "matmul_plain_ct_tensors"):
        assert callable(getattr(Engine, name))


def test_local_bench_lists_the_new_modes(built):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1
    for mode in ("plain_ct_matmul", "ciphertext_matmul_matrix"):
        assert mode in r.stderr
