"""CPU: the command line of the host harness (cofhe_amd/host/local_bench.cpp) where it touches no device: without a mode it
prints the usage, generated from its table of modes, and with an unknown mode it says so; both exit 1."""
import os
import subprocess

import pytest

from conftest import ROOT

MODES = ("encrypt_decrypt", "ciphertext_matadd", "scal_matmul", "threshold", "ciphertext_matmul", "ciphertext_matmul_matrix",
         "plain_ct_matmul", "fresh_randomness", "affine", "beaver_direct", "conv2d", "conv2d_grouped", "sum_pool2d",
         "poly_activation", "divide", "lookup", "formats", "threads", "plaintexts")


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    path = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    assert os.path.exists(path)
    return path


def test_no_mode_prints_every_mode_and_exits_1(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1
    assert r.stdout == ""
    assert "Usage: " in r.stderr
    assert len(MODES) == 19
    words = r.stderr.replace("|", " ").replace("<", " ").replace(">", " ").split()
    for mode in MODES:
        assert mode in words, mode


def test_unknown_mode_exits_1(exe):
    r = subprocess.run([exe, "no_such_mode"], capture_output=True, text=True)
    assert r.returncode == 1
    assert r.stdout == ""
    assert "Invalid benchmark type" in r.stderr
