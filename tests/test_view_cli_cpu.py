"""CPU: the host harness lists the mode that rearranges resident tensors, with its synopsis."""
import os
import subprocess

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def exe():
    import __graft_entry__ as g
    g.build()
    path = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    assert os.path.exists(path)
    return path


def test_local_bench_lists_rearrange(exe):
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == ""
    lines = [ln.strip() for ln in r.stderr.splitlines()]
    assert "rearrange [B=1 H=5 W=4 C=2 kh=3 kw=2 [sh=2 sw=1 ph=1 pw=1 dh=1 dw=1]]" in lines
