"""GPU: rearranging resident tensors through the C++ host layer (local_bench rearrange): every operation of
HIPCryptoSystem on the result of an addition, the column split of a triplet block through the device route of upload, and
max pooling with padding, decrypted and compared with host loops -- with no record download before the first decryption."""
import os
import subprocess

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
OPERATIONS = ("permute", "slice", "pad", "broadcast", "concat", "window_taps", "gather", "column_split_0", "column_split_1",
              "column_split_2", "max_pool2d_padded", "routes_agree")


@pytest.mark.parametrize("args", [(), ("2", "4", "4", "3", "2", "2", "2", "2", "0", "0", "1", "1")], ids=["defaults", "no_padding"])
def test_rearrange_through_the_host_layer(tmp_path, args):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "rearrange", *args], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = r.stdout.splitlines()
    for op in OPERATIONS:
        assert op + " ok" in lines, (op, r.stdout)
    assert "FAILED" not in r.stdout, r.stdout
    assert "block_downloads=0" in lines, r.stdout
    assert any(ln.startswith("upload_ms device=") and " host=" in ln for ln in lines), r.stdout
    assert "  agree: yes" in lines
