"""Valid ciphertext tensors as torch CUDA tensors, made by the product path (the helper the GPU tests and the tools under
tools/ share; bench.py itself keeps to the library's own allocator and has its own copy on DBuf), and the helpers the GPU
test modules share: one engine per discriminant, random tensors, plaintext-matrix bytes and the status-word check."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
from bench import exp_records, form_record, hx  # noqa: E402,F401
import pyref as P  # noqa: E402

_engines = {}


def _pt_bytes(shape, vals):
    import struct
    offs, blobs, last = [], [], 0
    for v in vals:
        offs.append(last | ((1 << 63) if v <= 0 else 0))
        w = max(abs(v).bit_length(), 1) // 8 + 1
        blobs.append(abs(v).to_bytes(w, "little"))
        last += w
    out = struct.pack("<I", len(shape)) + b"".join(struct.pack("<I", d) for d in shape)
    return out + b"".join(struct.pack("<Q", o) for o in offs) + b"".join(blobs)


@pytest.fixture(autouse=True)
def _device_status_stays_clear():
    """after EVERY GPU test: no kernel of any context the test used hit a safety cap (lane.hpp: CF_ST_*).  The status
    word is what caught round 2's wrong-discriminant bug; a parity test that passes with a cap bit set is not a pass."""
    yield
    for delta, E in list(_engines.items()):
        assert E.device_status(clear=True) == 0, "device status word set on the context of |Delta| = %d bits" % (-delta).bit_length()


def engine(delta):
    # the PyTorch wheel bundles its own HIP runtime: when torch shares the process (the resident
    # tensor tests below) it has to initialise the GPU before libcofhe_hip.so does
    import torch
    torch.cuda.init()
    from cofhe_amd import Engine
    if delta not in _engines:
        _engines[delta] = Engine(delta)
    return _engines[delta]


def _random_tensor(d, n, seed, nbase=24):
    rng = P.SplitMix64(seed)
    base = [P.random_form(d, rng) for _ in range(nbase)]
    cts = []
    for i in range(n):
        a = base[rng.below(nbase)]
        b = base[rng.below(nbase)]
        cts.append((a, b))
    return cts


def _records_of(E, cts):
    import numpy as np
    _, recs = E.bytes_to_records(P.serialize_ciphertext_tensor([len(cts)], cts))
    return recs.view(np.int32)


def encrypt_tensor_gpu(eng, torch, prm, plaintexts, r, dev):
    """c1 = h^r (shared), c2_i = f^{m_i} o pk^r (cpu_cryptosystem_tensor_ops.inl:7-15).  Returns a device int32 tensor
    of 2E records."""
    import numpy as np
    E = len(plaintexts)
    f = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    h = form_record(hx(prm["h"]["a"]), hx(prm["h"]["b"]), hx(prm["h"]["c"]))
    pk = form_record(hx(prm["pk"]["a"]), hx(prm["pk"]["b"]), hx(prm["pk"]["c"]))
    base = torch.from_numpy(np.concatenate([h, pk]).view(np.int32)).to(dev)
    ex = torch.from_numpy(exp_records([r]).view(np.int32)).to(dev)
    hp = torch.empty_like(base)
    eng.pow_records(base.data_ptr(), ex.data_ptr(), hp.data_ptr(), 1)
    torch.cuda.synchronize()
    em = torch.from_numpy(exp_records(plaintexts).view(np.int32)).to(dev)
    out = torch.empty(E * 2 * 168, dtype=torch.int32, device=dev)
    eng.encrypt_records(em.data_ptr(), hp.data_ptr(), f, out.data_ptr(), E, prm["k"])
    torch.cuda.synchronize()
    return out
