"""GPU: the convolution with ciphertext filters and its Beaver triplet (cofhe_amd/csrc/conv_ct.hip, plain_conv.hpp):
cofhe_hip_conv2d_plain_plain_records against Python integers on the grid of the CPU tier, cofhe_hip_conv2d_ct_filters_records byte
for byte against the C++/GMP oracle -- the element-wise expectation of the plaintext-left product on a host-built patch matrix --
with its launch routes, from pointers that are only 4-byte aligned, its refusals, the bytes entry point, the identity
X * Wf = E * [Bf] + [A] * D + [C] + E * D through the engine alone, and the C++ host layer (local_bench conv2d_ciphertext)."""
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import plain_conv_cases as PC
import plain_mm_cases as PM
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records, hx  # noqa: F401
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup
from test_gpu_matmul_left import exponents, random_cts, records_of, want_elementwise

pytestmark = pytest.mark.gpu
REC = 168
EINVAL, ESHAPE = -1, -2
FILL = 0x5A5A5A5A
EXE = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")

# (image, kernel, stride, pad, dilation, Co): one pixel; distinct extents, n = 18, m = 18; dilated, n = 15, m = 8
CT_GEOMETRIES = {
    "one": ((1, 1, 1, 1), (1, 1), (1, 1), (0, 0), (1, 1), 1),
    "distinct": ((2, 5, 4, 3), (3, 2), (2, 1), (1, 0), (1, 1), 2),
    "dilated": ((1, 5, 4, 2), (2, 2), (1, 1), (1, 0), (2, 1), 3),
}


def filters_of(geo):
    return (geo[1][0], geo[1][1], geo[0][3], geo[5])


def out_shape(geo):
    _, _, p, ho, wo = PC.sizes(geo)
    return [geo[0][0], ho, wo, p]


def want_conv(d, geo, img, cts, zero):
    """the oracle's expectation as the serialised [B, Ho, Wo, Co] tensor: want_elementwise on the numpy patch matrix of the exponents"""
    n, m, p, _, _ = PC.sizes(geo)
    flat = want_elementwise(d, PC.patch_values(geo, img), cts, zero, n, m, p)
    return P.serialize_ciphertext_tensor(out_shape(geo), P.deserialize_ciphertext_tensor(flat)[1])


@functools.lru_cache(maxsize=None)
def ct_case(gid):
    """(geometry, exponents of the image, filter ciphertexts, zero, expected bytes) of one geometry, computed once for every test"""
    prm = load_json("params_s128_k128.json")
    d, k = hx(prm["delta"]), prm["k"]
    geo = CT_GEOMETRIES[gid]
    _, m, p, _, _ = PC.sizes(geo)
    seed = 40 + len(gid)
    img, cts, zero = exponents(k, int(np.prod(geo[0])), seed), random_cts(d, m * p, seed + 1), random_cts(d, 1, seed + 2)[0]
    return geo, img, cts, zero, want_conv(d, geo, img, cts, zero)


def ct_filters_records(E, torch, geo, img, cts, zero, shift=0):
    """conv2d_ct_filters_records -> serialised [B, Ho, Wo, Co] tensor; shift: the image, the filters and the output start that many
    words into their buffers (pointers that are only 4-byte aligned)"""
    n, _, p, ho, wo = PC.sizes(geo)
    di = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), exp_records(img)]))
    dc = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), host(records_of(E, torch, cts))]))
    dz = records_of(E, torch, [zero])
    out = torch.zeros(shift + n * p * 2 * REC, dtype=torch.int32, device="cuda")
    got = E.conv2d_ct_filters_records(di.data_ptr() + 4 * shift, dc.data_ptr() + 4 * shift, dz.data_ptr(), out.data_ptr() + 4 * shift, geo[0],
                                      filters_of(geo), geo[2], geo[3], dilation=geo[4])
    torch.cuda.synchronize()
    assert got == (ho, wo)
    assert not host(out)[:shift].any()
    return E.records_to_bytes(host(out)[shift:], out_shape(geo))


# ---- the plaintext convolution mod 2^k ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", PC.KBITS)
def test_plain_plain_conv_matches_python_integers(params128, k):
    """k_plain_conv2d on the grid of the CPU tier (tests/plain_conv_cases.py): the limb counts of plain_mm_cases; n and Co either
    side of the 16 x 16 tile, an inner dimension of 33, distinct extents with a stride per axis, a tile row of padding, dilation,
    a window wholly in the padding; 0, +-1, 2^k - 1, magnitudes of 2^k and above, mixed signs.  Exact; every word written; sign
    word 0; nothing at or above bit k"""
    import torch
    E = engine(hx(params128["delta"]))
    for name, gid, img, w in PC.cases(k):
        geo = PC.GEOMETRIES[gid]
        n, _, p, ho, wo = PC.sizes(geo)
        di, dw = dev(torch, PM.exp_records(img)), dev(torch, PM.exp_records(w))
        out = torch.full((n * p * 32,), FILL, dtype=torch.int32, device="cuda")
        assert E.conv2d_plain_plain_records(di.data_ptr(), dw.data_ptr(), out.data_ptr(), geo[0], filters_of(geo), k, geo[2], geo[3],
                                            dilation=geo[4]) == (ho, wo)
        torch.cuda.synchronize()
        PM.check_output(host(out), PC.expected(geo, img, w, k), k)
        assert not (host(out) == FILL).any(), (name, gid)
    assert E.device_status(clear=False) == 0


# ---- the plaintext image under ciphertext filters ---------------------------------------------------------------------------------

@pytest.mark.parametrize("gid", sorted(CT_GEOMETRIES))
@pytest.mark.parametrize("tree", [0, 1])
def test_ct_filters_match_the_oracle_on_both_routes(params128, gid, tree):
    """byte for byte against the element-wise expectation on the host-built patch matrix, exponents 0, 1, -1, a k-bit value, a
    300-bit value, with the product underneath pinned onto the chains and onto the product tree: one launch of
    k_gather_patch_exponents either way, levels of k_tree_level only on the tree"""
    import torch
    d = hx(params128["delta"])
    E = engine(d)
    geo, img, cts, zero, want = ct_case(gid)
    m = PC.sizes(geo)[1]
    E.profile_read("k_tree_level", clear=True)
    E.set_option("matmul_tree", tree)
    E.set_option("profile_kernels", 1)
    try:
        got = ct_filters_records(E, torch, geo, img, cts, zero)
        gathers, levels = E.profile_read("k_gather_patch_exponents")[1], E.profile_read("k_tree_level")[1]
        patches = E.profile_read("k_gather_patches")[1]
    finally:
        E.set_option("profile_kernels", 0)
        E.set_option("matmul_tree", -1)
        E.profile_read("k_tree_level", clear=True)
    assert got == want
    assert gathers == 1 and patches == 0
    if m >= 8:                                                     # one pixel has nothing to pair up
        assert (levels > 0) == (tree == 1)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("gid", ["distinct", "dilated"])
def test_ct_filters_from_pointers_offset_by_one_word(params128, gid):
    """the dword paths of the gather and of the transposes"""
    import torch
    E = engine(hx(params128["delta"]))
    geo, img, cts, zero, want = ct_case(gid)
    assert ct_filters_records(E, torch, geo, img, cts, zero, shift=1) == want
    assert E.device_status(clear=False) == 0


def test_refusals_leave_the_output_untouched(params128):
    """an output that overlaps the image, the filters or zero, and groups = 2: COFHE_HIP_EINVAL from both records entries and not a
    word written"""
    import ctypes as C
    import torch
    from cofhe_amd import CofheHipError
    from cofhe_amd.engine import _ConvGeometry
    d, k = hx(params128["delta"]), params128["k"]
    E = engine(d)
    geo = ((1, 4, 3, 2), (2, 2), (1, 1), (1, 0), (1, 1), 2)
    n, m, p, _, _ = PC.sizes(geo)
    n_img = int(np.prod(geo[0]))
    fill = lambda words: torch.full((words,), FILL, dtype=torch.int32, device="cuda")                 # noqa: E731
    # ciphertext filters: [filters | image exponents | zero | out]
    buf = torch.cat([records_of(E, torch, random_cts(d, m * p, 61)), dev(torch, exp_records(exponents(k, n_img, 62))),
                     records_of(E, torch, random_cts(d, 1, 63)), fill(n * p * 2 * REC)])
    base = buf.data_ptr()
    o_img, o_z = 4 * m * p * 2 * REC, 4 * (m * p * 2 * REC + n_img * 32)
    o_out = o_z + 4 * 2 * REC
    before = buf.clone()
    call = lambda out: E.conv2d_ct_filters_records(base + o_img, base, base + o_z, out, geo[0], filters_of(geo), geo[2], geo[3])  # noqa: E731
    for out in (base + 4 * REC, base + o_img - 4, base + o_img + 4, base + o_z - 4, base + o_z):
        with pytest.raises(CofheHipError) as ei:
            call(out)
        assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    grouped = _ConvGeometry(*PC.shape14(geo, groups=2))
    assert E.L.cofhe_hip_conv2d_ct_filters_records(E.ctx, C.c_void_p(base + o_img), C.c_void_p(base), C.c_void_p(base + o_z),
                                                   C.c_void_p(base + o_out), C.byref(grouped), None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # the plaintext convolution: [image | filters | out]
    pbuf = torch.cat([dev(torch, exp_records(exponents(k, n_img, 64))), dev(torch, exp_records(exponents(k, m * p, 65))), fill(n * p * 32)])
    pbase = pbuf.data_ptr()
    o_w, o_pout = 4 * n_img * 32, 4 * (n_img + m * p) * 32
    pbefore = pbuf.clone()
    for out in (pbase + 4, pbase + o_w - 4, pbase + o_w, pbase + o_pout - 4):
        with pytest.raises(CofheHipError) as ei:
            E.conv2d_plain_plain_records(pbase, pbase + o_w, out, geo[0], filters_of(geo), k, geo[2], geo[3])
        assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    assert E.L.cofhe_hip_conv2d_plain_plain_records(E.ctx, C.c_void_p(pbase), C.c_void_p(pbase + o_w), C.c_void_p(pbase + o_pout), C.byref(grouped),
                                                    C.c_uint32(k), None) == EINVAL
    torch.cuda.synchronize()
    assert torch.equal(pbuf, pbefore)
    call(base + o_out)                                             # next to its inputs: fine
    torch.cuda.synchronize()
    assert torch.equal(buf[: o_out // 4], before[: o_out // 4]) and not (host(buf[o_out // 4:]) == FILL).all()
    assert E.device_status(clear=False) == 0


def test_ct_filters_bytes_entry(params128):
    """conv2d_ct_filters_tensors (composed in the Engine from the unpack, the records entry and the pack) equals the records
    entry's serialisation; a filter tensor of the wrong shape, or an operand that is not 4-D, is COFHE_HIP_ESHAPE; a filter or a
    zero that holds a non-form is COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    d = hx(params128["delta"])
    E = engine(d)
    geo, img, cts, zero, want = ct_case("distinct")
    ib, fb = _pt_bytes(list(geo[0]), img), P.serialize_ciphertext_tensor(list(filters_of(geo)), cts)
    zb = P.serialize_ciphertext_tensor([1], [zero])
    got = E.conv2d_ct_filters_tensors(ib, fb, zb, geo[2], geo[3], geo[4])
    assert got == ct_filters_records(E, torch, geo, img, cts, zero) == want
    kh, kw, c, co = filters_of(geo)
    for call in (lambda: E.conv2d_ct_filters_tensors(ib, P.serialize_ciphertext_tensor([kh, kw, co, c], cts), zb, geo[2], geo[3]),
                 lambda: E.conv2d_ct_filters_tensors(ib, P.serialize_ciphertext_tensor([kh * kw, c, co], cts), zb, geo[2], geo[3]),
                 lambda: E.conv2d_ct_filters_tensors(_pt_bytes([len(img)], img), fb, zb, geo[2], geo[3])):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == ESHAPE
    f = cts[5][1]
    bad = list(cts)
    bad[5] = (cts[5][0], P.Form(f.a, f.b, f.c + 1))            # b^2 - 4 a c is no longer the discriminant
    for call in (lambda: E.conv2d_ct_filters_tensors(ib, P.serialize_ciphertext_tensor(list(filters_of(geo)), bad), zb, geo[2], geo[3]),
                 lambda: E.conv2d_ct_filters_tensors(ib, fb, P.serialize_ciphertext_tensor([1], [bad[5]]), geo[2], geo[3])):
        with pytest.raises(CofheHipError, match="not a reduced form") as ei:
            call()
        assert ei.value.code == EINVAL
    assert E.device_status(clear=False) == 0


# ---- the convolution Beaver identity ------------------------------------------------------------------------------------------------

def test_beaver_conv_identity_through_the_engine(params128):
    """k = 128, image 1 x 4 x 3 x 2 under 2 x 2 x 2 x 2 filters, pad (1, 0), a convolution triplet [A], [Bf], [C = A * Bf]:
    E = Dec(X - A), D = Dec(Wf - Bf), then E * [Bf] + [A] * D + [C] + E * D decrypts to X * Wf mod 2^k -- every step an Engine call,
    all five tensors freshly encrypted"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(707)
    geo = ((1, 4, 3, 2), (2, 2), (1, 1), (1, 0), (1, 1), 2)
    image, filters, stride, pad = geo[0], filters_of(geo), geo[2], geo[3]
    n, m, p, ho, wo = PC.sizes(geo)
    n_img, n_w, n_out, M = int(np.prod(image)), m * p, n * p, 1 << k
    rand = lambda c: [rng.getrandbits(k) for _ in range(c)]                                  # noqa: E731
    enc = lambda vals: fresh(E, torch, recs, vals, [rng.randrange(bound) for _ in vals], k)  # noqa: E731
    conv = lambda a, b: PC.expected(geo, a, b, k)                                            # noqa: E731
    X, W, A, B = rand(n_img), rand(n_w), rand(n_img), rand(n_w)
    cX, cW, cA, cB, cC = enc(X), enc(W), enc(A), enc(B), enc(conv(A, B))
    zero = enc([0])
    xa, wb = torch.zeros_like(cX), torch.zeros_like(cW)
    E.sub_ciphertext_records(cX.data_ptr(), cA.data_ptr(), xa.data_ptr(), n_img)
    E.sub_ciphertext_records(cW.data_ptr(), cB.data_ptr(), wb.data_ptr(), n_w)
    Ev, Dv = decrypt(E, torch, prm, xa, n_img, k), decrypt(E, torch, prm, wb, n_w, k)
    assert Ev == [(x - a) % M for x, a in zip(X, A)] and Dv == [(w - b) % M for w, b in zip(W, B)]
    dE, dD = dev(torch, exp_records(Ev)), dev(torch, exp_records(Dv))
    eb = torch.zeros(n_out * 2 * REC, dtype=torch.int32, device="cuda")
    ad, acc = torch.zeros_like(eb), torch.zeros_like(eb)
    ed = torch.zeros(n_out * 32, dtype=torch.int32, device="cuda")
    assert E.conv2d_ct_filters_records(dE.data_ptr(), cB.data_ptr(), zero.data_ptr(), eb.data_ptr(), image, filters, stride, pad) == (ho, wo)
    assert E.conv2d_plain_ct_records(dD.data_ptr(), cA.data_ptr(), zero.data_ptr(), ad.data_ptr(), image, filters, stride, pad) == (ho, wo)
    E.add_ciphertext_records(eb.data_ptr(), ad.data_ptr(), acc.data_ptr(), n_out)
    E.add_ciphertext_records(acc.data_ptr(), cC.data_ptr(), acc.data_ptr(), n_out)
    E.conv2d_plain_plain_records(dE.data_ptr(), dD.data_ptr(), ed.data_ptr(), image, filters, k, stride, pad)
    E.add_plain_records(acc.data_ptr(), ed.data_ptr(), recs["f"], acc.data_ptr(), n_out, k, 0)
    torch.cuda.synchronize()
    PM.check_output(host(ed), conv(Ev, Dv), k)
    assert decrypt(E, torch, prm, acc, n_out, k) == conv(X, W)
    assert E.device_status(clear=False) == 0


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("threshold", [(), ("2", "3")])
def test_local_bench_conv2d_ciphertext(tmp_path, params128, threshold):
    """LocalCipherTextMultiplier::conv2d_ciphertext_tensors at the mode's defaults (1 x 5 x 4 x 2 under 3 x 2 x 2 x 2), with the secret
    key and by 2-of-3 threshold decryption: the result decrypts to the exact convolution, the flow opens 1 5 4 2 + 3 2 2 2 = 64
    values, and the E * [Bf] term it serialises equals the oracle's element-wise expectation on the operands it wrote"""
    defaults = ["1", "5", "4", "2", "3", "2", "2"]
    args = defaults + ["1", "1", "0", "0", "1", "1", *threshold] if threshold else []
    r = subprocess.run([EXE, "conv2d_ciphertext", *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    assert ("threshold 2 of 3" if threshold else "secret key") in r.stdout
    geo = ((1, 5, 4, 2), (3, 2), (1, 1), (0, 0), (1, 1), 2)
    n, m, p, _, _ = PC.sizes(geo)
    assert [int(v) for v in re.findall(r"conv flow: decrypted_elements (\d+)", r.stdout)] == [1 * 5 * 4 * 2 + 3 * 2 * 2 * 2]
    assert "2 n m p = %d " % (2 * n * m * p) in r.stdout and "n m + m p = %d " % (n * m + m * p) in r.stdout
    rd = lambda name: open(tmp_path / ("local_bench_cconv_%s.bin" % name), "rb").read()       # noqa: E731
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    E = engine(hx(params128["delta"]))                  # the format conversions are host code of any context
    shape, ex = E.bytes_to_exponents(rd("img"))
    assert shape == list(geo[0])
    img = [-v if sign else v for v, sign in PM.record_values(ex)]
    (fshape, cts), (_, zero) = P.deserialize_ciphertext_tensor(rd("filters")), P.deserialize_ciphertext_tensor(rd("zero"))
    assert fshape == list(filters_of(geo))
    assert rd("term") == want_conv(delta, geo, img, cts, zero[0])
    assert P.deserialize_ciphertext_tensor(rd("out"))[0] == out_shape(geo)
