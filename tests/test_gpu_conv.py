"""GPU: the 2-D convolution of a ciphertext image with plaintext filters (cofhe_amd/csrc/conv.hpp, conv.hip):
cofhe_hip_conv2d_plain_ct_records against the C++/GMP oracle byte for byte -- the expected value is the oracle's scal_2d on a
patch matrix built on the host, (identity, identity) in the padding -- on both routes, proven by their profile spans, chunked,
with special weights, from unaligned pointers; its refusals; the bytes entry; a round trip through decryption with a second
layer on top; and the C++ host layer (local_bench conv2d)."""
import os
import random
import subprocess

import numpy as np
import pytest

import conv_cases as CC
from conftest import ROOT, load_json
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records, hx  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup
from test_gpu_matmul_left import exponents, random_cts, records_of

pytestmark = pytest.mark.gpu
REC = 168
EINVAL, ESHAPE = -1, -2
FILL = 0x5A5A5A5A

# image, kernel, Co, stride, pad: distinct extents everywhere, so that no pair of swapped indices can pass
GEOS = [((1, 1, 1, 1), (1, 1), 1, (1, 1), (0, 0)),
        ((2, 5, 4, 3), (3, 2), 2, (2, 1), (1, 0)),
        ((2, 5, 4, 3), (3, 2), 2, (1, 1), (2, 1))]


def weights(k, count, seed):
    """the recipe of test_gpu_matmul_left.exponents (0, 1, -1, a k-bit and a 300-bit value, short and k-bit values of both signs)
    with int8-sized values of both signs written over four of the random ones"""
    vals = exponents(k, count, seed)
    if count >= 12:
        rng = random.Random(seed + 1)
        free = [i for i, v in enumerate(vals) if v not in (0, 1, -1) and abs(v).bit_length() not in (k, 300)]
        for i, v in zip(rng.sample(free, 4), (127, -128, 77, -3)):
            vals[i] = v
    return vals


def sizes(geo):
    image, kernel, co, stride, pad = geo
    ho, wo = CC.out_extents(image, kernel, stride, pad)
    return image[0] * ho * wo, kernel[0] * kernel[1] * image[3], co, ho, wo


def want_bytes(d, geo, w, cts, zero):
    """the oracle's scal_2d on the patch matrix, reshaped to [B, Ho, Wo, Co]"""
    image, kernel, co, stride, pad = geo
    n, m, p, ho, wo = sizes(geo)
    one = (P.identity(d), P.identity(d))
    cols = CC.im2col(image, kernel, stride, pad)
    patches = [one if px < 0 else cts[px] for px in cols.reshape(-1)]
    out = O.scal_2d(d, _pt_bytes([m, p], w), P.serialize_ciphertext_tensor([n, m], patches), P.serialize_ciphertext_tensor([1], [zero]))
    return P.serialize_ciphertext_tensor([image[0], ho, wo, co], P.deserialize_ciphertext_tensor(out)[1])


_cases = {}


def case(prm_name, gi):
    """(d, k, weights, image ciphertexts, zero, expected bytes) of geometry gi on a parameter set; computed once"""
    if (prm_name, gi) not in _cases:
        prm = load_json("params_%s.json" % prm_name)
        d, k = hx(prm["delta"]), prm["k"]
        n, m, p, _, _ = sizes(GEOS[gi])
        w = weights(k, m * p, 40 + gi)
        cts, zero = random_cts(d, int(np.prod(GEOS[gi][0])), 50 + gi), random_cts(d, 1, 60 + gi)[0]
        _cases[(prm_name, gi)] = (d, k, w, cts, zero, want_bytes(d, GEOS[gi], w, cts, zero))
    return _cases[(prm_name, gi)]


def conv_device(E, torch, geo, w, cts, zero, shift=0):
    """conv2d_plain_ct_records -> the output records (host); shift: w, cts and out start that many words into their buffers"""
    image, kernel, co, stride, pad = geo
    n, m, p, ho, wo = sizes(geo)
    dw = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), exp_records(w)]))
    dc = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), host(records_of(E, torch, cts))]))
    dz = records_of(E, torch, [zero])
    out = torch.zeros(shift + n * p * 2 * REC, dtype=torch.int32, device="cuda")
    got = E.conv2d_plain_ct_records(dw.data_ptr() + 4 * shift, dc.data_ptr() + 4 * shift, dz.data_ptr(), out.data_ptr() + 4 * shift,
                                    image, (*kernel, image[3], co), stride, pad)
    torch.cuda.synchronize()
    assert got == (ho, wo)
    assert not host(out)[:shift].any()
    return host(out)[shift:]


def conv_bytes(E, torch, geo, w, cts, zero, shift=0):
    n, m, p, ho, wo = sizes(geo)
    return E.records_to_bytes(conv_device(E, torch, geo, w, cts, zero, shift), [geo[0][0], ho, wo, geo[2]])


class pinned:
    """options pinned for a block, spans recorded; .spans() = (k_conv_level0, k_gather_patches, k_tree_level) launches"""

    def __init__(self, E, **opts):
        self.E, self.opts = E, opts

    def __enter__(self):
        self.E.profile_read("k_conv_level0", clear=True)
        for name, v in self.opts.items():
            self.E.set_option(name, v)
        self.E.set_option("profile_kernels", 1)
        return self

    def spans(self):
        return tuple(self.E.profile_read(name)[1] for name in ("k_conv_level0", "k_gather_patches", "k_tree_level"))

    def __exit__(self, *exc):
        self.E.set_option("profile_kernels", 0)
        for name in self.opts:
            self.E.set_option(name, -1 if name == "matmul_tree" else 0)
        self.E.profile_read("k_conv_level0", clear=True)


@pytest.mark.parametrize("width", [2, 5])
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("gi", [0, 1, 2])
def test_conv_matches_the_oracle_on_both_routes(gi, route, width):
    """byte for byte on the three geometries, pinned onto the direct route (k_conv_level0 launched, no k_gather_patches) and onto
    the gather route (the reverse), at window widths 2 (no table: the image is read) and 5 (a table of 8 entries per pixel)"""
    import torch
    d, k, w, cts, zero, want = case("s128_k128", gi)
    E = engine(d)
    with pinned(E, conv_route=route, wnaf_width=width) as pin:
        got = conv_bytes(E, torch, GEOS[gi], w, cts, zero)
        level0, gathers, _ = pin.spans()
    assert got == want
    assert (level0 > 0, gathers > 0) == (route == 1, route == 2), (level0, gathers)
    assert E.device_status(clear=False) == 0


def test_conv_under_the_default_options():
    """nothing pinned: the launcher's own choice of route and width gives the same bytes"""
    import torch
    d, k, w, cts, zero, want = case("s128_k128", 1)
    assert conv_bytes(engine(d), torch, GEOS[1], w, cts, zero) == want
    assert engine(d).device_status(clear=False) == 0


@pytest.mark.parametrize("rows", [8, 5])
def test_conv_in_chunks(rows):
    """the 18 output positions in chunks of 8 (8, 8, 2) and of 5 (5, 5, 5, 3): one k_conv_level0 per chunk, a ragged last chunk,
    and -- 2 rows = 16 or 10 work items per tree element -- workgroups that span two and more elements; the bytes of the unchunked
    result"""
    import torch
    d, k, w, cts, zero, want = case("s128_k128", 1)
    E = engine(d)
    with pinned(E, conv_route=1, conv_chunk_rows=rows, wnaf_width=4) as pin:
        got = conv_bytes(E, torch, GEOS[1], w, cts, zero)
        level0, gathers, _ = pin.spans()
    assert got == want
    assert (level0, gathers) == (-(-18 // rows), 0)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("route", [1, 2])
def test_all_zero_weights_give_zero_everywhere(route):
    import torch
    d, k, _, cts, zero, _ = case("s128_k128", 1)
    E = engine(d)
    n, m, p, ho, wo = sizes(GEOS[1])
    with pinned(E, conv_route=route):
        got = conv_bytes(E, torch, GEOS[1], [0] * (m * p), cts, zero)
    assert got == P.serialize_ciphertext_tensor([2, ho, wo, p], [zero] * (n * p))
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("route", [1, 2])
def test_sum_pooling_equals_the_sum_of_the_windows(route):
    """a 0/1 filter: 2 x 3 windows at stride (2, 3) over a 1 x 4 x 6 x 2 image, channel by channel (w[dy,dx,ci,co] = [ci == co]),
    equals zero plus the six shifted sub-images added with add_ciphertext_records"""
    import torch
    prm = load_json("params_s128_k128.json")
    d = hx(prm["delta"])
    E = engine(d)
    image, kernel, stride = (1, 4, 6, 2), (2, 3), (2, 3)
    geo = (image, kernel, 2, stride, (0, 0))
    n, m, p, ho, wo = sizes(geo)
    cts, zero = random_cts(d, int(np.prod(image)), 71), random_cts(d, 1, 72)[0]
    w = [1 if ci == co else 0 for _ in range(kernel[0] * kernel[1]) for ci in range(2) for co in range(2)]
    with pinned(E, conv_route=route):
        got = conv_device(E, torch, geo, w, cts, zero)
    recs = host(records_of(E, torch, cts)).reshape(1, 4, 6, 2, 2 * REC)
    acc = dev(torch, np.tile(host(records_of(E, torch, [zero])), n * p))
    for dy in range(kernel[0]):
        for dx in range(kernel[1]):
            part = dev(torch, recs[:, dy::stride[0], dx::stride[1], :, :].reshape(-1))
            E.add_ciphertext_records(acc.data_ptr(), part.data_ptr(), acc.data_ptr(), n * p)
    torch.cuda.synchronize()
    assert np.array_equal(got, host(acc))
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("route", [1, 2])
def test_conv_from_pointers_that_are_only_4_byte_aligned(route):
    """filters, image and output one word into their buffers: the dword gather, and level 0 reading the image as its table"""
    import torch
    d, k, w, cts, zero, want = case("s128_k128", 1)
    E = engine(d)
    with pinned(E, conv_route=route, wnaf_width=2 if route == 1 else 0):
        assert conv_bytes(E, torch, GEOS[1], w, cts, zero, shift=1) == want
    assert E.device_status(clear=False) == 0


def test_conv_refusals_leave_the_output_alone():
    """every COFHE_HIP_EINVAL of the header with the output at its fill pattern: a stride of 0, padding that is not smaller than
    the filter, a filter larger than the padded image, m = 2^21, extents beyond the index types, an output that overlaps the
    filters, the image or zero; the empty shapes (B = 0, Co = 0) return at once"""
    import torch
    from cofhe_amd import CofheHipError
    from test_conv_cpu import REFUSALS
    d, k, w, cts, zero, _ = case("s128_k128", 1)
    E = engine(d)
    image, kernel, co, stride, pad = GEOS[1]
    n, m, p, ho, wo = sizes(GEOS[1])
    o_cts, o_zero, o_out = m * p * 32, m * p * 32 + len(cts) * 2 * REC, m * p * 32 + (len(cts) + 1) * 2 * REC
    buf = torch.cat([dev(torch, exp_records(w)), records_of(E, torch, cts), records_of(E, torch, [zero]),
                     torch.full((n * p * 2 * REC,), FILL, dtype=torch.int32, device="cuda")])
    before = buf.clone()
    base = buf.data_ptr()
    ptrs = (base, base + 4 * o_cts, base + 4 * o_zero)
    for why, (im, ker, c_o, st, pd) in REFUSALS.items():
        with pytest.raises(CofheHipError) as ei:
            E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, im, (*ker, im[3], c_o), st, pd)
        assert ei.value.code == EINVAL, why
    for out in (base + 4 * (o_cts - 1), base + 4 * (o_cts + REC), base + 4 * (o_zero + 2 * REC - 1), base + 4 * o_zero - 4 * (n * p * 2 * REC - 1)):
        with pytest.raises(CofheHipError) as ei:
            E.conv2d_plain_ct_records(*ptrs, out, image, (*kernel, image[3], co), stride, pad)
        assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, (0, 5, 4, 3), (*kernel, 3, co), stride, pad)
    E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, image, (*kernel, 3, 0), stride, pad)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, image, (*kernel, image[3], co), stride, pad)          # next to its inputs: fine
    torch.cuda.synchronize()
    assert torch.equal(buf[:o_out], before[:o_out]) and not (host(buf[o_out:]) == FILL).all()
    assert E.device_status(clear=False) == 0


def test_conv_bytes_entry():
    """conv2d_plain_ct_tensors equals the records entry and returns the 4-D tensor [B, Ho, Wo, Co]; a 2-D operand or a channel
    mismatch is COFHE_HIP_ESHAPE; a tensor holding a non-form, and a refused geometry, are COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    d, k, w, cts, zero, want = case("s128_k128", 1)
    E = engine(d)
    image, kernel, co, stride, pad = GEOS[1]
    n, m, p, ho, wo = sizes(GEOS[1])
    wshape = [*kernel, image[3], co]
    wb, cb, zb = _pt_bytes(wshape, w), P.serialize_ciphertext_tensor(list(image), cts), P.serialize_ciphertext_tensor([1], [zero])
    got = E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad)
    assert got == want
    assert list(np.frombuffer(got[:20], dtype="<u4")) == [4, image[0], ho, wo, co]
    for call in (lambda: E.conv2d_plain_ct_tensors(_pt_bytes([m, p], w), cb, zb, stride, pad),
                 lambda: E.conv2d_plain_ct_tensors(wb, P.serialize_ciphertext_tensor([image[0] * image[1], image[2] * image[3]], cts), zb, stride, pad),
                 lambda: E.conv2d_plain_ct_tensors(_pt_bytes([kernel[0], kernel[1], co, image[3]], w), cb, zb, stride, pad),
                 lambda: E.conv2d_plain_ct_tensors(wb, P.serialize_ciphertext_tensor([image[0], image[1], image[3], image[2]], cts), zb, stride, pad)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == ESHAPE
    f = cts[7][1]
    bad = list(cts)
    bad[7] = (cts[7][0], P.Form(f.a, f.b, f.c + 1))            # b^2 - 4 a c is no longer the discriminant
    for call in (lambda: E.conv2d_plain_ct_tensors(wb, P.serialize_ciphertext_tensor(list(image), bad), zb, stride, pad),
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, P.serialize_ciphertext_tensor([1], [bad[7]]), stride, pad),
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, (0, 1), pad),
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, (3, 0))):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    assert E.device_status(clear=False) == 0


def int_conv(x, image, w, filters, stride, pad, k):
    """the integer convolution mod 2^k, channels last, on flat lists"""
    kh, kw, C, co = filters
    ho, wo = CC.out_extents(image, (kh, kw), stride, pad)
    cols = CC.im2col(image, (kh, kw), stride, pad)
    out = []
    for row in range(image[0] * ho * wo):
        for c in range(co):
            out.append(sum(x[px] * w[j * co + c] for j, px in enumerate(cols[row]) if px >= 0) % (1 << k))
    return out, (image[0], ho, wo, co)


def test_conv_decrypts_to_the_integer_convolution_and_chains(params128):
    """k = 128: a freshly encrypted 1 x 4 x 3 x 2 image under 2 x 2 x 2 x 3 filters (padding (1, 0), small weights of both signs)
    decrypts to the integer convolution mod 2^k; the [B, Ho, Wo, Co] output goes into a second convolution (3 x 1 filters,
    stride (2, 1)) as it is, and that decrypts to the convolution of the convolution"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(808)
    enc = lambda vals: fresh(E, torch, recs, vals, [rng.randrange(bound) for _ in vals], k)  # noqa: E731
    image, f1, s1, p1 = (1, 4, 3, 2), (2, 2, 2, 3), (1, 1), (1, 0)
    x = [rng.getrandbits(k) for _ in range(int(np.prod(image)))]
    w1 = [rng.randrange(-128, 128) for _ in range(int(np.prod(f1)))]
    y, im2 = int_conv(x, image, w1, f1, s1, p1, k)
    cx, zero = enc(x), enc([0])
    cy = torch.zeros(len(y) * 2 * REC, dtype=torch.int32, device="cuda")
    assert E.conv2d_plain_ct_records(dev(torch, exp_records(w1)).data_ptr(), cx.data_ptr(), zero.data_ptr(), cy.data_ptr(), image, f1, s1, p1) == im2[1:3]
    torch.cuda.synchronize()
    assert im2 == (1, 5, 2, 3) and decrypt(E, torch, prm, cy, len(y), k) == y
    f2, s2, p2 = (3, 1, 3, 2), (2, 1), (0, 0)
    w2 = [rng.randrange(-128, 128) for _ in range(int(np.prod(f2)))]
    z, im3 = int_conv(y, im2, w2, f2, s2, p2, k)
    cz = torch.zeros(len(z) * 2 * REC, dtype=torch.int32, device="cuda")
    E.conv2d_plain_ct_records(dev(torch, exp_records(w2)).data_ptr(), cy.data_ptr(), zero.data_ptr(), cz.data_ptr(), im2, f2, s2, p2)
    torch.cuda.synchronize()
    assert im3 == (1, 2, 2, 2) and decrypt(E, torch, prm, cz, len(z), k) == z
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("name", ["s128_k128", "s128_k256", "tiny_k8"])
def test_conv_on_every_parameter_set(name):
    """the second geometry on the direct route, tiny_k8, k = 128 and k = 256"""
    import torch
    d, k, w, cts, zero, want = case(name, 1)
    E = engine(d)
    with pinned(E, conv_route=1) as pin:
        got = conv_bytes(E, torch, GEOS[1], w, cts, zero)
        assert pin.spans()[0] > 0
    assert got == want
    assert E.device_status(clear=False) == 0


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")


def test_local_bench_conv2d(tmp_path):
    """HIPCryptoSystem::conv2d_plaintext_ciphertext_tensors on a 1 x 6 x 6 x 2 image with 3 x 3 x 2 x 2 filters: the tensor
    decrypts to the integer convolution mod 2^k"""
    r = subprocess.run([EXE, "conv2d", "1", "6", "6", "2", "3", "3", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "decrypts to the convolution: yes" in r.stdout, r.stdout
