"""GPU: groups, depthwise filters and dilation of the convolution, and sum pooling on top (cofhe_amd/csrc/conv.hpp, conv.hip):
cofhe_hip_conv2d_grouped_plain_ct_records against the C++/GMP oracle byte for byte -- per group, the oracle's scal_2d on that
group's patch matrix and column block, the columns interleaved -- on both routes, proven by their profile spans; against the
block-diagonal dense filter through the old entry; chunked; from unaligned pointers; its refusals; the bytes entries;
cofhe_hip_sum_pool2d_records against additions; a round trip through decryption; and the C++ host layer."""
import os
import random
import subprocess

import numpy as np
import pytest

import conv_groups_cases as CG
from conftest import ROOT, load_json
from gpu_inputs import P, _pt_bytes, engine, exp_records, hx  # noqa: F401
import oracle_lib as O
import test_gpu_conv as TC
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup
from test_gpu_matmul_left import random_cts, records_of

pytestmark = pytest.mark.gpu
REC = 168
EINVAL, ESHAPE = -1, -2
FILL = 0x5A5A5A5A
SPANS = ("k_conv_level0", "k_gather_patches", "k_expand_group_filters")


def want_bytes(d, case, w, cts, zero):
    """per group: the oracle's scal_2d on the group's patch matrix and column block; the columns interleaved to [B, Ho, Wo, Co]"""
    image, kernel, stride, pad, dilation, G, co = case
    n, m, p, ho, wo = CG.sizes(case)
    cog = co // G
    one = (P.identity(d), P.identity(d))
    cols = CG.group_im2col(case)
    zb = P.serialize_ciphertext_tensor([1], [zero])
    out = [None] * (n * co)
    for g in range(G):
        patches = [one if px < 0 else cts[px] for px in cols[g].reshape(-1)]
        wg = [w[j * co + g * cog + c] for j in range(m) for c in range(cog)]
        res = P.deserialize_ciphertext_tensor(O.scal_2d(d, _pt_bytes([m, cog], wg), P.serialize_ciphertext_tensor([n, m], patches), zb))[1]
        for row in range(n):
            for c in range(cog):
                out[row * co + g * cog + c] = res[row * cog + c]
    return P.serialize_ciphertext_tensor([image[0], ho, wo, co], out)


_cases = {}


def case_data(prm_name, name):
    """(d, k, weights, image ciphertexts, zero, expected bytes) of a case on a parameter set; computed once"""
    if (prm_name, name) not in _cases:
        prm = load_json("params_%s.json" % prm_name)
        d, k = hx(prm["delta"]), prm["k"]
        case = CG.CASES[name]
        n, m, p, _, _ = CG.sizes(case)
        seed = ord(name)
        w = TC.weights(k, m * p, 400 + seed)
        cts, zero = random_cts(d, int(np.prod(case[0])), 500 + seed), random_cts(d, 1, 600 + seed)[0]
        _cases[(prm_name, name)] = (d, k, w, cts, zero, want_bytes(d, case, w, cts, zero))
    return _cases[(prm_name, name)]


def conv_device(E, torch, case, w, cts, zero, shift=0):
    """conv2d_plain_ct_records with dilation and groups -> the output records (host); shift: w, cts and out start that many
    words into their buffers"""
    image, kernel, stride, pad, dilation, G, co = case
    n, m, p, ho, wo = CG.sizes(case)
    dw = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), exp_records(w)]))
    dc = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), host(records_of(E, torch, cts))]))
    dz = records_of(E, torch, [zero])
    out = torch.zeros(shift + n * p * 2 * REC, dtype=torch.int32, device="cuda")
    got = E.conv2d_plain_ct_records(dw.data_ptr() + 4 * shift, dc.data_ptr() + 4 * shift, dz.data_ptr(), out.data_ptr() + 4 * shift,
                                    image, CG.filters_of(case), stride, pad, dilation=dilation, groups=G)
    torch.cuda.synchronize()
    assert got == (ho, wo)
    assert not host(out)[:shift].any()
    return host(out)[shift:]


def conv_bytes(E, torch, case, w, cts, zero, shift=0):
    n, m, p, ho, wo = CG.sizes(case)
    return E.records_to_bytes(conv_device(E, torch, case, w, cts, zero, shift), [case[0][0], ho, wo, p])


class pinned(TC.pinned):
    """.spans() = (k_conv_level0, k_gather_patches, k_expand_group_filters) launches"""

    def spans(self):
        return tuple(self.E.profile_read(name)[1] for name in SPANS)


def check_route(case, route, spans):
    level0, gathers, expands = spans
    assert (level0 > 0, gathers > 0) == (route == 1, route == 2), spans
    assert (expands > 0) == (route == 2 and case[5] > 1), spans


@pytest.mark.parametrize("width", [2, 5])
@pytest.mark.parametrize("route", [1, 2])
@pytest.mark.parametrize("name", sorted(CG.CASES))
def test_grouped_conv_matches_the_oracle_on_both_routes(name, route, width):
    """A-F byte for byte, pinned onto the direct route (k_conv_level0 launched, no k_gather_patches) and onto the gather route
    (the reverse, behind k_expand_group_filters when there are groups), at window widths 2 and 5"""
    import torch
    d, k, w, cts, zero, want = case_data("s128_k128", name)
    E = engine(d)
    with pinned(E, conv_route=route, wnaf_width=width) as pin:
        got = conv_bytes(E, torch, CG.CASES[name], w, cts, zero)
        spans = pin.spans()
    assert got == want
    check_route(CG.CASES[name], route, spans)
    assert E.device_status(clear=False) == 0


def old_entry_bytes(E, torch, image, kernel, co, stride, pad, w, cts, zero):
    return TC.conv_bytes(E, torch, (image, kernel, co, stride, pad), w, cts, zero)


@pytest.mark.parametrize("name", ["B", "C"])
def test_grouped_conv_equals_the_block_diagonal_dense_filter(name):
    """the existing conv2d_plain_ct_records fed the dense [kh, kw, C, Co] filter that is zero outside the blocks: the same bytes"""
    import torch
    d, k, w, cts, zero, want = case_data("s128_k128", name)
    case = CG.CASES[name]
    image, kernel, stride, pad, dilation, G, co = case
    E = engine(d)
    assert old_entry_bytes(E, torch, image, kernel, co, stride, pad, CG.dense_filter(case, w), cts, zero) == want
    assert conv_bytes(E, torch, case, w, cts, zero) == want
    assert E.device_status(clear=False) == 0


def test_no_groups_no_dilation_through_the_new_entry_is_the_old_entry():
    """cofhe_hip_conv2d_grouped_plain_ct_records with groups = 1, dilation = (1, 1) on test_gpu_conv.GEOS[1]"""
    import ctypes as C
    import torch
    from cofhe_amd import engine as eng_mod
    d, k, w, cts, zero, want = TC.case("s128_k128", 1)
    E = engine(d)
    image, kernel, co, stride, pad = TC.GEOS[1]
    n, m, p, ho, wo = TC.sizes(TC.GEOS[1])
    geo = eng_mod._conv_geometry(image, (*kernel, image[3], co), stride, pad, (1, 1), 1)
    dw, dc, dz = dev(torch, exp_records(w)), records_of(E, torch, cts), records_of(E, torch, [zero])
    out = torch.zeros(n * p * 2 * REC, dtype=torch.int32, device="cuda")
    assert E.L.cofhe_hip_conv2d_grouped_plain_ct_records(E.ctx, C.c_void_p(dw.data_ptr()), C.c_void_p(dc.data_ptr()), C.c_void_p(dz.data_ptr()),
                                                         C.c_void_p(out.data_ptr()), C.byref(geo), None) == 0
    torch.cuda.synchronize()
    got = E.records_to_bytes(host(out), [image[0], ho, wo, co])
    assert got == want == TC.conv_bytes(E, torch, TC.GEOS[1], w, cts, zero)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("route", [1, 2])
def test_a_window_wholly_in_the_padding_gives_zero(route):
    """E: the dilated 2 x 1 filter's two taps sit two rows above and two rows below the one-row image"""
    import torch
    d, k, w, cts, zero, _ = case_data("s128_k128", "E")
    E = engine(d)
    n, m, p, ho, wo = CG.sizes(CG.CASES["E"])
    with pinned(E, conv_route=route):
        got = conv_bytes(E, torch, CG.CASES["E"], w, cts, zero)
    assert got == P.serialize_ciphertext_tensor([1, ho, wo, p], [zero] * (n * p))
    assert E.device_status(clear=False) == 0


def test_grouped_conv_in_chunks():
    """B's 9 output positions in chunks of 4 (4, 4, 1): one k_conv_level0 per chunk, the bytes of the unchunked result"""
    import torch
    d, k, w, cts, zero, want = case_data("s128_k128", "B")
    E = engine(d)
    with pinned(E, conv_route=1, conv_chunk_rows=4, wnaf_width=4) as pin:
        got = conv_bytes(E, torch, CG.CASES["B"], w, cts, zero)
        level0, gathers, expands = pin.spans()
    assert got == want
    assert (level0, gathers, expands) == (3, 0, 0)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("route", [1, 2])
def test_grouped_conv_from_pointers_that_are_only_4_byte_aligned(route):
    """filters, image and output one word into their buffers: the dword expansion and gather, and level 0 reading the image as
    its table"""
    import torch
    d, k, w, cts, zero, want = case_data("s128_k128", "B")
    E = engine(d)
    with pinned(E, conv_route=route, wnaf_width=2 if route == 1 else 0) as pin:
        got = conv_bytes(E, torch, CG.CASES["B"], w, cts, zero, shift=1)
        spans = pin.spans()
    assert got == want
    check_route(CG.CASES["B"], route, spans)
    assert E.device_status(clear=False) == 0


def test_grouped_conv_under_the_default_options():
    """nothing pinned: the launcher's own choice of width gives the same bytes, and its choice of route for groups > 1 is the
    direct one (k_conv_level0 launched, neither k_gather_patches nor k_expand_group_filters) although B, with m = 12 and 108
    output records, is below the size at which an ungrouped convolution leaves the gather route"""
    import torch
    d, k, w, cts, zero, want = case_data("s128_k128", "B")
    E = engine(d)
    with pinned(E) as pin:
        got = conv_bytes(E, torch, CG.CASES["B"], w, cts, zero)
        spans = pin.spans()
    assert got == want
    check_route(CG.CASES["B"], 1, spans)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("prm_name", ["tiny_k8", "s128_k256"])
def test_depthwise_conv_on_the_other_parameter_sets(prm_name):
    import torch
    d, k, w, cts, zero, want = case_data(prm_name, "A")
    E = engine(d)
    with pinned(E, conv_route=1) as pin:
        got = conv_bytes(E, torch, CG.CASES["A"], w, cts, zero)
        assert pin.spans()[0] > 0
    assert got == want
    assert E.device_status(clear=False) == 0


# ---- sum pooling -------------------------------------------------------------------------------------------------------------

POOL_IMAGE, POOL_KERNEL, POOL_STRIDE = (1, 4, 6, 2), (2, 3), (2, 3)


def pool_device(E, torch, cts, zero, image=POOL_IMAGE, kernel=POOL_KERNEL, stride=POOL_STRIDE):
    ho, wo = image[1] // stride[0], image[2] // stride[1]
    dc, dz = records_of(E, torch, cts), records_of(E, torch, [zero])
    out = torch.zeros(image[0] * ho * wo * image[3] * 2 * REC, dtype=torch.int32, device="cuda")
    assert E.sum_pool2d_records(dc.data_ptr(), dz.data_ptr(), out.data_ptr(), image, kernel, stride) == (ho, wo)
    torch.cuda.synchronize()
    return host(out)


@pytest.mark.parametrize("route", [0, 1, 2])
def test_sum_pooling_equals_the_additions_and_the_old_trick(route):
    """2 x 3 windows at stride (2, 3) over a 1 x 4 x 6 x 2 image: zero plus the six shifted sub-images added with
    add_ciphertext_records, byte for byte; and the bytes of the 0/1 dense filter through the old entry.  conv_route 0 (automatic)
    takes the direct route, as 1 does"""
    import torch
    prm = load_json("params_s128_k128.json")
    d = hx(prm["delta"])
    E = engine(d)
    n, p = 1 * 2 * 2, 2
    cts, zero = random_cts(d, int(np.prod(POOL_IMAGE)), 71), random_cts(d, 1, 72)[0]
    with pinned(E, conv_route=route) as pin:
        got = pool_device(E, torch, cts, zero)
        spans = pin.spans()
    check_route((None,) * 5 + (POOL_IMAGE[3],), route or 1, spans)          # automatic with groups: the direct route
    recs = host(records_of(E, torch, cts)).reshape(1, 4, 6, 2, 2 * REC)
    acc = dev(torch, np.tile(host(records_of(E, torch, [zero])), n * p))
    for dy in range(POOL_KERNEL[0]):
        for dx in range(POOL_KERNEL[1]):
            part = dev(torch, recs[:, dy::POOL_STRIDE[0], dx::POOL_STRIDE[1], :, :].reshape(-1))
            E.add_ciphertext_records(acc.data_ptr(), part.data_ptr(), acc.data_ptr(), n * p)
    torch.cuda.synchronize()
    assert np.array_equal(got, host(acc))
    w = [1 if ci == co else 0 for _ in range(POOL_KERNEL[0] * POOL_KERNEL[1]) for ci in range(2) for co in range(2)]
    old = TC.conv_device(E, torch, (POOL_IMAGE, POOL_KERNEL, 2, POOL_STRIDE, (0, 0)), w, cts, zero)
    assert np.array_equal(got, old)
    assert E.device_status(clear=False) == 0


def int_grouped_conv(x, case, w, k):
    """the integer grouped and dilated convolution mod 2^k, channels last, on flat lists"""
    n, m, p, ho, wo = CG.sizes(case)
    cols = CG.column_im2col(case)
    return [sum(x[cols[row, j, c]] * w[j * p + c] for j in range(m) if cols[row, j, c] >= 0) % (1 << k) for row in range(n) for c in range(p)]


def test_grouped_conv_decrypts_and_pools(params128):
    """k = 128: a freshly encrypted 1 x 4 x 5 x 4 image under B's grouped filters (small weights of both signs) decrypts to the
    integer grouped convolution mod 2^k; its [1, 3, 3, 6] output under 2 x 2 sum pooling at stride 1 decrypts to the window sums"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(909)
    enc = lambda vals: fresh(E, torch, recs, vals, [rng.randrange(bound) for _ in vals], k)  # noqa: E731
    case = CG.CASES["B"]
    image, kernel, stride, pad, dilation, G, co = case
    n, m, p, ho, wo = CG.sizes(case)
    x = [rng.getrandbits(k) for _ in range(int(np.prod(image)))]
    w = [rng.randrange(-128, 128) for _ in range(m * p)]
    y = int_grouped_conv(x, case, w, k)
    cx, zero = enc(x), enc([0])
    cy = torch.zeros(len(y) * 2 * REC, dtype=torch.int32, device="cuda")
    assert E.conv2d_plain_ct_records(dev(torch, exp_records(w)).data_ptr(), cx.data_ptr(), zero.data_ptr(), cy.data_ptr(), image,
                                     CG.filters_of(case), stride, pad, dilation=dilation, groups=G) == (ho, wo)
    torch.cuda.synchronize()
    assert decrypt(E, torch, prm, cy, len(y), k) == y
    ya = np.array(y, dtype=object).reshape(ho, wo, p)
    z = [int(ya[oy:oy + 2, ox:ox + 2, c].sum()) % (1 << k) for oy in range(ho - 1) for ox in range(wo - 1) for c in range(p)]
    cz = torch.zeros(len(z) * 2 * REC, dtype=torch.int32, device="cuda")
    assert E.sum_pool2d_records(cy.data_ptr(), zero.data_ptr(), cz.data_ptr(), (1, ho, wo, p), (2, 2), (1, 1)) == (ho - 1, wo - 1)
    torch.cuda.synchronize()
    assert decrypt(E, torch, prm, cz, len(z), k) == z
    assert E.device_status(clear=False) == 0


# ---- refusals and the bytes entries ------------------------------------------------------------------------------------------

def test_grouped_refusals_leave_the_output_alone():
    """each of the eleven new COFHE_HIP_EINVAL of the shape check (groups of 0 and a channel count that groups does not divide
    among them) through the records entry with a real context and a filled output, and an output that overlaps the filters -- whose extent is that of the
    GROUPED filter: an output just behind it is fine though the dense filter would reach into it"""
    import torch
    from cofhe_amd import CofheHipError
    from test_conv_groups_cpu import REFUSALS
    d, k, w, cts, zero, want = case_data("s128_k128", "B")
    E = engine(d)
    case = CG.CASES["B"]
    image, kernel, stride, pad, dilation, G, co = case
    n, m, p, ho, wo = CG.sizes(case)
    o_cts, o_zero = m * p * 32, m * p * 32 + len(cts) * 2 * REC
    o_out = o_zero + 2 * REC
    buf = torch.cat([dev(torch, exp_records(w)), records_of(E, torch, cts), records_of(E, torch, [zero]),
                     torch.full((n * p * 2 * REC,), FILL, dtype=torch.int32, device="cuda")])
    before = buf.clone()
    base = buf.data_ptr()
    ptrs = (base, base + 4 * o_cts, base + 4 * o_zero)
    assert len(REFUSALS) == 11
    for why, (im, ker, c_o, st, pd, dil, g) in REFUSALS.items():
        third = im[3] // g if g else im[3]                  # groups = 0: any extent reaches the entry, which refuses the geometry
        with pytest.raises(CofheHipError) as ei:
            E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, im, (*ker, third, c_o), st, pd, dilation=dil, groups=g)
        assert ei.value.code == EINVAL, why
        torch.cuda.synchronize()
        assert torch.equal(buf, before), why
    for out in (base + 4 * (o_cts - 1), base + 4 * (o_cts + REC), base + 4 * (o_zero + 2 * REC - 1)):
        with pytest.raises(CofheHipError) as ei:
            E.conv2d_plain_ct_records(*ptrs, out, image, CG.filters_of(case), stride, pad, dilation=dilation, groups=G)
        assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    with pytest.raises(CofheHipError) as ei:
        E.sum_pool2d_records(base + 4 * o_cts, base + 4 * o_zero, base + 4 * o_zero, image, (2, 2))
    assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    assert E.sum_pool2d_records(base + 4 * o_cts, base + 4 * o_zero, base + 4 * o_out, (1, 4, 5, 0), (2, 2)) == (2, 2)          # no channels: nothing to do
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    E.conv2d_plain_ct_records(*ptrs, base + 4 * o_out, image, CG.filters_of(case), stride, pad, dilation=dilation, groups=G)
    torch.cuda.synchronize()
    assert torch.equal(buf[:o_out], before[:o_out])
    assert E.records_to_bytes(host(buf[o_out:]), [image[0], ho, wo, p]) == want
    # an output that starts where the grouped filter ends, inside what the dense filter (G times as long) would cover: no overlap
    out2 = torch.full((n * p * 2 * REC,), FILL, dtype=torch.int32, device="cuda")
    tail = torch.cat([dev(torch, exp_records(w)), out2])
    E.conv2d_plain_ct_records(tail.data_ptr(), base + 4 * o_cts, base + 4 * o_zero, tail.data_ptr() + 4 * o_cts, image, CG.filters_of(case), stride,
                              pad, dilation=dilation, groups=G)
    torch.cuda.synchronize()
    assert E.records_to_bytes(host(tail[o_cts:]), [image[0], ho, wo, p]) == want
    assert E.device_status(clear=False) == 0


def test_grouped_bytes_entries():
    """conv2d_plain_ct_tensors with groups equals the records entry and returns the 4-D tensor [B, Ho, Wo, Co]; a third filter
    extent other than C / groups is COFHE_HIP_ESHAPE; a refused geometry is COFHE_HIP_EINVAL; sum_pool2d_tensors equals
    sum_pool2d_records with the header [B, Ho, Wo, C]"""
    import torch
    from cofhe_amd import CofheHipError
    d, k, w, cts, zero, want = case_data("s128_k128", "B")
    E = engine(d)
    case = CG.CASES["B"]
    image, kernel, stride, pad, dilation, G, co = case
    n, m, p, ho, wo = CG.sizes(case)
    wb = _pt_bytes(list(CG.filters_of(case)), w)
    cb, zb = P.serialize_ciphertext_tensor(list(image), cts), P.serialize_ciphertext_tensor([1], [zero])
    got = E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad, dilation, G)
    assert got == want
    assert list(np.frombuffer(got[:20], dtype="<u4")) == [4, image[0], ho, wo, co]
    for call in (lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad, dilation, 1),                   # third extent 2, C / 1 = 4
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad, dilation, 4),                   # C / 4 = 1
                 lambda: E.conv2d_plain_ct_tensors(_pt_bytes([kernel[0], kernel[1], image[3], co // 2], w), cb, zb, stride, pad, (1, 2), G),
                 lambda: E.conv2d_plain_ct_tensors(_pt_bytes([m, p], w), cb, zb, stride, pad, dilation, G)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == ESHAPE
    for call in (lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad, (0, 1), G),
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, pad, dilation, 0),
                 lambda: E.conv2d_plain_ct_tensors(wb, cb, zb, stride, (0, 5), (1, 2), G)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    pcts, pzero = random_cts(d, int(np.prod(POOL_IMAGE)), 71), random_cts(d, 1, 72)[0]
    pooled = E.sum_pool2d_tensors(P.serialize_ciphertext_tensor(list(POOL_IMAGE), pcts), P.serialize_ciphertext_tensor([1], [pzero]), POOL_KERNEL)
    assert list(np.frombuffer(pooled[:20], dtype="<u4")) == [4, 1, 2, 2, 2]
    assert pooled == E.records_to_bytes(pool_device(E, torch, pcts, pzero), [1, 2, 2, 2])
    assert E.device_status(clear=False) == 0


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")


def test_local_bench_conv2d_grouped(tmp_path):
    """HIPCryptoSystem::conv2d_plaintext_ciphertext_tensors with dilation and groups on a 1 x 6 x 6 x 4 image with 3 x 3 x 2 x 6
    filters in two groups, dilation (2, 1): the tensor decrypts to the integer grouped convolution mod 2^k"""
    r = subprocess.run([EXE, "conv2d_grouped", "1", "6", "6", "4", "3", "3", "6", "2", "2", "1"], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "decrypts to the grouped convolution: yes" in r.stdout, r.stdout


def test_local_bench_sum_pool2d(tmp_path):
    """HIPCryptoSystem::sum_pool2d_ciphertext_tensor: 2 x 2 windows at stride 2 over a 1 x 6 x 6 x 3 image decrypt to the sums"""
    r = subprocess.run([EXE, "sum_pool2d", "1", "6", "6", "3", "2", "2"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "decrypts to the window sums: yes" in r.stdout, r.stdout
