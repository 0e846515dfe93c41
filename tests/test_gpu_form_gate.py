"""The form gate on the GPU (k_validate_forms behind validate_records, unpack_tensor_device and every *_tensors_bytes entry
point) against the Python predicate of form_gate_cases: one clause at a time, in every group slot of a wavefront, at the
edges of the launch, through the wire format and through every operand that takes forms from outside.

Forged records go to validate_records and unpack_tensor_device only; an arithmetic entry point sees forged bytes only after
unpack_tensor_device has refused those very bytes in the same test, so a hole in the gate fails the test before a malformed
form can reach a composition."""
import numpy as np
import pytest

import form_gate_cases as G
import simlib as S
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, form_record, hx  # noqa: F401

pytestmark = pytest.mark.gpu
REC = 168
REFUSED = "not a reduced form"


def dev(torch, recs):
    return torch.from_numpy(np.concatenate([S.raw_record(*r) for r in recs]).view(np.int32)).cuda()


def to_gpu(torch, data):
    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


@pytest.fixture(scope="module", params=range(5), ids=[d.name for d in G.discriminants()])
def disc(request):
    return G.discriminants()[request.param]


def test_a_2401_bit_discriminant_is_refused():
    from cofhe_amd import CofheHipError, Engine
    engine(G.discriminants()[4].delta)                     # 2400 bits: taken
    with pytest.raises(CofheHipError, match="above 2400 bits"):
        Engine(G.too_wide_discriminant())


def test_every_record_alone(disc):
    """n = 1: the verdict of the kernel is the Python predicate's, record by record"""
    import torch
    E = engine(disc.delta)
    buf = dev(torch, [cs.rec for cs in disc.cases])
    for i, cs in enumerate(disc.cases):
        want = G.valid(cs.rec, -disc.delta)
        assert want == (cs.names is None)
        assert E.validate_records(buf.data_ptr() + 4 * REC * i, 1) == want, (disc.name, cs.label)
    assert E.device_status(clear=False) == 0


def test_every_forgery_in_every_group_slot(disc):
    """n = 8, one wavefront: each forgery in each of its 8 limb groups beside 7 valid records"""
    import torch
    E = engine(disc.delta)
    ok = G.passes(disc)[:8]
    base = dev(torch, [cs.rec for cs in ok])
    assert E.validate_records(base.data_ptr(), 8)
    bad = G.forgeries(disc)
    forged = dev(torch, [cs.rec for cs in bad])
    for i, cs in enumerate(bad):
        for slot in range(8):
            buf = base.clone()
            buf[slot * REC:(slot + 1) * REC] = forged[i * REC:(i + 1) * REC]
            assert not E.validate_records(buf.data_ptr(), 8), (disc.name, cs.label, slot)
    assert E.validate_records(base.data_ptr(), 8)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257])
def test_placement_count_and_no_latch(n):
    """one forgery at the first record, at both sides of the workgroup edge (32 groups) and at the last record; a forgery just
    past the count is not looked at; a valid call straight after an invalid one is valid"""
    import torch
    d = G.discriminants()[1]
    E = engine(d.delta)
    ok = [cs.rec for cs in G.passes(d)]
    by = {cs.label: cs.rec for cs in d.cases}
    good = dev(torch, [ok[i % len(ok)] for i in range(n + 1)])
    assert E.validate_records(good.data_ptr(), n + 1)
    for label in ("c_plus_1", "content2_random"):
        forged = dev(torch, [by[label]])
        for idx in sorted({0, 31, 32, n - 1}):
            if idx >= n:
                continue
            buf = good.clone()
            buf[idx * REC:(idx + 1) * REC] = forged
            assert not E.validate_records(buf.data_ptr(), n), (label, idx)
            assert E.validate_records(good.data_ptr(), n), "the verdict must not latch"
        buf = good.clone()
        buf[n * REC:(n + 1) * REC] = forged
        assert E.validate_records(buf.data_ptr(), n), "record n is outside a count of n"
        assert not E.validate_records(buf.data_ptr(), n + 1)
    assert E.device_status(clear=False) == 0


def test_wire_refuses_every_forgery_it_can_express(disc):
    """kind 2 with the forgery as c1 and as c2, kind 1 with the forgery alone: each is refused by unpack_tensor_device"""
    import torch
    from cofhe_amd import CofheHipError
    E = engine(disc.delta)
    g = G.as_form(G.passes(disc)[0].rec)
    rec = torch.zeros(2 * REC, dtype=torch.int32, device="cuda")
    sent = 0
    for cs in G.forgeries(disc):
        if not G.on_wire(cs.rec):
            continue
        f = G.as_form(cs.rec)
        for kind, data in ((2, P.serialize_ciphertext_tensor([1], [(f, g)])), (2, P.serialize_ciphertext_tensor([1], [(g, f)])),
                           (1, P.serialize_form_tensor([1], [f]))):
            t = to_gpu(torch, data)
            with pytest.raises(CofheHipError, match=REFUSED):
                E.unpack_tensor_device(t.data_ptr(), len(data), kind, rec.data_ptr(), 2)
            sent += 1
    assert sent >= 3 * 30
    assert E.device_status(clear=False) == 0


def test_wire_takes_every_pass_record_and_repacks_it(disc):
    """the pass-records as one ciphertext tensor and as one partial-decryption tensor: unpacked to the records of the table,
    packed again byte for byte; a zero b travels with its sign flag set (the reference's flag for zero) and arrives as +0,
    while the same thing said as a record, sign word 1, is refused"""
    import torch
    E = engine(disc.delta)
    ok = G.passes(disc)
    ok = ok + ok[:len(ok) % 2]
    forms = [G.as_form(cs.rec) for cs in ok]
    want = np.concatenate([S.raw_record(*cs.rec) for cs in ok])
    n = len(forms)
    for kind, data, shape in ((2, P.serialize_ciphertext_tensor([n // 2], list(zip(forms[0::2], forms[1::2]))), [n // 2]),
                              (1, P.serialize_form_tensor([n], forms), [n])):
        t = to_gpu(torch, data)
        rec = torch.full((n * REC,), -1, dtype=torch.int32, device="cuda")
        assert E.unpack_tensor_device(t.data_ptr(), len(data), kind, rec.data_ptr(), n) == (shape, n)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32), want)
        cap = E.packed_size_bound(n, kind, 1)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        ln = E.pack_tensor_device(rec.data_ptr(), n, kind, shape, out.data_ptr(), cap)
        assert out.cpu().numpy()[:ln].tobytes() == data
    zero_b = [cs for cs in ok if cs.rec[1] == 0]
    if disc.delta % 2 == 0:
        f = G.as_form(zero_b[0].rec)
        data = P.serialize_form_tensor([1], [f])
        assert int.from_bytes(data[8 + 8:8 + 16], "little") >> 63 == 1, "b = 0 carries the flag on the wire"
        t = to_gpu(torch, data)
        rec = torch.full((REC,), -1, dtype=torch.int32, device="cuda")
        assert E.unpack_tensor_device(t.data_ptr(), len(data), 1, rec.data_ptr(), 1) == ([1], 1)
        assert np.array_equal(rec.cpu().numpy().view(np.uint32), S.raw_record(f.a, 0, 0, f.c))
        rec[160] = 1
        assert not E.validate_records(rec.data_ptr(), 1)
    assert E.device_status(clear=False) == 0


def _sweep(prm):
    """(name, call(operand bytes...), operands) for every *_tensors_bytes entry point of include/cofhe_hip.h: `operands` maps
    the name of each operand that carries forms to its shape; the call takes them by name"""
    k = prm["k"]
    f = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    pt = _pt_bytes
    return [
        ("add", lambda E, t1, t2: E.add_ciphertext_tensors(t1, t2), {"t1": [3], "t2": [3]}),
        ("sub", lambda E, t1, t2: E.sub_ciphertext_tensors(t1, t2), {"t1": [2, 2], "t2": [2, 2]}),
        ("add_plaintext", lambda E, cts: E.add_plaintext_tensor(cts, pt([3], [5, -7, 0]), f, k, 0), {"cts": [3]}),
        ("scal_1d", lambda E, cts: E.scal_ciphertext_tensors(pt([2], [3, -5]), cts), {"cts": [2]}),
        ("scal_2d", lambda E, cts, zero: E.scal_ciphertext_tensors(pt([2, 1], [3, 5]), cts, zero), {"cts": [2, 2], "zero": [1]}),
        ("matmul_plain_ct", lambda E, cts, zero: E.matmul_plain_ct_tensors(pt([1, 2], [3, 5]), cts, zero), {"cts": [2, 2], "zero": [1]}),
        ("conv2d", lambda E, cts, zero: E.conv2d_plain_ct_tensors(pt([1, 1, 1, 1], [3]), cts, zero), {"cts": [1, 2, 2, 1], "zero": [1]}),
        ("conv2d_grouped", lambda E, cts, zero: E.conv2d_plain_ct_tensors(pt([1, 1, 1, 2], [3, 5]), cts, zero, groups=2),
         {"cts": [1, 1, 2, 2], "zero": [1]}),
        ("sum_pool2d", lambda E, cts, zero: E.sum_pool2d_tensors(cts, zero, (2, 1)), {"cts": [1, 2, 2, 1], "zero": [1]}),
        ("poly_close", lambda E, powers: E.poly_close_tensors(pt([3], [1, 2, 3]), pt([2], [7, 9]), powers, f, k), {"powers": [2, 2]}),
        ("div_close", lambda E, rq: E.div_close_tensors_bytes(pt([3], [7, 9, 11]), pt([1], [3]), rq, f, k), {"rq": [3]}),
    ]


def test_the_sweep_names_every_bytes_entry_point():
    import os
    import re
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "cofhe_hip.h")) as fh:
        declared = set(re.findall(r"int (cofhe_hip_\w+_tensors?_bytes)\(cofhe_hip_ctx", fh.read()))
    swept = {"cofhe_hip_add_ciphertext_tensors_bytes", "cofhe_hip_sub_ciphertext_tensors_bytes", "cofhe_hip_add_plaintext_tensor_bytes",
             "cofhe_hip_scal_ciphertext_tensors_bytes", "cofhe_hip_matmul_plain_ct_tensors_bytes", "cofhe_hip_conv2d_plain_ct_tensors_bytes",
             "cofhe_hip_conv2d_grouped_plain_ct_tensors_bytes", "cofhe_hip_sum_pool2d_tensors_bytes", "cofhe_hip_poly_close_tensors_bytes",
             "cofhe_hip_div_close_tensors_bytes"}
    assert declared == swept, "a new *_bytes entry point belongs in _sweep"


SWEEP_NAMES = ("add", "sub", "add_plaintext", "scal_1d", "scal_2d", "matmul_plain_ct", "conv2d", "conv2d_grouped", "sum_pool2d", "poly_close",
               "div_close")


@pytest.mark.parametrize("entry", range(len(SWEEP_NAMES)), ids=SWEEP_NAMES)
def test_every_entry_point_refuses_a_forgery_in_every_operand(params128, entry):
    """k = 128, tensors of 1 to 4 elements: one equation forgery (c + 1) and one non-primitive forgery in each operand that
    carries forms, as c1 of the first element and as c2 of the last, the other operands valid"""
    import torch
    from cofhe_amd import CofheHipError
    d = G.discriminants()[1]
    assert d.delta == hx(params128["delta"])
    E = engine(d.delta)
    name, call, operands = _sweep(params128)[entry]
    assert name == SWEEP_NAMES[entry] and len(_sweep(params128)) == len(SWEEP_NAMES)
    ok = [G.as_form(cs.rec) for cs in G.passes(d)]
    by = {cs.label: cs.rec for cs in d.cases}

    def tensor(shape, seed, forged=None, at=None):
        n = int(np.prod(shape))
        cts = [(ok[(seed + 2 * i) % len(ok)], ok[(seed + 2 * i + 1) % len(ok)]) for i in range(n)]
        if at == "first_c1":
            cts[0] = (forged, cts[0][1])
        if at == "last_c2":
            cts[-1] = (cts[-1][0], forged)
        return P.serialize_ciphertext_tensor(shape, cts)

    rec = torch.zeros(8 * REC, dtype=torch.int32, device="cuda")
    valid_ops = {op: tensor(shape, 3 * j) for j, (op, shape) in enumerate(operands.items())}
    assert len(call(E, **valid_ops)) > 0, "with valid operands the call goes through: a refusal below is about the forgery"
    for op, shape in operands.items():
        assert 1 <= int(np.prod(shape)) <= 4
        for label in ("c_plus_1", "content2_random"):
            forged = G.as_form(by[label])
            for at in ("first_c1", "last_c2"):
                data = tensor(shape, 1, forged, at)
                t = to_gpu(torch, data)
                with pytest.raises(CofheHipError, match=REFUSED):          # the gate first: nothing forged goes past a hole
                    E.unpack_tensor_device(t.data_ptr(), len(data), 2, rec.data_ptr(), 8)
                with pytest.raises(CofheHipError, match=REFUSED):
                    call(E, **dict(valid_ops, **{op: data}))
    assert E.device_status(clear=False) == 0
