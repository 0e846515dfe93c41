"""GPU: the plaintext-left matrix product W . [x] and what the matrix Beaver triplets add (cofhe_amd/csrc/matmul_left.hip):
cofhe_hip_matmul_plain_plain_records against Python integers, cofhe_hip_matmul_plain_ct_records against the C++/GMP oracle
byte for byte -- the expected value built element by element, without a transposition --, its launch routes, the refusal of
an overlapping output, the bytes entry point, the Beaver identity X Y = E [B] + [A] D + [C] + E D through the engine alone,
and the C++ host layer (local_bench plain_ct_matmul, ciphertext_matmul_matrix)."""
import os
import random
import re
import subprocess

import numpy as np
import pytest

import plain_mm_cases as PM
from conftest import ROOT
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes, engine, exp_records, hx  # noqa: F401
import oracle_lib as O
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
REC = 168
EINVAL, ESHAPE = -1, -2


# ---- the plaintext matrix product mod 2^k ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", PM.KBITS)
def test_plain_plain_matches_python_integers(params128, k):
    """k_plain_matmul on the grid of the CPU tier (tests/plain_mm_cases.py): one limb with a sub-word mask, a mask inside the
    top limb, 4 and 8 limbs, the runtime limb count; one element, ragged shapes, either side of the 16 x 16 tile with an inner
    dimension of 33; 0, 1, -1, 2^k - 1 everywhere, magnitudes of 2^k and above, mixed signs.  Exact; sign word 0; nothing
    at or above bit k"""
    import torch
    E = engine(hx(params128["delta"]))
    for name, n, m, p, a, b in PM.cases(k):
        da, db = dev(torch, PM.exp_records(a)), dev(torch, PM.exp_records(b))
        out = torch.full((n * p * 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        E.matmul_plain_plain_records(da.data_ptr(), db.data_ptr(), out.data_ptr(), n, m, p, k)
        torch.cuda.synchronize()
        PM.check_output(host(out), PM.product(a, b, n, m, p, k), k)
    assert E.device_status(clear=False) == 0


def test_plain_plain_refusals_and_empty_shapes(params128):
    """k = 0 and k = 640 (beyond the 20-limb tile buffers) are COFHE_HIP_EINVAL, so is an output that overlaps an operand;
    n p = 0 launches nothing; m = 0 gives zeros"""
    import torch
    from cofhe_amd import CofheHipError
    E = engine(hx(params128["delta"]))
    a = dev(torch, PM.exp_records([3, -5, 7, 9]))
    out = torch.full((4 * 32,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    for call in (lambda: E.matmul_plain_plain_records(a.data_ptr(), a.data_ptr(), out.data_ptr(), 2, 2, 2, 0),
                 lambda: E.matmul_plain_plain_records(a.data_ptr(), a.data_ptr(), out.data_ptr(), 2, 2, 2, 640),
                 lambda: E.matmul_plain_plain_records(a.data_ptr(), a.data_ptr(), a.data_ptr() + 128, 2, 2, 2, 128)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    E.matmul_plain_plain_records(a.data_ptr(), a.data_ptr(), out.data_ptr(), 0, 2, 2, 128)
    torch.cuda.synchronize()
    assert (host(out) == 0x5A5A5A5A).all()
    E.matmul_plain_plain_records(a.data_ptr(), a.data_ptr(), out.data_ptr(), 2, 0, 2, 128)
    torch.cuda.synchronize()
    PM.check_output(host(out), [0] * 4, 128)
    assert E.device_status(clear=False) == 0


# ---- the plaintext-left product ------------------------------------------------------------------------------------------------

def random_cts(d, count, seed, nbase=12):
    rng = P.SplitMix64(seed)
    small = (-d).bit_length() < 256
    base = [P.random_form(d, rng, 12, 10) if small else P.random_form(d, rng) for _ in range(nbase)]
    return [(base[rng.below(nbase)], base[rng.below(nbase)]) for _ in range(count)]


def exponents(k, count, seed):
    """0, 1, -1, a k-bit value and one 300-bit value, then short and k-bit values of both signs, shuffled; fewer than five
    elements take the end of that list (one element: the 300-bit value)"""
    rng = random.Random(seed)
    edge = [0, 1, -1, (1 << k) - 3, rng.getrandbits(300) | (1 << 299)]
    if count < len(edge):
        return edge[len(edge) - count:]
    vals = edge + [rng.choice((1, -1)) * rng.getrandbits(rng.choice((5, 14, k))) for _ in range(count - len(edge))]
    rng.shuffle(vals)
    return vals


def want_elementwise(d, s, cts, zero, n, m, p):
    """want[i,k] = zero + sum_j s[i,j] * cts[j,k] with the oracle's element-wise scal_1d and add; no transposition anywhere:
    term j holds s[i,j] * cts[j,k] at its flat index i p + k"""
    acc = P.serialize_ciphertext_tensor([n * p], [zero] * (n * p))
    for j in range(m):
        sv = [s[i * m + j] for i in range(n) for _ in range(p)]
        cv = [cts[j * p + c] for _ in range(n) for c in range(p)]
        acc = O.add(d, acc, O.scal_1d(d, _pt_bytes([n * p], sv), P.serialize_ciphertext_tensor([n * p], cv)))
    return P.serialize_ciphertext_tensor([n, p], P.deserialize_ciphertext_tensor(acc)[1])


def want_transposed(d, s, cts, zero, n, m, p):
    """the same through the oracle's ciphertext-left scal_2d on transposed operands, transposed back"""
    s_t = [s[i * m + j] for j in range(m) for i in range(n)]
    cts_t = [cts[j * p + c] for c in range(p) for j in range(m)]
    out_t = P.deserialize_ciphertext_tensor(O.scal_2d(d, _pt_bytes([m, n], s_t), P.serialize_ciphertext_tensor([p, m], cts_t),
                                                      P.serialize_ciphertext_tensor([1], [zero])))[1]
    return P.serialize_ciphertext_tensor([n, p], [out_t[c * n + i] for i in range(n) for c in range(p)])


def records_of(E, torch, cts):
    return dev(torch, E.bytes_to_records(P.serialize_ciphertext_tensor([len(cts)], cts))[1])


def left_records(E, torch, s, cts, zero, n, m, p, shift=0):
    """matmul_plain_ct_records -> serialised n x p tensor; shift: s, cts and out start that many words into their buffers (a
    pointer that is only 4-byte aligned)"""
    ds = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), exp_records(s)]))
    dc = dev(torch, np.concatenate([np.zeros(shift, dtype=np.uint32), host(records_of(E, torch, cts))]))
    dz = records_of(E, torch, [zero])
    out = torch.zeros(shift + n * p * 2 * REC, dtype=torch.int32, device="cuda")
    E.matmul_plain_ct_records(ds.data_ptr() + 4 * shift, dc.data_ptr() + 4 * shift, dz.data_ptr(), out.data_ptr() + 4 * shift, n, m, p)
    torch.cuda.synchronize()
    assert not host(out)[:shift].any()
    return E.records_to_bytes(host(out)[shift:], [n, p])


@pytest.mark.parametrize("n,m,p", [(1, 1, 1), (3, 5, 4), (4, 2, 7)])
def test_plain_ct_matches_the_oracle(params128, n, m, p):
    """byte for byte against the element-wise expectation, with n, m, p pairwise different (a swapped index cannot pass);
    exponents 0, 1, -1, a k-bit value, a 300-bit value.  The same from pointers that are only 4-byte aligned (the dword
    transposes)"""
    import torch
    d, k = hx(params128["delta"]), params128["k"]
    E = engine(d)
    s, cts, zero = exponents(k, n * m, 10 * n + m), random_cts(d, m * p, 77 + p), random_cts(d, 1, 78)[0]
    want = want_elementwise(d, s, cts, zero, n, m, p)
    assert left_records(E, torch, s, cts, zero, n, m, p) == want
    assert left_records(E, torch, s, cts, zero, n, m, p, shift=1) == want
    assert E.device_status(clear=False) == 0


def test_plain_ct_on_every_parameter_set(golden):
    """(3, 5, 4) for tiny_k8, k = 128 and k = 256"""
    import torch
    d, k = hx(golden[0]["delta"]), golden[0]["k"]
    E = engine(d)
    n, m, p = 3, 5, 4
    s, cts, zero = exponents(k, n * m, 500 + k), random_cts(d, m * p, 501 + k), random_cts(d, 1, 502 + k)[0]
    assert left_records(E, torch, s, cts, zero, n, m, p) == want_elementwise(d, s, cts, zero, n, m, p)
    assert E.device_status(clear=False) == 0


def test_plain_ct_empty_shapes(params128):
    """n p = 0 is a no-op; m = 0 gives zero everywhere"""
    import torch
    d = hx(params128["delta"])
    E = engine(d)
    zero = random_cts(d, 1, 79)[0]
    E.matmul_plain_ct_records(0, 0, 0, 0, 0, 3, 4)
    E.matmul_plain_ct_records(0, 0, 0, 0, 3, 3, 0)
    assert left_records(E, torch, [], [], zero, 2, 0, 3) == P.serialize_ciphertext_tensor([2, 3], [zero] * 6)
    assert E.device_status(clear=False) == 0


@pytest.mark.parametrize("n,m,p,tree", [(2, 16, 3, -1), (5, 8, 4, 1), (5, 8, 4, 0)])
def test_plain_ct_routes(params128, n, m, p, tree):
    """the routes of the product underneath, against the oracle's scal_2d on transposed operands: (2, 16, 3) under the default
    options (few outputs, a long inner dimension: the segmented chains), (5, 8, 4) pinned onto the product tree and onto the
    chains"""
    import torch
    d, k = hx(params128["delta"]), params128["k"]
    E = engine(d)
    s, cts, zero = exponents(k, n * m, 900 + m), random_cts(d, m * p, 901 + m), random_cts(d, 1, 902)[0]
    E.profile_read("k_tree_level", clear=True)
    E.set_option("matmul_tree", tree)
    E.set_option("profile_kernels", 1)
    try:
        got = left_records(E, torch, s, cts, zero, n, m, p)
        levels, chains = E.profile_read("k_tree_level")[1], E.profile_read("k_scal_matmul_wnaf")[1]
    finally:
        E.set_option("profile_kernels", 0)
        E.set_option("matmul_tree", -1)
        E.profile_read("k_tree_level", clear=True)
    assert got == want_transposed(d, s, cts, zero, n, m, p)
    assert (levels > 0) == (tree == 1) and chains == 1              # the tree's top level ends in the same Horner kernel
    assert E.device_status(clear=False) == 0


def test_plain_ct_refuses_an_overlapping_output(params128):
    """d_out inside d_cts, ending in d_s, or on d_zero: COFHE_HIP_EINVAL and not a word written"""
    import torch
    from cofhe_amd import CofheHipError
    d, k = hx(params128["delta"]), params128["k"]
    E = engine(d)
    n, m, p = 2, 3, 2
    buf = torch.cat([records_of(E, torch, random_cts(d, m * p, 88)), dev(torch, exp_records(exponents(k, n * m, 89))),
                     records_of(E, torch, random_cts(d, 1, 90)), torch.zeros(n * p * 2 * REC, dtype=torch.int32, device="cuda")])
    base = buf.data_ptr()
    o_s, o_z, o_out = 4 * m * p * 2 * REC, 4 * (m * p * 2 * REC + n * m * 32), 4 * (m * p * 2 * REC + n * m * 32 + 2 * REC)
    before = buf.clone()
    for out in (base + 4 * REC, base + o_s - 4, base + o_z - 4 * (n * p * 2 * REC - 1), base + o_z):
        with pytest.raises(CofheHipError) as ei:
            E.matmul_plain_ct_records(base + o_s, base, base + o_z, out, n, m, p)
        assert ei.value.code == EINVAL and "overlaps" in str(ei.value)
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    E.matmul_plain_ct_records(base + o_s, base, base + o_z, base + o_out, n, m, p)        # next to its inputs: fine
    torch.cuda.synchronize()
    assert torch.equal(buf[: o_out // 4], before[: o_out // 4]) and host(buf[o_out // 4:]).any()
    assert E.device_status(clear=False) == 0


def test_plain_ct_bytes_entry(params128):
    """matmul_plain_ct_tensors equals the records entry at (3, 5, 4); operands that are not 2-D or whose inner dimensions
    differ are COFHE_HIP_ESHAPE; a tensor holding a non-form is COFHE_HIP_EINVAL"""
    import torch
    from cofhe_amd import CofheHipError
    d, k = hx(params128["delta"]), params128["k"]
    E = engine(d)
    n, m, p = 3, 5, 4
    s, cts, zero = exponents(k, n * m, 300), random_cts(d, m * p, 301), random_cts(d, 1, 302)[0]
    sb, cb, zb = _pt_bytes([n, m], s), P.serialize_ciphertext_tensor([m, p], cts), P.serialize_ciphertext_tensor([1], [zero])
    assert E.matmul_plain_ct_tensors(sb, cb, zb) == left_records(E, torch, s, cts, zero, n, m, p)
    for call in (lambda: E.matmul_plain_ct_tensors(_pt_bytes([m, n], s), cb, zb),
                 lambda: E.matmul_plain_ct_tensors(sb, P.serialize_ciphertext_tensor([p, m], cts), zb),
                 lambda: E.matmul_plain_ct_tensors(_pt_bytes([n * m], s), cb, zb),
                 lambda: E.matmul_plain_ct_tensors(sb, P.serialize_ciphertext_tensor([m * p], cts), zb)):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == ESHAPE
    f = cts[7][1]
    bad = list(cts)
    bad[7] = (cts[7][0], P.Form(f.a, f.b, f.c + 1))            # b^2 - 4 a c is no longer the discriminant
    for call in (lambda: E.matmul_plain_ct_tensors(sb, P.serialize_ciphertext_tensor([m, p], bad), zb),
                 lambda: E.matmul_plain_ct_tensors(sb, cb, P.serialize_ciphertext_tensor([1], [bad[7]]))):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL
    assert E.device_status(clear=False) == 0


def test_beaver_matrix_identity_through_the_engine(params128):
    """k = 128, X 3 x 4, Y 4 x 2, a matrix triplet [A], [B], [C = A B]: E = Dec(X - A), D = Dec(Y - B), then
    E [B] + [A] D + [C] + E D decrypts to X Y mod 2^k -- every step an Engine call, all five tensors freshly encrypted"""
    import torch
    prm = params128
    d, k, forms, recs, bound = setup(prm)
    E = engine(d)
    rng = random.Random(606)
    n, m, p, M = 3, 4, 2, 1 << k
    rand = lambda c: [rng.getrandbits(k) for _ in range(c)]                                  # noqa: E731
    enc = lambda vals: fresh(E, torch, recs, vals, [rng.randrange(bound) for _ in vals], k)  # noqa: E731
    mm = lambda a, b: PM.product(a, b, n, m, p, k)                                           # noqa: E731
    X, Y, A, B = rand(n * m), rand(m * p), rand(n * m), rand(m * p)
    cX, cY, cA, cB, cC = enc(X), enc(Y), enc(A), enc(B), enc(mm(A, B))
    zero = enc([0])
    xa, yb = torch.zeros_like(cX), torch.zeros_like(cY)
    E.sub_ciphertext_records(cX.data_ptr(), cA.data_ptr(), xa.data_ptr(), n * m)
    E.sub_ciphertext_records(cY.data_ptr(), cB.data_ptr(), yb.data_ptr(), m * p)
    Ev, Dv = decrypt(E, torch, prm, xa, n * m, k), decrypt(E, torch, prm, yb, m * p, k)
    assert Ev == [(x - a) % M for x, a in zip(X, A)] and Dv == [(y - b) % M for y, b in zip(Y, B)]
    dE, dD = dev(torch, exp_records(Ev)), dev(torch, exp_records(Dv))
    eb = torch.zeros(n * p * 2 * REC, dtype=torch.int32, device="cuda")
    ad, acc = torch.zeros_like(eb), torch.zeros_like(eb)
    ed = torch.zeros(n * p * 32, dtype=torch.int32, device="cuda")
    E.matmul_plain_ct_records(dE.data_ptr(), cB.data_ptr(), zero.data_ptr(), eb.data_ptr(), n, m, p)
    E.scal_matmul_records(cA.data_ptr(), dD.data_ptr(), zero.data_ptr(), ad.data_ptr(), n, m, p)
    E.add_ciphertext_records(eb.data_ptr(), ad.data_ptr(), acc.data_ptr(), n * p)
    E.add_ciphertext_records(acc.data_ptr(), cC.data_ptr(), acc.data_ptr(), n * p)
    E.matmul_plain_plain_records(dE.data_ptr(), dD.data_ptr(), ed.data_ptr(), n, m, p, k)
    E.add_plain_records(acc.data_ptr(), ed.data_ptr(), recs["f"], acc.data_ptr(), n * p, k, 0)
    torch.cuda.synchronize()
    PM.check_output(host(ed), mm(Ev, Dv), k)
    assert decrypt(E, torch, prm, acc, n * p, k) == mm(X, Y)
    assert E.device_status(clear=False) == 0


# ---- the C++ host layer ----------------------------------------------------------------------------------------------------------

EXE = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")


def test_local_bench_plain_ct_matmul(tmp_path, params128):
    """HIPCryptoSystem::matmul_plaintext_ciphertext_tensors at (3, 5, 4): the tensor it serialises equals the oracle's
    element-wise expectation on the operands it wrote, and decrypts to W x"""
    r = subprocess.run([EXE, "plain_ct_matmul", "3", "5", "4"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "decrypts to W x: yes" in r.stdout, r.stdout
    rd = lambda name: open(tmp_path / ("local_bench_lmm_%s.bin" % name), "rb").read()       # noqa: E731
    delta = -int(open(tmp_path / "local_bench_absdelta.txt").read().strip())
    E = engine(hx(params128["delta"]))                  # the format conversions are host code of any context
    shape, ex = E.bytes_to_exponents(rd("s"))
    assert shape == [3, 5]
    s = [-v if sign else v for v, sign in PM.record_values(ex)]
    (cshape, cts), (_, zero) = P.deserialize_ciphertext_tensor(rd("cts")), P.deserialize_ciphertext_tensor(rd("zero"))
    assert cshape == [5, 4]
    assert rd("out") == want_elementwise(delta, s, cts, zero[0], 3, 5, 4)


@pytest.mark.parametrize("threshold", [(), ("2", "3")])
def test_local_bench_ciphertext_matmul_matrix(tmp_path, threshold):
    """the element flow and the matrix-triplet flow of LocalCipherTextMultiplier at (3, 4, 2), with the secret key and by
    2-of-3 threshold decryption: both equal the exact product, the matrix flow opens 3 4 + 4 2 = 20 values, the element flow
    2 (3 4 2) = 48"""
    r = subprocess.run([EXE, "ciphertext_matmul_matrix", "3", "4", "2", *threshold], cwd=tmp_path, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    assert "agree: yes" in r.stdout, r.stdout
    opened = {flow: int(cnt) for flow, cnt in re.findall(r"(element|matrix) flow: decrypted_elements (\d+)", r.stdout)}
    assert opened == {"element": 48, "matrix": 20}, r.stdout
