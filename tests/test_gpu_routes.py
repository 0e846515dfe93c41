"""GPU: every size-dependent launch route of the public entry points, on both sides of the size where the launcher's choice
changes, checked against the C++/GMP oracle (or against known plaintexts).  Each test turns on the "profile_kernels" option
and asserts the launch counts of the spans named after the kernel builds the call launched (include/cofhe_hip.h), so that
a threshold moved by one fails a test instead of quietly taking a path nobody checks."""
import functools

import pytest

import oracle_lib as O
from conftest import load_json
from gpu_inputs import (P, _device_status_stays_clear, _pt_bytes, _random_tensor, _records_of, encrypt_tensor_gpu, engine,  # noqa: F401
                        exp_records, form_record, hx)
from lopsided import lopsided_pool

pytestmark = pytest.mark.gpu

SPANS = ("k_compose_wg3", "k_compose_wg", "k_add_ct3", "k_add_ct", "k_pow_shared_pair", "k_pow_shared_wide", "k_pow_shared_solo",
         "k_pow_shared", "k_spread_records", "k_decrypt3", "k_decrypt", "k_tree_level", "k_scal_matmul_wnaf", "k_scal_matmul_wnaf3",
         "k_pow_table", "k_pow_table3")
X3_LIMIT = 3 * 256 * 32          # compositions of the largest grid the three-per-CU builds take: 768 workgroups of 32


def _launches(E):
    """launches of every route witness since the last call (names with none left out); the spans are then dropped"""
    got = {k: E.profile_read(k)[1] for k in SPANS}
    E.profile_read(SPANS[0], clear=True)
    return {k: v for k, v in got.items() if v}


@pytest.fixture
def E(params128):
    """the k = 128 context with profiling on; every option a test pins is reset afterwards"""
    eng = engine(hx(params128["delta"]))
    eng.set_option("profile_kernels", 1)
    _launches(eng)
    yield eng
    for name, v in (("profile_kernels", 0), ("matmul_tree", -1), ("matmul_segments", 0), ("wnaf_width", 0), ("ladder_form", 0)):
        eng.set_option(name, v)
    eng.profile_read(SPANS[0], clear=True)


def _dev(arr):
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).cuda()


def _host(t):
    import numpy as np
    return t.cpu().numpy().view(np.uint32).reshape(-1)


def _matmul(E, cts, ex, zero, n, m, p):
    import torch
    out = torch.zeros(n * p * 336, dtype=torch.int32, device="cuda")
    E.scal_matmul_records(cts.data_ptr(), ex.data_ptr(), zero.data_ptr(), out.data_ptr(), n, m, p)
    torch.cuda.synchronize()
    return out


def _oracle_outputs_match(E, d, cts_of, exp_of, zero_l, out, m, p, rows, cols):
    """outputs (i, k), i in rows, k in cols, of an n x m . m x p product against O.scal_2d on just those rows and columns;
    cts_of(i, j): the ciphertext at (i, j), exp_of(j, k): the exponent at (j, k)"""
    import torch
    sub_cts = [cts_of(i, j) for i in rows for j in range(m)]
    sub_s = _pt_bytes([m, len(cols)], [exp_of(j, k) for j in range(m) for k in cols])
    want = O.scal_2d(d, sub_s, P.serialize_ciphertext_tensor([len(rows), m], sub_cts), P.serialize_ciphertext_tensor([1], zero_l))
    o = out.view(-1, p, 336)
    got = torch.stack([o[i, k] for i in rows for k in cols])
    return E.records_to_bytes(_host(got), [len(rows), len(cols)]) == want


# ---- 1. the product tree's top-level index (op word: 21 bits) -------------------------------------------------------------------

def _nafs_at_every_position(p, seed):
    """exponent records of an 8 x p matrix: row 0 = 0x5555...5, row 1 = 0xAAAA...A (128 bits; between them a NAF digit at every
    position 0..127), rows 2..7 random below 2^125 -- so the longest recoding is 128 digits and every (position, column) segment
    of every column is non-empty: with the width pinned to 2 the tree's top level has exactly 128 p elements"""
    import numpy as np
    rng = np.random.default_rng(seed)
    ex = np.zeros((8, p, 32), dtype=np.uint32)
    ex[0, :, :4] = 0x55555555
    ex[1, :, :4] = 0xAAAAAAAA
    ex[2:, :, :4] = rng.integers(0, 1 << 32, size=(6, p, 4), dtype=np.uint64).astype(np.uint32)
    ex[2:, :, 3] &= 0x1FFFFFFF
    return ex


def _exp_int(ex, j, k):
    w = ex[j, k]
    v = int.from_bytes(w[:31].tobytes(), "little")
    return -v if w[31] else v


@pytest.mark.parametrize("p", [16384, 16385])
def test_tree_top_level_index_at_2_to_21(E, params128, p):
    """1 x 8 . 8 x p with a non-zero digit at every bit position of every column (width 2): the tree's top level has N_T = 128 p
    elements.  p = 16384: the largest index is 2^21 - 1 and the tree runs; p = 16385: index 2^21 would not fit the Horner op word,
    so the chains run -- by default and with "matmul_tree" = 1 alike.  Full: the whole output against the chains
    ("matmul_tree" = 0); sampled: 11 columns against the oracle, among them 16256..16384, whose top positions carry the indices
    >= 2^21 (column k of position 127 has index 127 p + k)"""
    d = hx(params128["delta"])
    n, m = 1, 8
    cts_l = _random_tensor(d, n * m, 3100 + p, nbase=8)
    zero_l = _random_tensor(d, 1, 3101, nbase=2)
    cts, zero = _dev(_records_of(E, cts_l)), _dev(_records_of(E, zero_l))
    ex_np = _nafs_at_every_position(p, p)
    ex = _dev(ex_np.reshape(-1))
    E.set_option("wnaf_width", 2)
    got = _matmul(E, cts, ex, zero, n, m, p)
    routes = _launches(E)
    E.set_option("matmul_tree", 0)
    chains = _matmul(E, cts, ex, zero, n, m, p)
    routes_chains = _launches(E)
    import torch
    assert torch.equal(got, chains)
    cols = sorted({0, 1, 4097, p // 2, 16255, 16256, 16257, 16300, 16383, p - 2, p - 1})
    assert _oracle_outputs_match(E, d, lambda i, j: cts_l[i * m + j], lambda j, k: _exp_int(ex_np, j, k), zero_l, got, m, p, [0], cols)
    assert "k_tree_level" not in routes_chains and routes_chains["k_scal_matmul_wnaf"] == 1
    assert routes["k_scal_matmul_wnaf"] == 1
    if p == 16384:
        assert routes.get("k_tree_level", 0) >= 1, routes
    else:
        assert "k_tree_level" not in routes, routes
        E.set_option("matmul_tree", 1)                   # pinned: the tree only where its encoding allows
        pinned = _matmul(E, cts, ex, zero, n, m, p)
        routes_pinned = _launches(E)
        assert torch.equal(pinned, chains)
        assert "k_tree_level" not in routes_pinned and routes_pinned["k_scal_matmul_wnaf"] == 1


def test_tree_top_level_index_default_route_992_bit_exponents(E, params128):
    """the default route at 1 x 8 . 8 x 4096 with random 992-bit exponents and the automatic width (8): ~2.5 M non-empty
    (position, column) segments, beyond the op word's 2^21 -- the launcher must leave the tree for the chains.  Full: the whole
    output against "matmul_tree" = 0; sampled: 6 columns against the oracle"""
    import numpy as np
    import torch
    d = hx(params128["delta"])
    n, m, p = 1, 8, 4096
    cts_l = _random_tensor(d, n * m, 3200, nbase=8)
    zero_l = _random_tensor(d, 1, 3201, nbase=2)
    cts, zero = _dev(_records_of(E, cts_l)), _dev(_records_of(E, zero_l))
    rng = np.random.default_rng(3202)
    ex_np = np.zeros((m, p, 32), dtype=np.uint32)
    ex_np[:, :, :31] = rng.integers(0, 1 << 32, size=(m, p, 31), dtype=np.uint64).astype(np.uint32)
    ex_np[:, :, 30] |= 0x80000000                        # every exponent exactly 992 bits long
    ex_np[:, 1::2, 31] = 1                               # odd columns negative
    ex = _dev(ex_np.reshape(-1))
    got = _matmul(E, cts, ex, zero, n, m, p)
    routes = _launches(E)
    E.set_option("matmul_tree", 0)
    chains = _matmul(E, cts, ex, zero, n, m, p)
    assert torch.equal(got, chains)
    cols = [0, 1, 2048, 4093, 4094, 4095]
    assert _oracle_outputs_match(E, d, lambda i, j: cts_l[i * m + j], lambda j, k: _exp_int(ex_np, j, k), zero_l, got, m, p, [0], cols)
    assert "k_tree_level" not in routes and routes["k_scal_matmul_wnaf"] == 1, routes


# ---- 2. ciphertext addition: one launch, the pair, one launch ---------------------------------------------------------------

ADD_CASES = ("shared+shared", "shared+mixed", "mixed+shared", "first+shared", "last+shared", "mixed+mixed")


@pytest.mark.parametrize("n_ct,want,oracle_case", [
    (12288, {"k_add_ct3": 1}, "last+shared"),                    # 768 workgroups of 2 n compositions: k_add_ct3 alone
    (12289, {"k_add_ct3": 1, "k_add_ct": 1}, "mixed+shared"),    # 769: the pair (folded grid 385)
    (16384, {"k_add_ct3": 1, "k_add_ct": 1}, "shared+shared"),   # the 128 x 128 headline shape
    (24575, {"k_add_ct3": 1, "k_add_ct": 1}, "first+shared"),    # folded grid n + 1 = 24576: 768, the pair's last size
    (24576, {"k_add_ct": 1}, "shared+mixed"),                    # folded grid 769: k_add_ct alone
])
def test_add_ciphertext_records_routes(E, params128, n_ct, want, oracle_case):
    """cofhe_hip_add_ciphertext_records at the sizes where its launches change, for both operands sharing their c1, one of
    them mixed, one differing c1 in the first / last ciphertext, and both mixed; out of place and in place (out == a).  Full:
    every case and both uses against cofhe_hip_compose_records over the 2 n records, and one case per size against the
    oracle's add on the whole tensor"""
    import torch
    d = hx(params128["delta"])
    forms = _dev(_records_of(E, _random_tensor(d, 48, 3300, nbase=32))).view(96, 168)
    g = torch.Generator(device="cuda").manual_seed(n_ct)
    rnd = lambda: torch.randint(0, 96, (n_ct,), device="cuda", generator=g)
    one = lambda i: torch.full((n_ct,), i, dtype=torch.int64, device="cuda")
    c1 = {"shared": one(5), "mixed": rnd(), "first": one(5), "last": one(5)}
    c1["first"][0] = 7
    c1["last"][n_ct - 1] = 7
    shared_b = one(11)

    def tensor(c1_idx, c2_idx):
        return torch.stack([forms[c1_idx], forms[c2_idx]], 1).reshape(-1).contiguous()
    for case in ADD_CASES:
        ka, kb = case.split("+")
        a = tensor(c1[ka], rnd())
        b = tensor(shared_b if kb == "shared" else c1["mixed"].roll(1), rnd())
        want_t = torch.empty_like(a)
        E.compose_records(a.data_ptr(), b.data_ptr(), want_t.data_ptr(), 2 * n_ct)
        torch.cuda.synchronize()
        _launches(E)
        got = torch.zeros_like(a)
        E.add_ciphertext_records(a.data_ptr(), b.data_ptr(), got.data_ptr(), n_ct)
        torch.cuda.synchronize()
        assert torch.equal(got, want_t), case
        assert _launches(E) == want, case
        a2 = a.clone()
        E.add_ciphertext_records(a2.data_ptr(), b.data_ptr(), a2.data_ptr(), n_ct)
        torch.cuda.synchronize()
        assert torch.equal(a2, want_t), case + " in place"
        assert _launches(E) == want, case
        if case == oracle_case:
            to_b = lambda t: E.records_to_bytes(_host(t), [n_ct])
            assert to_b(got) == O.add(d, to_b(a), to_b(b)), case
    assert E.device_status(clear=False) == 0


# ---- 3. the shared-exponent ladders of decryption ---------------------------------------------------------------------------

def _encrypted(E, prm, n, n_r, seed, odd=None):
    """n ciphertexts, ciphertext i from the encryption with randomness r_(i mod n_r) (so n_r distinct c1); odd = 0 or n - 1
    replaces that one ciphertext by one of another encryption.  Returns the device tensor and the plaintexts"""
    import torch
    rng = P.SplitMix64(seed)
    k = prm["k"]
    per = (n + n_r - 1) // n_r
    ms = [[rng.bits(k) for _ in range(per)] for _ in range(n_r)]
    ts = [encrypt_tensor_gpu(E, torch, prm, ms[q], rng.bits(900), torch.device("cuda", 0)).view(per, 336) for q in range(n_r)]
    cts = torch.stack(ts, 1).reshape(per * n_r, 336)[:n].contiguous()
    plains = [ms[i % n_r][i // n_r] for i in range(n)]
    if odd is not None:
        x = rng.bits(k)
        cts[odd] = encrypt_tensor_gpu(E, torch, prm, [x], rng.bits(900), torch.device("cuda", 0))
        plains[odd] = x
    return cts.reshape(-1).contiguous(), plains


def _c1_pow_oracle(E, d, cts, n, e):
    """partial-decryption tensor bytes c1_i^e from the oracle, one ladder per distinct c1"""
    import numpy as np
    c1 = _host(cts).reshape(n, 2, 168)[:, 0]
    uniq, inv = np.unique(c1, axis=0, return_inverse=True)
    pairs = np.stack([uniq, uniq], 1).reshape(-1)
    got = O.scal_1d(d, _pt_bytes([len(uniq)], [e] * len(uniq)), E.records_to_bytes(pairs, [len(uniq)]))
    _, wcts = P.deserialize_ciphertext_tensor(got)
    return P.serialize_form_tensor([n], [wcts[u][0] for u in np.asarray(inv).reshape(-1)])


def _plaintexts(pt, n, k):
    import numpy as np
    ow = (k + 31) // 32 + 1
    a = pt.cpu().numpy().view(np.uint32).reshape(n, ow)
    assert not a[:, -1].any()
    return [int.from_bytes(a[i, :-1].tobytes(), "little") for i in range(n)]


@pytest.mark.parametrize("n,kind,form,want", [
    (63, "shared", 0, {"k_pow_shared_pair": 1}),                              # below 64: no search for a shared c1, 63 ladders
    (64, "shared", 0, {"k_pow_shared_pair": 1, "k_spread_records": 1}),       # one ladder, copied
    (64, "first", 0, {"k_pow_shared_pair": 1}),                               # one differing c1: 64 ladders
    (64, "last", 0, {"k_pow_shared_pair": 1}),
    (4096, "first", 0, {"k_pow_shared": 1}),                                  # 4096 ladders: the throughput kernel
    (4096, "last", 0, {"k_pow_shared": 1}),
    (256, "mixed", 0, {"k_pow_shared_pair": 1}),                              # the pair at full capacity: 512 workgroups
    (257, "mixed", 0, {"k_pow_shared": 1}),
    (257, "mixed", 1, {"k_pow_shared_wide": 1}),                              # the pair pinned beyond its limit: form 4
])
def test_decryption_ladder_routes(E, params128, n, kind, form, want):
    """decrypt_records and part_decrypt_records (pow_shared_c1 / pow_shared) at the edges of the shared-c1 search (n >= 64)
    and of the two-workgroup pair ladder (n <= 256), on tensors made of interleaved encryptions with 4 different r, of one,
    or of one with a single other ciphertext first or last.  Full: every part-decryption byte for byte against the oracle's
    c1^sk (one oracle ladder per distinct c1) and every decrypted plaintext against the one encrypted"""
    import torch
    prm = params128
    d, k, sk = hx(prm["delta"]), prm["k"], hx(prm["sk"])
    odd = {"first": 0, "last": n - 1}.get(kind)
    cts, plains = _encrypted(E, prm, n, 4 if kind == "mixed" else 1, 3400 + n, odd)
    dsk = _dev(exp_records([sk]))
    frec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    E.set_option("ladder_form", form)
    _launches(E)
    part = torch.zeros(n * 168, dtype=torch.int32, device="cuda")
    E.part_decrypt_records(cts.data_ptr(), dsk.data_ptr(), part.data_ptr(), n)
    torch.cuda.synchronize()
    assert _launches(E) == want
    pt = torch.zeros(n * ((k + 31) // 32 + 1), dtype=torch.int32, device="cuda")
    E.decrypt_records(cts.data_ptr(), dsk.data_ptr(), frec, pt.data_ptr(), n, k)
    torch.cuda.synchronize()
    assert _launches(E) == dict(want, k_decrypt3=1)
    assert E.pdr_records_to_bytes(_host(part), [n]) == _c1_pow_oracle(E, d, cts, n, sk)
    assert _plaintexts(pt, n, k) == plains


# ---- 4. the three-per-CU builds against the plain ones at 768 / 769 workgroups ------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _boundary_forms(name):
    prm = load_json("params_%s.json" % name)
    d, k = hx(prm["delta"]), prm["k"]
    f = P.Form(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    pool = lopsided_pool(d, k, f)
    rng = P.SplitMix64(3500)
    return pool + [P.inverse(x) for x in pool] + [P.random_form(d, rng) for _ in range(64)]


@pytest.mark.parametrize("n,want", [(X3_LIMIT, "k_compose_wg3"), (X3_LIMIT + 1, "k_compose_wg")])
def test_compose_records_build_boundary(E, params128, n, want):
    """compose_records on 768 x 32 and 768 x 32 + 1 records (the last workgroup of the second holds one composition): pairs
    drawn from the lopsided pool, its inverses and random forms, in both orders.  Full: the whole output against the oracle
    (one padding pair appended on the host to make whole ciphertexts), and a o b == b o a on the device"""
    import numpy as np
    import torch
    d = hx(params128["delta"])
    forms = _boundary_forms("s128_k128")
    recs = _dev(np.stack([form_record(x.a, x.b, x.c) for x in forms])).view(len(forms), 168)
    g = torch.Generator(device="cuda").manual_seed(n)
    a = recs[torch.randint(0, len(forms), (n,), device="cuda", generator=g)].reshape(-1).contiguous()
    b = recs[torch.randint(0, len(forms), (n,), device="cuda", generator=g)].reshape(-1).contiguous()
    ab, ba = torch.zeros_like(a), torch.zeros_like(a)
    E.compose_records(a.data_ptr(), b.data_ptr(), ab.data_ptr(), n)
    E.compose_records(b.data_ptr(), a.data_ptr(), ba.data_ptr(), n)
    torch.cuda.synchronize()
    assert _launches(E) == {want: 2}
    assert torch.equal(ab, ba)
    pad = lambda t: np.concatenate([_host(t), _host(recs[len(forms) - 1])]) if n % 2 else _host(t)
    nct = (n + 1) // 2
    want_b = O.add(d, E.records_to_bytes(pad(a), [nct]), E.records_to_bytes(pad(b), [nct]))
    _, want_r = E.bytes_to_records(want_b)
    assert np.array_equal(_host(ab), want_r[: n * 168])


@pytest.mark.parametrize("n_ct,want", [(X3_LIMIT, "k_decrypt3"), (X3_LIMIT + 1, "k_decrypt")])
def test_decrypt_and_combine_build_boundary(E, n_ct, want):
    """decrypt_records and combine_part_decryptions_records at 768 x 32 and 768 x 32 + 1 ciphertexts (one workgroup of 32
    decryptions each): interleaved encryptions with 4 different r, partial decryptions with the golden threshold shares (t = 2,
    lambda = +1 / -1).  Full: every plaintext against the one encrypted"""
    import torch
    prm, th = load_json("params_s128_k128.json"), load_json("threshold_s128_k128.json")
    k = prm["k"]
    cts, plains = _encrypted(E, prm, n_ct, 4, 3600 + n_ct)
    dsk = _dev(exp_records([hx(prm["sk"])]))
    frec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    ow = (k + 31) // 32 + 1
    _launches(E)
    pt = torch.zeros(n_ct * ow, dtype=torch.int32, device="cuda")
    E.decrypt_records(cts.data_ptr(), dsk.data_ptr(), frec, pt.data_ptr(), n_ct, k)
    torch.cuda.synchronize()
    assert _launches(E) == {"k_pow_shared": 1, want: 1}
    assert _plaintexts(pt, n_ct, k) == plains
    case = th["cases"][0]
    parts = torch.zeros(len(case["used_shares"]) * n_ct * 168, dtype=torch.int32, device="cuda")
    for i, sh in enumerate(case["used_shares"]):
        dsh = _dev(exp_records([hx(sh)]))
        E.part_decrypt_records(cts.data_ptr(), dsh.data_ptr(), parts.data_ptr() + i * n_ct * 168 * 4, n_ct)
        torch.cuda.synchronize()
    _launches(E)
    pt2 = torch.zeros_like(pt)
    E.combine_part_decryptions_records(cts.data_ptr(), parts.data_ptr(), case["lambda"], frec, pt2.data_ptr(), n_ct, k)
    torch.cuda.synchronize()
    assert _launches(E) == {want: 1}
    assert _plaintexts(pt2, n_ct, k) == plains


@pytest.mark.parametrize("n,m,p,w,want", [
    (96, 2, 128, 2, {"k_scal_matmul_wnaf": 1, "k_scal_matmul_wnaf3": 1}),      # chain grid 2 n p / 32 = 768
    (7, 2, 1756, 2, {"k_scal_matmul_wnaf": 1}),                                # 24 584 chains: 769
    (96, 128, 1, 3, {"k_pow_table": 1, "k_pow_table3": 1, "k_scal_matmul_wnaf": 1, "k_scal_matmul_wnaf3": 1}),   # table grid 2 n m / 32 = 768
    (100, 123, 1, 3, {"k_pow_table": 1, "k_scal_matmul_wnaf": 1, "k_scal_matmul_wnaf3": 1}),                      # 24 600 bases: 769
])
def test_scal_matmul_chain_build_boundary(E, params128, n, m, p, w, want):
    """the chain form ("matmul_tree" = 0, one segment) with its k_scal_matmul_wnaf grid, or its k_pow_table grid (width pinned
    to 3, so a table is built), at 768 and 769 workgroups.  Sampled against the oracle: the outputs of the last workgroup
    (last row, last 16 columns), rows 0 and n / 2, columns 0, 1 and p / 2"""
    import torch
    d = hx(params128["delta"])
    pool_cts = _random_tensor(d, 48, 3700, nbase=24)
    pool = _dev(_records_of(E, pool_cts)).view(48, 336)
    rng = P.SplitMix64(3701 + n)
    idx = [rng.below(48) for _ in range(n * m)]
    cts = pool[torch.tensor(idx, device="cuda")].reshape(-1).contiguous()
    special = [0, 1, -1, 3, -5, 255, -(1 << 12) + 7, (1 << 16) - 1]
    exps = [special[t % len(special)] if t % 3 == 0 else rng.bits(12) - (1 << 11) for t in range(m * p)]
    ex = _dev(exp_records(exps))
    zero_l = _random_tensor(d, 1, 3702, nbase=2)
    zero = _dev(_records_of(E, zero_l))
    E.set_option("matmul_tree", 0)
    E.set_option("matmul_segments", 1)
    E.set_option("wnaf_width", w)
    out = _matmul(E, cts, ex, zero, n, m, p)
    assert _launches(E) == want
    rows = sorted({0, n // 2, n - 1})
    cols = sorted(k for k in {0, 1, p // 2} | set(range(max(0, p - 16), p)) if k < p)
    for r in rows:                                      # one oracle call per row: each samples the columns of that row
        assert _oracle_outputs_match(E, d, lambda i, j: pool_cts[idx[i * m + j]], lambda j, k: exps[j * p + k], zero_l, out, m, p,
                                     [r], cols), r
