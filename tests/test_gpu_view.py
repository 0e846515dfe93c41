"""GPU: rearranging resident tensors (cofhe_amd/csrc/view.hip): k_view_records on every case of view_cases at the three record
sizes and both access widths, byte for byte against the Python reference with the destination pre-filled and guarded; the
grid-stride loops; k_gather_records with its sentinels and its status bit; the refusals; real ciphertexts through decryption;
and the bytes entry composed in Engine."""
import numpy as np
import pytest

import view_cases as VC
from conftest import load_json
from gpu_inputs import P, _device_status_stays_clear, engine  # noqa: F401
from test_gpu_fresh_randomness import decrypt, dev, fresh, host, setup

pytestmark = pytest.mark.gpu
EINVAL = -1
CT, FORM, EXP = 336, 168, 32                 # words of a ciphertext, of a form or a partial decryption, of an exponent record
SENT = 0xA5A5A5A5
GUARD = 64                                   # words behind every destination


@pytest.fixture(scope="module")
def tiny():
    return load_json("params_tiny_k8.json")


@pytest.fixture()
def E(tiny):
    """the engine with its kernels' spans on, and every option this file pins back at automatic afterwards"""
    eng = engine(setup(tiny)[0])
    eng.set_option("profile_kernels", 1)
    for name in ("k_view_records", "k_gather_records"):
        eng.profile_read(name, clear=True)
    try:
        yield eng
    finally:
        eng.set_option("view_grid_blocks", 0)
        eng.set_option("profile_kernels", 0)
        eng.profile_read("k_view_records", clear=True)


def rows(rng, n, words):
    """n records of random words, none of them the sentinel"""
    r = rng.integers(0, 1 << 32, size=(n, words), dtype=np.uint64).astype(np.uint32)
    r[r == SENT] = 0
    return r


class Buf:
    """device words that start `shift` words beyond a 16-byte boundary, GUARD sentinel words behind them"""

    def __init__(self, torch, words, shift):
        arr = np.concatenate([np.full(shift, SENT, np.uint32), np.asarray(words, np.uint32).reshape(-1), np.full(GUARD, SENT, np.uint32)])
        self.t, self.shift, self.n = dev(torch, arr), shift, arr.size - shift - GUARD
        assert self.t.data_ptr() % 16 == 0
        self.ptr = self.t.data_ptr() + 4 * shift

    def words(self):
        """the payload, after checking that nothing around it changed"""
        h = host(self.t)
        assert (h[:self.shift] == SENT).all() and (h[self.shift + self.n:] == SENT).all()
        return h[self.shift:self.shift + self.n]


def run_views(E, torch, views, words, shift, seed):
    """every view of a case from a random source of its own into ONE destination: (the destination's words, the reference's,
    the calls that had a box to write)"""
    rng = np.random.default_rng(seed)
    n_dst = VC.count(views[0].dst_extent)
    fill = rows(rng, 1, words)
    dfill = Buf(torch, fill, shift)
    dst = Buf(torch, np.full(n_dst * words, SENT, np.uint32), shift)
    want = [np.full(words, SENT, np.uint32)] * n_dst
    launches = 0
    for v in views:
        src = rows(rng, VC.count(v.src_extent), words)
        dsrc = Buf(torch, src, shift)
        E.view_records(VC.to_c(v), dsrc.ptr, dfill.ptr, dst.ptr, words)
        VC.apply(v, list(src), fill[0], want)
        launches += VC.count(v.out_extent) > 0
        torch.cuda.synchronize()
        assert np.array_equal(dsrc.words().reshape(src.shape), src)
    want = np.concatenate(want) if want else np.zeros(0, np.uint32)
    return dst.words(), want, launches


@pytest.mark.parametrize("shift", [0, 1], ids=["vec16", "dword"])
@pytest.mark.parametrize("words", [CT, FORM, EXP])
@pytest.mark.parametrize("name,views", VC.CASES, ids=VC.CASE_IDS)
def test_every_case_byte_for_byte(E, name, views, words, shift):
    """the box equals the reference and holds no sentinel word (every word of it was written); the destination outside the box,
    the words before the shifted pointers and the guard words behind every buffer are untouched; the status word stays 0; one
    launch per call under "k_view_records", none for an empty box"""
    import torch
    got, want, launches = run_views(E, torch, views, words, shift, seed=words + shift)
    assert np.array_equal(got, want)
    inside = np.zeros(VC.count(views[0].dst_extent), bool)
    for v in views:
        for _, d in VC.indices(v):
            inside[d] = True
    g = got.reshape(-1, words)
    assert not (g[inside] == SENT).any() and (g[~inside] == SENT).all()
    assert E.device_status(clear=False) == 0
    assert E.profile_read("k_view_records", clear=True)[1] == launches


@pytest.mark.parametrize("words,shift", [(CT, 0), (CT, 1), (EXP, 0)])
def test_the_grid_stride_loop(E, words, shift):
    """"view_grid_blocks" = 3: a [40, 25] transpose has 1000 records, three workgroups hold 12 (a wavefront each) or 96 (eight
    lanes each) in one pass"""
    import torch
    E.set_option("view_grid_blocks", 3)
    got, want, launches = run_views(E, torch, [VC.permute([40, 25], [1, 0])], words, shift, seed=3)
    assert np.array_equal(got, want) and not (got == SENT).any()
    assert E.profile_read("k_view_records", clear=True)[1] == launches == 1


GATHER_INDEX = [3, 0, 10, VC.GATHER_FILL, 7, 7, VC.GATHER_KEEP, 11, 1, 0xFFFFFFFD, 2, 9, VC.GATHER_KEEP, 4, 5, 6, 8, 10, 10, 0,
                VC.GATHER_FILL, 3, 2, 1, 0, 9, 8, 7, 6, 5, 4, VC.GATHER_KEEP, 3, 0, 10, 1, 2]


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("words,shift", [(CT, 0), (CT, 1), (FORM, 0), (EXP, 0), (EXP, 1)])
def test_gather(E, words, shift, blocks):
    """37 indices over 11 source records with FILL, KEEP, repeated indices and the bad indices 11 and 0xFFFFFFFD: bytes against
    the reference, KEEP positions keep the sentinel, the bad indices give the fill record and status bit 32, which the read
    clears; with no fill record the bad indices (and FILL) leave the destination alone and the bit is still set"""
    import torch
    assert len(GATHER_INDEX) == 37 and 11 in GATHER_INDEX and 0xFFFFFFFD in GATHER_INDEX
    E.set_option("view_grid_blocks", blocks)
    rng = np.random.default_rng(words + shift)
    src, fill = rows(rng, 11, words), rows(rng, 1, words)
    dsrc, dfill, dix = Buf(torch, src, shift), Buf(torch, fill, shift), Buf(torch, np.array(GATHER_INDEX, np.uint32), 0)
    for fill_ptr, fill_row in ((dfill.ptr, fill[0]), (0, None)):
        dst = Buf(torch, np.full(37 * words, SENT, np.uint32), shift)
        E.gather_records(dsrc.ptr, 11, dix.ptr, fill_ptr, dst.ptr, 37, words)
        torch.cuda.synchronize()
        want, bad = VC.gather(list(src), GATHER_INDEX, fill_row, [np.full(words, SENT, np.uint32)] * 37)
        assert bad
        got = dst.words().reshape(37, words)
        assert np.array_equal(got, np.stack(want))
        kept = [i for i, ix in enumerate(GATHER_INDEX) if ix == VC.GATHER_KEEP or (fill_row is None and ix >= 11)]
        assert len(kept) == (3 if fill_row is not None else 7) and (got[kept] == SENT).all()
        assert not (np.delete(got, kept, axis=0) == SENT).any()
        assert E.device_status(clear=True) == 32
        assert E.device_status(clear=True) == 0
    assert E.profile_read("k_gather_records", clear=True)[1] == 2
    # without a bad index the status word stays clear
    good = np.array([ix for ix in GATHER_INDEX if ix < 11 or ix >= VC.GATHER_KEEP], np.uint32)
    dst = Buf(torch, np.full(good.size * words, SENT, np.uint32), shift)
    E.gather_records(dsrc.ptr, 11, Buf(torch, good, 0).ptr, dfill.ptr, dst.ptr, good.size, words)
    torch.cuda.synchronize()
    want, bad = VC.gather(list(src), [int(i) for i in good], fill[0], [np.full(words, SENT, np.uint32)] * good.size)
    assert not bad and np.array_equal(dst.words().reshape(-1, words), np.stack(want))
    assert E.device_status(clear=False) == 0


def test_refusals_leave_the_destination_alone(E):
    """COFHE_HIP_EINVAL, nothing written, nothing launched: a fill is needed and there is none; words = 0; the destination overlaps
    the source or the fill; a descriptor that view_check refuses.  An empty box and an empty gather return at once."""
    import torch
    from cofhe_amd import CofheHipError
    rng = np.random.default_rng(1)
    src, fill = rows(rng, 12, CT), rows(rng, 1, CT)
    dsrc, dfill = Buf(torch, src, 0), Buf(torch, fill, 0)
    dst = Buf(torch, np.full(35 * CT, SENT, np.uint32), 0)
    dix = Buf(torch, np.arange(12, dtype=np.uint32), 0)
    pad, same = VC.to_c(VC.pad([3, 4], [1, 2], [1, 1])), VC.to_c(VC.identity([12]))
    nine = VC.to_c(VC.identity([12]))
    nine.out_ndim = 9
    outside = VC.to_c(VC.identity([12]))
    outside.dst_start[0] = 1
    wrap = VC.to_c(VC.identity([12]))
    wrap.start[0], wrap.map[0][0], wrap.out_extent[0], wrap.dst_extent[0] = 2 ** 62, 2 ** 31 - 1, 2 ** 32, 2 ** 32
    calls = [lambda: E.view_records(pad, dsrc.ptr, 0, dst.ptr, CT),
             lambda: E.view_records(same, dsrc.ptr, dfill.ptr, dst.ptr, 0),
             lambda: E.view_records(same, dsrc.ptr, dfill.ptr, dsrc.ptr, CT),
             lambda: E.view_records(same, dsrc.ptr, dfill.ptr, dsrc.ptr + 11 * CT * 4 + 4, CT),
             lambda: E.view_records(same, dsrc.ptr, dfill.ptr, dsrc.ptr - 12 * CT * 4 + 4, CT),
             lambda: E.view_records(same, dsrc.ptr, dst.ptr + 4, dst.ptr, CT),
             lambda: E.view_records(nine, dsrc.ptr, dfill.ptr, dst.ptr, CT),
             lambda: E.view_records(outside, dsrc.ptr, dfill.ptr, dst.ptr, CT),
             lambda: E.view_records(wrap, dsrc.ptr, dfill.ptr, dst.ptr, CT),
             lambda: E.gather_records(dsrc.ptr, 12, dix.ptr, dfill.ptr, dst.ptr, 12, 0),
             lambda: E.gather_records(dsrc.ptr, 12, dix.ptr, dfill.ptr, dsrc.ptr + 4, 12, CT),
             lambda: E.gather_records(dsrc.ptr, 12, dix.ptr, dst.ptr + 8, dst.ptr, 12, CT),
             lambda: E.gather_records(dsrc.ptr, 12, dst.ptr + 40, dfill.ptr, dst.ptr, 12, CT),
             lambda: E.gather_records(dsrc.ptr, 0xFFFFFFFF, dix.ptr, dfill.ptr, dst.ptr, 12, CT)]
    for i, call in enumerate(calls):
        with pytest.raises(CofheHipError) as ei:
            call()
        assert ei.value.code == EINVAL, i
    E.view_records(VC.to_c(dict(VC.CASES)["empty"][0]), dsrc.ptr, 0, dst.ptr, CT)              # n_box = 0: nothing to do
    E.view_records(VC.to_c(dict(VC.CASES)["empty"][0]), 0, 0, 0, CT)
    E.gather_records(0, 0, 0, 0, 0, 0, CT)
    torch.cuda.synchronize()
    assert (dst.words() == SENT).all() and np.array_equal(dsrc.words().reshape(src.shape), src)
    assert E.profile_read("k_view_records")[1] == 0 and E.profile_read("k_gather_records", clear=True)[1] == 0


def test_through_real_ciphertexts(E, tiny):
    """[1, 4, 3, 2] with value i at element i, the fill an encryption of 99: window taps, a permutation and a padding decrypt to the
    reference applied to the plaintext array"""
    import torch
    import random
    d, k, forms, recs, bound = setup(tiny)
    rng = random.Random(8)
    ms = list(range(24)) + [99]
    cts = fresh(E, torch, recs, ms, [rng.randrange(1, bound) for _ in ms], k)
    assert decrypt(E, torch, tiny, cts, 25, k) == ms
    src, fill = cts[:24 * CT], cts[24 * CT:].clone()
    for v in (VC.window_taps(1, 4, 3, 2, 2, 2, sh=1, sw=2, ph=1, pw=1), VC.permute([1, 4, 3, 2], [3, 2, 0, 1]),
              VC.pad([1, 4, 3, 2], [0, 1, 0, 1], [0, 0, 2, 0])):
        n = VC.count(v.out_extent)
        out = torch.zeros(n * CT, dtype=torch.int32, device="cuda")
        E.view_records(VC.to_c(v), src.data_ptr(), fill.data_ptr(), out.data_ptr(), CT)
        torch.cuda.synchronize()
        want = VC.apply(v, ms[:24], 99, [None] * n)
        assert 99 in want or v.out_extent == [2, 3, 1, 4]
        assert decrypt(E, torch, tiny, out, n, k) == want


def test_view_tensor_bytes(E, tiny):
    """a serialised [2, 3] tensor in, the serialised [3, 2] transpose out: records_to_bytes of the reference rows; a padded view
    with a serialised fill; a tensor of another shape, a view placed in a larger destination and a tensor with an invalid form
    are refused"""
    import torch
    import random
    from cofhe_amd import CofheHipError
    from cofhe_amd import engine as eng
    d, k, forms, recs, bound = setup(tiny)
    rng = random.Random(9)
    cts = host(fresh(E, torch, recs, list(range(7)), [rng.randrange(1, bound) for _ in range(7)], k)).reshape(7, CT)
    data, fill = E.records_to_bytes(cts[:6].reshape(-1), [2, 3]), E.records_to_bytes(cts[6], [1])
    v = VC.permute([2, 3], [1, 0])
    want = np.stack(VC.apply(v, list(cts[:6]), None, [None] * 6))
    assert E.view_tensor_bytes(data, eng.view_permute([2, 3], [1, 0])) == E.records_to_bytes(want.reshape(-1), [3, 2])
    v = VC.pad([2, 3], [1, 0], [0, 1])
    want = np.stack(VC.apply(v, list(cts[:6]), cts[6], [None] * 12))
    assert E.view_tensor_bytes(data, eng.view_pad([2, 3], [1, 0], [0, 1]), fill=fill) == E.records_to_bytes(want.reshape(-1), [3, 4])
    with pytest.raises(CofheHipError):
        E.view_tensor_bytes(data, eng.view_pad([2, 3], [1, 0], [0, 1]))                        # a fill is needed
    with pytest.raises(CofheHipError):
        E.view_tensor_bytes(data, eng.view_permute([3, 2], [1, 0]))                            # another source shape
    with pytest.raises(CofheHipError):
        E.view_tensor_bytes(data, eng.view_into(eng.view_permute([2, 3], [1, 0]), [3, 3], [0, 1]))
    forged = cts[:6].copy()
    forged[4, FORM + 80] += 1                                                                  # c + 1 in c2 of element 4
    with pytest.raises(CofheHipError, match="not a reduced form"):
        E.view_tensor_bytes(E.records_to_bytes(forged.reshape(-1), [2, 3]), eng.view_permute([2, 3], [1, 0]))
    assert E.device_status(clear=False) == 0
