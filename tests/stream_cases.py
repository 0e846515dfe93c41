"""The smallest valid call of every device entry of include/cofhe_hip.h that takes a `stream`, as data: TABLE maps the entry's
name to a builder, VARIANTS names the routes an entry is built for more than once.  A builder returns a Case: the device inputs
(each with a decoy: different, valid data of the same kind and size), the outputs, and call(E, ptrs, stream), which runs the
entry on `stream` reading its device inputs at `ptrs` -- what tests/test_gpu_streams.py needs to run an entry behind other
work on a non-blocking stream.  tests/test_stream_cases_cpu.py holds the table against the header; it imports this module
without a GPU, so everything that needs torch or the library is imported inside env().

Parameter set s128_k128 only, and the smallest sizes the GPU modules use: 2 to 33 elements, m <= 20 for the products,
1 x 4 x 4 x 2 images."""
import random

REC, CT, EXP = 168, 336, 32                  # words of a form record, of a ciphertext, of an exponent record
IMAGE = (1, 4, 4, 2)

# entries with a `stream` parameter that have no case, each with its reason
EXCLUDED = {
    "cofhe_hip_stream_create": "makes the stream; test_gpu_streams.py (g) and every scenario there use it",
    "cofhe_hip_stream_destroy": "ends the stream; test_gpu_streams.py (g)",
    "cofhe_hip_stream_query": "the probe of every scenario of test_gpu_streams.py",
    "cofhe_hip_stream_sync": "the fence of every scenario of test_gpu_streams.py",
    "cofhe_hip_upload": "host memory: no device input to put a decoy in",
    "cofhe_hip_download": "host memory: synchronises and returns the bytes",
    "cofhe_hip_timer_start": "records an event, launches nothing; the holder's duration is measured with it",
    "cofhe_hip_timer_stop": "records an event and waits for it",
    "cofhe_hip_time_compose": "a timing loop around cofhe_hip_compose_records, which has a case",
    "cofhe_hip_all_gather_rows": "needs a communicator; covered by the existing world-of-one test",
}


class Buf:
    """one device input: `t` (int32 words), read as records of `words` words, and `decoy`, valid data of the same kind and size
    that gives another result (default: the input rolled by one record)"""

    def __init__(self, torch, t, words, decoy=None):
        assert t.numel() % words == 0
        self.t, self.words, self.n = t.contiguous(), words, t.numel() // words
        self.decoy = (torch.roll(self.t.view(self.n, words), 1, 0).reshape(-1) if decoy is None else decoy).contiguous()
        assert self.decoy.numel() == self.t.numel() and not torch.equal(self.decoy, self.t)


class Case:
    """inputs: [Buf]; outputs: device tensors the call writes, or an int i for "the buffer passed as input i" (in place);
    call(E, ptrs, stream) -> a host value or None, ptrs[i] the address input i is read at; syncs: the entry is documented to
    synchronise its stream inside; reads_holder: ptrs gets one more address at its end, n_holder form records that the test's
    holder writes on the same stream; no_inputs: nothing on the device to put a decoy in (the call pre-fills its output on
    the stream instead, so that a launch on another stream is overwritten); further keywords: the integers behind the inputs"""

    def __init__(self, inputs, outputs, call, syncs=False, reads_holder=False, no_inputs=False, **meta):
        self.inputs, self.outputs, self.call = inputs, outputs, call
        self.syncs, self.reads_holder, self.no_inputs = syncs, reads_holder, no_inputs
        self.meta = meta                     # the integers behind the inputs, for the tests that check against an oracle


_env = {}


def env(prm):
    """what the builders share, made once: the parameter set, the form pool of test_gpu_affine, the cached engine"""
    if "v" not in _env:
        import numpy as np
        import torch
        import view_cases as VC
        from gpu_inputs import P, engine, exp_records, form_record
        from test_gpu_affine import NPOOL, pool, tensor
        from test_gpu_fresh_randomness import dev, fresh, setup

        class V:
            pass
        v = V()
        v.np, v.torch, v.VC, v.P, v.prm = np, torch, VC, P, prm
        v.d, v.k, v.forms, v.recs, v.bound = setup(prm)
        v.E = engine(v.d)
        v.fw, v.inv = pool(torch, v.d, v.k, v.forms["f"])
        v.npool = NPOOL - 2                                  # the random forms; the two boundary forms stay out
        v.dev = lambda arr: dev(torch, arr)
        v.exp_records, v.form_record, v.tensor, v.fresh = exp_records, form_record, tensor, fresh
        _env["v"] = v
    return _env["v"]


# ---- what the builders are made of ------------------------------------------------------------------------------------------

def _idx(v, n, seed, distinct=False):
    rng = random.Random(seed)
    pick = rng.sample(range(v.npool), n) if distinct else [rng.randrange(v.npool) for _ in range(n)]
    return v.torch.tensor(pick, dtype=v.torch.int64, device="cuda")


def forms(v, n, seed):
    """n distinct form records of the pool"""
    return v.fw[_idx(v, n, seed, distinct=True)].reshape(-1).contiguous()


def cts(v, n, seed):
    """n ciphertexts of pool forms with n distinct c1"""
    return v.tensor(v.torch, v.fw, _idx(v, n, seed, distinct=True), _idx(v, n, seed + 1, distinct=True))


def ints(n, seed, bits, signed=False):
    """n distinct values of exactly `bits` bits"""
    rng = random.Random(seed)
    vals = set()
    while len(vals) < n:
        vals.add(rng.getrandbits(bits - 1) | 1 << (bits - 1))
    vals = sorted(vals)
    rng.shuffle(vals)
    return [-x if signed and i % 3 == 1 else x for i, x in enumerate(vals)]


def exps(v, vals):
    return v.dev(v.exp_records(vals))


def zeros(v, words):
    return v.torch.zeros(words, dtype=v.torch.int32, device="cuda")


def fbuf(v, n, seed):
    return Buf(v.torch, forms(v, n, seed), REC)


def cbuf(v, n, seed):
    return Buf(v.torch, cts(v, n, seed), CT)


def ebuf(v, vals):
    return Buf(v.torch, exps(v, vals), EXP)


def one(v, t, other, words):
    """an input of ONE record (Enc(0), a share, a key): its decoy is another record, not a roll"""
    return Buf(v.torch, t, words, decoy=other)


def zero_ct(v, seed):
    return one(v, cts(v, 1, seed), cts(v, 1, seed + 7), CT)


def identity_view(v, n):
    return v.VC.to_c(v.VC.identity([n]))


def with_option(name, value, reset, fn):
    """fn under a pinned launcher option of the context, which goes back to `reset` on every way out"""
    def call(E, ptrs, stream):
        E.set_option(name, value)
        try:
            return fn(E, ptrs, stream)
        finally:
            E.set_option(name, reset)
    return call


def encryptions(v, n, seed):
    """n fresh encryptions (own randomness each) of n distinct k-bit plaintexts, made on the null stream"""
    ms = ints(n, seed, v.k)
    rs = [random.Random(seed + 1 + i).randrange(v.bound) for i in range(n)]
    t = v.fresh(v.E, v.torch, v.recs, ms, rs, v.k)
    v.E.stream_sync(0)
    return t


# ---- the builders -------------------------------------------------------------------------------------------------------------

def b_validate(v, variant):
    good = forms(v, 4, 101)
    rng = v.P.SplitMix64(102)
    f = v.P.random_form(v.d, rng)
    # the same class, one step off the reduced form: (a, b + 2a, a + b + c) has the discriminant and |b| > a
    bad = good.clone()
    bad[2 * REC:3 * REC] = v.dev(v.form_record(f.a, f.b + 2 * f.a, f.a + f.b + f.c))
    return Case([Buf(v.torch, bad, REC, decoy=good)], [], lambda E, p, s: E.validate_records(p[0], 4, stream=s), syncs=True)


def b_compose(v, variant):
    out = zeros(v, 5 * REC)
    return Case([fbuf(v, 5, 110), fbuf(v, 5, 120)], [out], lambda E, p, s: E.compose_records(p[0], p[1], out.data_ptr(), 5, stream=s))


def b_compose_wide(v, variant):
    out = zeros(v, 3 * REC)
    return Case([fbuf(v, 3, 130), fbuf(v, 3, 140)], [out], lambda E, p, s: E.compose_wide_records(p[0], p[1], out.data_ptr(), 3, stream=s))


def b_add_ct(v, variant):
    out = zeros(v, 5 * CT)
    return Case([cbuf(v, 5, 150), cbuf(v, 5, 160)], [out], lambda E, p, s: E.add_ciphertext_records(p[0], p[1], out.data_ptr(), 5, stream=s), n=5)


def b_sub_ct(v, variant):
    out = zeros(v, 5 * CT)
    return Case([cbuf(v, 5, 170), cbuf(v, 5, 180)], [out], lambda E, p, s: E.sub_ciphertext_records(p[0], p[1], out.data_ptr(), 5, stream=s))


def b_invert(v, variant):
    out = zeros(v, 5 * REC)
    return Case([fbuf(v, 5, 190)], [out], lambda E, p, s: E.invert_records(p[0], out.data_ptr(), 5, stream=s))


def b_pow(v, variant):
    es = ints(3, 201, v.k, signed=True)
    ins = [cbuf(v, 3, 200), ebuf(v, es)]
    if variant == "in place":
        return Case(ins, [0], lambda E, p, s: E.pow_records(p[0], p[1], p[0], 3, stream=s), n=3, exps=es)
    out = zeros(v, 3 * CT)
    return Case(ins, [out], lambda E, p, s: E.pow_records(p[0], p[1], out.data_ptr(), 3, stream=s), n=3, exps=es)


def b_pow_form(v, variant):
    out = zeros(v, 3 * REC)
    return Case([fbuf(v, 3, 210), ebuf(v, ints(3, 211, v.k, signed=True))], [out],
                lambda E, p, s: E.pow_form_records(p[0], p[1], out.data_ptr(), 3, stream=s))


def b_scal_matmul(v, variant):
    n, m, p_ = 2, 3, 2
    out = zeros(v, n * p_ * CT)
    fn = lambda E, p, s: E.scal_matmul_records(p[0], p[1], p[2], out.data_ptr(), n, m, p_, stream=s)      # noqa: E731
    return Case([cbuf(v, n * m, 220), ebuf(v, ints(m * p_, 221, v.k, signed=True)), zero_ct(v, 222)], [out],
                with_option("matmul_tree", 1 if variant == "tree" else 0, -1, fn), syncs=True)


def b_matmul_plain_ct(v, variant):
    n, m, p_ = 2, 3, 2
    out = zeros(v, n * p_ * CT)
    return Case([ebuf(v, ints(n * m, 230, v.k, signed=True)), cbuf(v, m * p_, 231), zero_ct(v, 232)], [out],
                lambda E, p, s: E.matmul_plain_ct_records(p[0], p[1], p[2], out.data_ptr(), n, m, p_, stream=s), syncs=True)


def _conv_case(v, variant, groups, seed):
    B, H, W, C = IMAGE
    filters = (2, 2, C // groups, 2)
    out = zeros(v, B * 3 * 3 * 2 * CT)
    fn = lambda E, p, s: E.conv2d_plain_ct_records(p[0], p[1], p[2], out.data_ptr(), IMAGE, filters, stream=s, groups=groups)   # noqa: E731
    w = ints(filters[0] * filters[1] * filters[2] * filters[3], seed, 16, signed=True)
    return Case([ebuf(v, w), cbuf(v, B * H * W * C, seed + 1), zero_ct(v, seed + 2)], [out],
                with_option("conv_route", 1 if variant == "direct" else 2, 0, fn), syncs=True)


def b_conv2d(v, variant):
    return _conv_case(v, variant, 1, 240)


def b_conv2d_grouped(v, variant):
    return _conv_case(v, variant, 2, 250)


def b_sum_pool(v, variant):
    B, H, W, C = IMAGE
    out = zeros(v, B * 2 * 2 * C * CT)
    fn = lambda E, p, s: E.sum_pool2d_records(p[0], p[1], out.data_ptr(), IMAGE, (2, 2), stream=s)      # noqa: E731
    return Case([cbuf(v, B * H * W * C, 260), zero_ct(v, 261)], [out], with_option("conv_route", 1 if variant == "direct" else 2, 0, fn), syncs=True)


def b_matmul_plain_plain(v, variant):
    n, m, p_ = 3, 5, 4
    out = zeros(v, n * p_ * EXP)
    return Case([ebuf(v, ints(n * m, 270, v.k, signed=True)), ebuf(v, ints(m * p_, 271, v.k, signed=True))], [out],
                lambda E, p, s: E.matmul_plain_plain_records(p[0], p[1], out.data_ptr(), n, m, p_, v.k, stream=s))


def b_conv2d_plain_plain(v, variant):
    filters = (2, 2, 2, 2)
    out = zeros(v, 3 * 3 * 2 * EXP)
    return Case([ebuf(v, ints(32, 280, v.k, signed=True)), ebuf(v, ints(16, 281, v.k, signed=True))], [out],
                lambda E, p, s: E.conv2d_plain_plain_records(p[0], p[1], out.data_ptr(), IMAGE, filters, v.k, stream=s))


def b_conv2d_ct_filters(v, variant):
    filters = (2, 2, 2, 2)
    out = zeros(v, 3 * 3 * 2 * CT)
    return Case([ebuf(v, ints(32, 290, 16, signed=True)), cbuf(v, 16, 291), zero_ct(v, 292)], [out],
                lambda E, p, s: E.conv2d_ct_filters_records(p[0], p[1], p[2], out.data_ptr(), IMAGE, filters, stream=s), syncs=True)


def b_pow_dot(v, variant):
    n, d = 3, 2
    out = zeros(v, n * CT)
    return Case([cbuf(v, d * n, 300), ebuf(v, ints(d * n, 301, v.k, signed=True))], [out],
                lambda E, p, s: E.pow_dot_records(p[0], p[1], out.data_ptr(), n, d, stream=s))


def b_poly_shift(v, variant):
    n, d = 5, 2
    out = zeros(v, (d + 1) * n * EXP)
    return Case([ebuf(v, ints(d + 1, 310, v.k, signed=True)), ebuf(v, ints(n, 311, v.k, signed=True))], [out],
                lambda E, p, s: E.poly_shift_records(p[0], p[1], out.data_ptr(), n, d, v.k, stream=s))


def b_poly_close(v, variant, seed=0):
    n, d = 5, 2
    out = zeros(v, n * CT)
    coef, es = ints(d + 1, 320 + seed, v.k, signed=True), ints(n, 321 + seed, v.k, signed=True)
    return Case([ebuf(v, coef), ebuf(v, es), cbuf(v, d * n, 322 + seed)], [out],
                lambda E, p, s: E.poly_close_records(p[0], p[1], p[2], v.recs["f"], out.data_ptr(), n, d, v.k, stream=s), n=n, d=d, coef=coef, es=es)


def b_divfloor(v, variant):
    n = 5
    out = zeros(v, n * EXP)
    return Case([ebuf(v, ints(n, 330, v.k, signed=True)), ebuf(v, ints(n, 331, 40))], [out],
                lambda E, p, s: E.divfloor_plain_records(p[0], p[1], n, out.data_ptr(), n, v.k, stream=s))


def b_div_close(v, variant, seed=0):
    n = 5
    out = zeros(v, n * CT)
    es, divs = ints(n, 340 + seed, v.k, signed=True), ints(n, 341 + seed, 40)
    return Case([ebuf(v, es), ebuf(v, divs), cbuf(v, n, 342 + seed)], [out],
                lambda E, p, s: E.div_close_records(p[0], p[1], n, p[2], v.recs["f"], out.data_ptr(), n, v.k, stream=s), n=n, es=es, divs=divs)


def b_divmod(v, variant):
    n, rows = 5, 7
    q, rem = zeros(v, n * EXP), zeros(v, n)
    return Case([ebuf(v, ints(n, 350, v.k, signed=True)), ebuf(v, [3, 7, 2, 5, 6])], [q, rem],
                lambda E, p, s: E.divmod_plain_records(p[0], p[1], n, q.data_ptr(), rem.data_ptr(), n, rows, v.k, stream=s))


def b_divx_rows(v, variant):
    n, rows = 3, 4
    out = zeros(v, n * rows * EXP)
    return Case([ebuf(v, ints(n, 360, v.k)), ebuf(v, [3, 4, 2])], [out],
                lambda E, p, s: E.divx_rows_records(p[0], p[1], n, out.data_ptr(), n, rows, v.k, stream=s))


def rho_values(v, n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, v.bound) for _ in range(n)]


def _rho(v, n, seed):
    return ebuf(v, rho_values(v, n, seed))


def b_divx_tuples(v, variant):
    n, rows = 3, 4
    out = zeros(v, n * rows * CT)
    r = v.recs
    return Case([ebuf(v, ints(n, 370, v.k)), ebuf(v, [3, 4, 2]), _rho(v, n * rows, 371)], [out],
                lambda E, p, s: E.divx_tuples_records(p[0], p[1], n, p[2], r["h"], r["pk"], r["f"], out.data_ptr(), n, rows, v.k, stream=s), syncs=True)


def b_divx_close(v, variant, seed=0):
    n, rows = 3, 4
    out = zeros(v, n * CT)
    es, divs = ints(n, 380 + seed, v.k, signed=True), [3, 4, 2]
    return Case([ebuf(v, es), ebuf(v, divs), cbuf(v, n * rows, 381 + seed)], [out],
                lambda E, p, s: E.divx_close_records(p[0], p[1], n, p[2], rows, v.recs["f"], out.data_ptr(), n, v.k, stream=s), n=n, rows=rows, es=es,
                divs=divs)


def b_lut_rotate(v, variant):
    n, bits = 5, 2
    out = zeros(v, (n << bits) * EXP)
    return Case([ebuf(v, ints(1 << bits, 390, v.k)), ebuf(v, ints(n, 391, v.k))], [out],
                lambda E, p, s: E.lut_rotate_records(p[0], 1, p[1], out.data_ptr(), n, bits, stream=s))


def b_lut_tuples(v, variant):
    n, bits = 3, 2
    out = zeros(v, (n << bits) * CT)
    r = v.recs
    return Case([ebuf(v, ints(1 << bits, 400, v.k)), ebuf(v, ints(n, 401, v.k)), _rho(v, n << bits, 402)], [out],
                lambda E, p, s: E.lut_tuples_records(p[0], 1, p[1], p[2], r["h"], r["pk"], r["f"], out.data_ptr(), n, bits, v.k, stream=s), syncs=True)


def b_lut_select(v, variant):
    n, bits = 5, 2
    out = zeros(v, n * CT)
    return Case([ebuf(v, ints(n, 410, v.k, signed=True)), cbuf(v, n << bits, 411)], [out],
                lambda E, p, s: E.lut_select_records(p[0], p[1], out.data_ptr(), n, bits, stream=s))


CMP = (8, 2)                                 # bits, digit_bits: 4 digits of 4 entries each


def b_cmp_rows(v, variant):
    n = 3
    out = zeros(v, n * 16 * EXP)
    return Case([ebuf(v, ints(n, 420, v.k))], [out], lambda E, p, s: E.cmp_rows_records(p[0], out.data_ptr(), n, CMP[0], CMP[1], v.k, stream=s))


def b_cmp_tuples(v, variant):
    n = 2
    out = zeros(v, n * 16 * CT)
    r = v.recs
    return Case([ebuf(v, ints(n, 430, v.k)), _rho(v, n * 16, 431)], [out],
                lambda E, p, s: E.cmp_tuples_records(p[0], p[1], r["h"], r["pk"], r["f"], out.data_ptr(), n, CMP[0], CMP[1], v.k, stream=s), syncs=True)


def b_cmp_close(v, variant):
    n = 2
    out, wrap = zeros(v, 2 * n * CT), zeros(v, n * EXP)
    return Case([ebuf(v, ints(n, 440, v.k, signed=True)), cbuf(v, n * 16, 441)], [out, wrap],
                lambda E, p, s: E.cmp_close_records(p[0], p[1], out.data_ptr(), wrap.data_ptr(), n, CMP[0], CMP[1], v.k, stream=s))


N_HOLDER = 2                                 # form records the holder of test_gpu_streams.py writes


def b_view(v, variant):
    out = zeros(v, N_HOLDER * REC)
    flip = v.VC.to_c(v.VC.flip([N_HOLDER], 0))
    return Case([], [out], lambda E, p, s: E.view_records(flip, p[0], 0, out.data_ptr(), REC, stream=s), reads_holder=True)


def b_gather(v, variant):
    out = zeros(v, 3 * REC)
    idx = v.torch.tensor([1, 0, 1], dtype=v.torch.int32, device="cuda")
    dec = v.torch.tensor([0, 1, 0], dtype=v.torch.int32, device="cuda")
    return Case([Buf(v.torch, idx, 1, decoy=dec)], [out],
                lambda E, p, s: E.gather_records(p[1], N_HOLDER, p[0], 0, out.data_ptr(), 3, REC, stream=s), reads_holder=True)


SPLINE = (1, 2, 1)                           # bits, shift, d: two pieces of two coefficients


def b_spline_rows(v, variant):
    n, (bits, shift, d) = 3, SPLINE
    out = zeros(v, (n << bits) * (d + 1) * EXP)
    return Case([ebuf(v, ints((1 << bits) * (d + 1), 450, v.k)), ebuf(v, ints(n, 451, v.k))], [out],
                lambda E, p, s: E.spline_rows_records(p[0], 1, p[1], out.data_ptr(), n, bits, shift, d, v.k, stream=s))


def b_spline_tuples(v, variant):
    n, (bits, shift, d) = 2, SPLINE
    rows = (n << bits) * (d + 1)
    out = zeros(v, rows * CT)
    r = v.recs
    return Case([ebuf(v, ints((1 << bits) * (d + 1), 460, v.k)), ebuf(v, ints(n, 461, v.k)), _rho(v, rows, 462)], [out],
                lambda E, p, s: E.spline_tuples_records(p[0], 1, p[1], p[2], r["h"], r["pk"], r["f"], out.data_ptr(), n, bits, shift, d, v.k, stream=s),
                syncs=True)


def b_spline_powers(v, variant):
    n, d = 5, 2
    out = zeros(v, d * n * EXP)
    return Case([ebuf(v, ints(n, 470, v.k, signed=True))], [out], lambda E, p, s: E.spline_powers_records(p[0], out.data_ptr(), n, d, v.k, stream=s))


def b_spline_close(v, variant):
    n, (bits, shift, d) = 3, SPLINE
    out = zeros(v, n * CT)
    return Case([ebuf(v, ints(n, 480, v.k, signed=True)), cbuf(v, (n << bits) * (d + 1), 481)], [out],
                lambda E, p, s: E.spline_close_records(p[0], p[1], out.data_ptr(), n, bits, shift, d, v.k, stream=s))


def _sk(v):
    from gpu_inputs import hx
    return hx(v.prm["sk"])


def b_decrypt(v, variant, n=3):
    out = zeros(v, n * ((v.k + 31) // 32 + 1))
    # the decoy of the key is another key: its ciphertexts do not land in <f>, which the kernel reports in the status word of
    # each output (tests/test_gpu_parity.py, the wrong share)
    key = one(v, exps(v, [_sk(v)]), exps(v, [_sk(v) + 1]), EXP)
    # from 64 ciphertexts on the call reads back whether they share their c1
    return Case([Buf(v.torch, encryptions(v, n, 490), CT), key], [out],
                lambda E, p, s: E.decrypt_records(p[0], p[1], v.recs["f"], out.data_ptr(), n, v.k, stream=s), syncs=n >= 64, n=n, plain=ints(n, 490, v.k))


def b_accumulate(v, variant):
    n, m, p_ = 2, 4 if variant == "tree" else 3, 2             # m >= 4 with few outputs: the pairwise tree; below: the chain kernel
    out = zeros(v, n * p_ * CT)
    return Case([cbuf(v, n * m * p_, 500), zero_ct(v, 501)], [out],
                lambda E, p, s: E.accumulate_records(p[0], p[1], out.data_ptr(), n, m, p_, stream=s))


def _prefilled(v, out, junk, fn):
    """an entry without device inputs: the call first copies valid junk over its output ON THE STREAM, so that a kernel of
    the entry launched on another stream has its result overwritten"""
    view = identity_view(v, out.numel() // REC)

    def call(E, ptrs, stream):
        E.view_records(view, junk.data_ptr(), 0, out.data_ptr(), REC, stream=stream)
        return fn(E, ptrs, stream)
    return call


def b_pow_fixed_base_record(v, variant):
    out = zeros(v, REC)
    base = v.fw[3].cpu().numpy().view(v.np.uint32)
    e = v.exp_records(ints(1, 510, 960))
    fn = lambda E, p, s: E.pow_fixed_base_record(base, e, out.data_ptr(), stream=s)      # noqa: E731
    return Case([], [out], _prefilled(v, out, forms(v, 1, 511), fn), syncs=True, no_inputs=True)


def b_pow_fixed_base_records(v, variant):
    out = zeros(v, 2 * REC)
    base = v.np.concatenate([v.recs["h"], v.recs["pk"]])
    e = v.exp_records(ints(2, 520, 960))
    fn = lambda E, p, s: E.pow_fixed_base_records(base, e, out.data_ptr(), stream=s)      # noqa: E731
    return Case([], [out], _prefilled(v, out, forms(v, 2, 521), fn), syncs=True, no_inputs=True)


def b_encrypt(v, variant):
    n = 5
    out = zeros(v, n * CT)
    return Case([ebuf(v, ints(n, 530, v.k, signed=True)), one(v, forms(v, 2, 531), forms(v, 2, 532), 2 * REC)], [out],
                lambda E, p, s: E.encrypt_records(p[0], p[1], v.recs["f"], out.data_ptr(), n, v.k, stream=s), syncs=True)


def b_pow_fixed_base_many(v, variant):
    n = 5
    out = zeros(v, n * REC)
    return Case([ebuf(v, ints(n, 540, 960, signed=True))], [out],
                lambda E, p, s: E.pow_fixed_base_many_records(v.recs["h"], p[0], out.data_ptr(), n, stream=s), syncs=True)


def b_encrypt_fresh(v, variant):
    n = 3
    out = zeros(v, n * CT)
    r = v.recs
    return Case([ebuf(v, ints(n, 550, v.k, signed=True)), _rho(v, n, 551)], [out],
                lambda E, p, s: E.encrypt_fresh_records(p[0], p[1], r["h"], r["pk"], r["f"], out.data_ptr(), n, v.k, stream=s), syncs=True)


def b_rerandomize(v, variant, seed=0):
    n = 5
    out = zeros(v, n * CT)
    r = v.recs
    return Case([cbuf(v, n, 560 + seed), _rho(v, n, 561 + seed)], [out],
                lambda E, p, s: E.rerandomize_records(p[0], p[1], r["h"], r["pk"], out.data_ptr(), n, stream=s), syncs=True, n=n,
                rs=rho_values(v, n, 561 + seed))


def b_add_plain(v, variant, seed=0):
    n = 5
    out = zeros(v, n * CT)
    r = v.recs
    if variant == "fresh randomness":                            # kind 4: the one read-back of the longest exponent
        return Case([cbuf(v, n, 570), ebuf(v, ints(n, 571, v.k, signed=True)), _rho(v, n, 572)], [out],
                    lambda E, p, s: E.add_plain_records(p[0], p[1], r["f"], out.data_ptr(), n, v.k, 0, d_r=p[2], h_record=r["h"], pk_record=r["pk"],
                                                        stream=s), syncs=True)
    ms = ints(n, 571 + seed, v.k, signed=True)
    return Case([cbuf(v, n, 570 + seed), ebuf(v, ms)], [out],
                lambda E, p, s: E.add_plain_records(p[0], p[1], r["f"], out.data_ptr(), n, v.k, 1, stream=s), n=n, ms=ms, mode=1)


def b_part_decrypt(v, variant, seed=0, n=3):
    out = zeros(v, n * REC)
    sh = ints(1, 580 + seed, 960)
    share = one(v, exps(v, sh), exps(v, ints(1, 581 + seed, 960)), EXP)
    return Case([cbuf(v, n, 582 + seed), share], [out], lambda E, p, s: E.part_decrypt_records(p[0], p[1], out.data_ptr(), n, stream=s), n=n,
                share=sh[0])


def b_combine(v, variant):
    n = 3
    ct = encryptions(v, n, 590)
    parts = zeros(v, n * REC)
    v.E.part_decrypt_records(ct.data_ptr(), exps(v, [_sk(v)]).data_ptr(), parts.data_ptr(), n)
    v.E.stream_sync(0)
    out = zeros(v, n * ((v.k + 31) // 32 + 1))
    return Case([Buf(v.torch, ct, CT), Buf(v.torch, parts, REC)], [out],
                lambda E, p, s: E.combine_part_decryptions_records(p[0], p[1], [1], v.recs["f"], out.data_ptr(), n, v.k, stream=s), n=n,
                plain=ints(n, 590, v.k))


WIRE_SHAPE = [1, 3, 1]                       # an odd ndim: the offset table of the serialised tensor is not 8-byte aligned


def _padded_bytes(v, data):
    raw = v.np.frombuffer(data + b"\0" * (-len(data) % 4), dtype=v.np.uint32)
    return v.dev(raw)


def b_unpack(v, variant):
    c = cts(v, 3, 600)
    E = v.E
    host = lambda t: t.cpu().numpy().view(v.np.uint32)       # noqa: E731
    data = E.records_to_bytes(host(c), WIRE_SHAPE)
    decoy = E.records_to_bytes(host(v.torch.roll(c.view(3, CT), 1, 0).reshape(-1)), WIRE_SHAPE)
    assert len(decoy) == len(data)                              # the same integers in another order
    out = zeros(v, 6 * REC)
    return Case([Buf(v.torch, _padded_bytes(v, data), 1, decoy=_padded_bytes(v, decoy))], [out],
                lambda E, p, s: E.unpack_tensor_device(p[0], len(data), 2, out.data_ptr(), 6, stream=s), syncs=True)


def b_pack(v, variant):
    cap = v.E.packed_size_bound(6, 2, len(WIRE_SHAPE))
    out = zeros(v, (cap + 3) // 4)
    return Case([cbuf(v, 3, 610)], [out], lambda E, p, s: E.pack_tensor_device(p[0], 6, 2, WIRE_SHAPE, out.data_ptr(), cap, stream=s), syncs=True)


def b_device_status(v, variant):
    # the status word as the entry reads it on its stream: an index beyond the source of cofhe_hip_gather_records sets bit 32
    # there (nothing is read out of range, and without a fill record the output keeps what it had)
    src = forms(v, 2, 620)
    out = zeros(v, 3 * REC)
    idx = v.torch.tensor([1, 99, 0], dtype=v.torch.int32, device="cuda")
    dec = v.torch.tensor([0, 1, 0], dtype=v.torch.int32, device="cuda")

    def call(E, p, s):
        E.gather_records(src.data_ptr(), 2, p[0], 0, out.data_ptr(), 3, REC, stream=s)
        return E.device_status(clear=True, stream=s)
    return Case([Buf(v.torch, idx, 1, decoy=dec)], [out], call, syncs=True)


def b_free_on_stream(v, variant):
    # a block that carries the data from its input to the output and goes back behind the stream's work at once
    n = 3
    out = zeros(v, n * REC)
    view = identity_view(v, n)

    def call(E, p, s):
        blk = E.malloc(n * REC * 4)
        E.view_records(view, p[0], 0, blk, REC, stream=s)
        E.view_records(view, blk, 0, out.data_ptr(), REC, stream=s)
        E.free(blk, stream=s)
    return Case([fbuf(v, n, 630)], [out], call)


TABLE = {
    "cofhe_hip_free_on_stream": b_free_on_stream,
    "cofhe_hip_device_status": b_device_status,
    "cofhe_hip_validate_records": b_validate,
    "cofhe_hip_compose_records": b_compose,
    "cofhe_hip_compose_wide_records": b_compose_wide,
    "cofhe_hip_add_ciphertext_records": b_add_ct,
    "cofhe_hip_sub_ciphertext_records": b_sub_ct,
    "cofhe_hip_invert_records": b_invert,
    "cofhe_hip_pow_records": b_pow,
    "cofhe_hip_scal_matmul_records": b_scal_matmul,
    "cofhe_hip_matmul_plain_ct_records": b_matmul_plain_ct,
    "cofhe_hip_conv2d_plain_ct_records": b_conv2d,
    "cofhe_hip_conv2d_grouped_plain_ct_records": b_conv2d_grouped,
    "cofhe_hip_sum_pool2d_records": b_sum_pool,
    "cofhe_hip_matmul_plain_plain_records": b_matmul_plain_plain,
    "cofhe_hip_conv2d_plain_plain_records": b_conv2d_plain_plain,
    "cofhe_hip_conv2d_ct_filters_records": b_conv2d_ct_filters,
    "cofhe_hip_pow_dot_records": b_pow_dot,
    "cofhe_hip_poly_shift_records": b_poly_shift,
    "cofhe_hip_poly_close_records": b_poly_close,
    "cofhe_hip_divfloor_plain_records": b_divfloor,
    "cofhe_hip_div_close_records": b_div_close,
    "cofhe_hip_divmod_plain_records": b_divmod,
    "cofhe_hip_divx_rows_records": b_divx_rows,
    "cofhe_hip_divx_tuples_records": b_divx_tuples,
    "cofhe_hip_divx_close_records": b_divx_close,
    "cofhe_hip_lut_rotate_records": b_lut_rotate,
    "cofhe_hip_lut_tuples_records": b_lut_tuples,
    "cofhe_hip_lut_select_records": b_lut_select,
    "cofhe_hip_cmp_rows_records": b_cmp_rows,
    "cofhe_hip_cmp_tuples_records": b_cmp_tuples,
    "cofhe_hip_cmp_close_records": b_cmp_close,
    "cofhe_hip_view_records": b_view,
    "cofhe_hip_gather_records": b_gather,
    "cofhe_hip_spline_rows_records": b_spline_rows,
    "cofhe_hip_spline_tuples_records": b_spline_tuples,
    "cofhe_hip_spline_powers_records": b_spline_powers,
    "cofhe_hip_spline_close_records": b_spline_close,
    "cofhe_hip_decrypt_records": b_decrypt,
    "cofhe_hip_accumulate_records": b_accumulate,
    "cofhe_hip_pow_form_records": b_pow_form,
    "cofhe_hip_pow_fixed_base_record": b_pow_fixed_base_record,
    "cofhe_hip_pow_fixed_base_records": b_pow_fixed_base_records,
    "cofhe_hip_encrypt_records": b_encrypt,
    "cofhe_hip_pow_fixed_base_many_records": b_pow_fixed_base_many,
    "cofhe_hip_encrypt_fresh_records": b_encrypt_fresh,
    "cofhe_hip_rerandomize_records": b_rerandomize,
    "cofhe_hip_add_plain_records": b_add_plain,
    "cofhe_hip_part_decrypt_records": b_part_decrypt,
    "cofhe_hip_combine_part_decryptions_records": b_combine,
    "cofhe_hip_unpack_tensor_device": b_unpack,
    "cofhe_hip_pack_tensor_device": b_pack,
}

# the entries that are built once per route; every other entry has the one variant ""
VARIANTS = {
    "cofhe_hip_pow_records": ("out of place", "in place"),
    "cofhe_hip_accumulate_records": ("chain", "tree"),
    "cofhe_hip_scal_matmul_records": ("chains", "tree"),
    "cofhe_hip_conv2d_plain_ct_records": ("direct", "gather"),
    "cofhe_hip_conv2d_grouped_plain_ct_records": ("direct", "gather"),
    "cofhe_hip_sum_pool2d_records": ("direct", "gather"),
    "cofhe_hip_add_plain_records": ("deterministic", "fresh randomness"),
}


def case_ids():
    """(entry, variant) of every case, in the table's order"""
    return [(name, var) for name in TABLE for var in VARIANTS.get(name, ("",))]
