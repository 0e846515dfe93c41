"""GPU: the C ABI on NON-BLOCKING streams of one context (cofhe_hip_stream_create): every entry that takes a stream runs
behind other work on such a stream and must see it; the workspace, the table caches, the block cache and the flag words are
handed from stream to stream and between two host threads; a destroyed stream is forgotten.  Everything is exact.

The holder: cofhe_hip_part_decrypt_records of 2 ciphertexts with distinct c1 under a 960-bit share, into a buffer of its own --
one ladder's time on its stream and on the workspace, returned without a host synchronisation.  Every scenario that leans on
"the holder is still running" ASSERTS it with cofhe_hip_stream_query instead of assuming it, and checks the holder's result
against the GMP oracle, so a clobbered workspace shows there too.
Measured on an MI355X with cofhe_hip_timer_start / _stop on its stream: one holder takes 128.1 ms (three runs: 128.14, 128.09,
128.77), and cofhe_hip_stream_query right after enqueuing it says "busy".

References: the GMP oracle (oracle_lib) and the plain-integer models of the *_cases modules where one call gives the answer;
otherwise the same entry alone on the null stream (of a context of its own where the scenario is about a context's state).
Two results of one racing run are never compared with each other.  At most three streams are alive at a time."""
import contextlib
import ctypes as C
import random
import threading

import numpy as np
import pytest

import div_cases as DC
import divx_cases as DX
import poly_cases as PC
import stream_cases as SC
from gpu_inputs import P, _device_status_stays_clear, _pt_bytes  # noqa: F401
import oracle_lib as O

pytestmark = pytest.mark.gpu
REC, CT, EXP = SC.REC, SC.CT, SC.EXP
HOLDER_TIMES = 1                             # the holder is enqueued this many times in a row
EARLY = "the holder had finished before the dependent call was enqueued: nothing was proved"


@pytest.fixture(scope="module")
def v(params128):
    return SC.env(params128)


@pytest.fixture(scope="module")
def ref_engine(v):
    """a context of its own for references: its null stream, its own workspace and caches"""
    from cofhe_amd import Engine
    E = Engine(v.d)
    yield E
    assert E.device_status(clear=True) == 0
    E.close()


@contextlib.contextmanager
def fresh_engine(v):
    """a context with cold caches; its status word is checked here (the module's fixture sees the cached engines only)"""
    from cofhe_amd import Engine
    E = Engine(v.d)
    try:
        yield E
        assert E.device_status(clear=True) == 0
    finally:
        E.close()


@contextlib.contextmanager
def streams(E, n):
    assert n <= 3                            # the machines run with 4 hardware queues
    made = []
    try:
        for _ in range(n):
            made.append(E.stream_create(nonblocking=1))
        yield made
    finally:
        for s in made:
            E.stream_destroy(s)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def ct_bytes(E, t, n):
    return E.records_to_bytes(host(t), [n])


def c1_powers(v, E, cts, n, e):
    """the partial decryptions c1^e of n ciphertexts by the GMP oracle, serialised"""
    want = O.scal_1d(v.d, _pt_bytes([n], [e] * n), ct_bytes(E, cts, n))
    _, w = P.deserialize_ciphertext_tensor(want)
    return P.serialize_form_tensor([n], [c[0] for c in w])


class Holder:
    """the holder and its oracle value, made once; a decoy of valid form records to pre-fill its output with"""

    def __init__(self, v):
        self.v, self.n = v, SC.N_HOLDER
        self.cts = SC.cts(v, self.n, 7000)
        self.e = SC.ints(1, 7005, 960)[0]
        self.share = SC.exps(v, [self.e])
        self.decoy = SC.forms(v, self.n, 7010)
        self.out = self.decoy.clone()
        self.want = c1_powers(v, v.E, self.cts, self.n, self.e)
        _, recs = v.E.pdr_bytes_to_records(self.want)
        self.want_dev = v.dev(recs)

    def reset(self):
        self.out.copy_(self.decoy)

    def enqueue(self, E, stream):
        for _ in range(HOLDER_TIMES):
            E.part_decrypt_records(self.cts.data_ptr(), self.share.data_ptr(), self.out.data_ptr(), self.n, stream=stream)

    def check(self, E):
        assert E.pdr_records_to_bytes(host(self.out), [self.n]) == self.want, "the holder's own result is wrong"


@pytest.fixture(scope="module")
def holder(v):
    return Holder(v)


def busy(E, stream):
    assert E.stream_query(stream) == 1, EARLY


class Run:
    """one run of a Case: working copies of its inputs (so that an in-place call spoils nothing), its outputs zeroed"""

    def __init__(self, v, case, decoys=False):
        self.v, self.case = v, case
        self.work = [(b.decoy if decoys else b.t).clone() for b in case.inputs]
        for o in case.outputs:
            if not isinstance(o, int):
                o.zero_()
        self.ret = None

    def ptrs(self, extra=()):
        return [w.data_ptr() for w in self.work] + [t.data_ptr() for t in extra]

    def fill_on(self, E, stream):
        """the real inputs over the working copies, by identity views on `stream`"""
        for b, w in zip(self.case.inputs, self.work):
            E.view_records(SC.identity_view(self.v, b.n), b.t.data_ptr(), 0, w.data_ptr(), b.words, stream=stream)

    def result(self):
        return self.ret, [(self.work[o] if isinstance(o, int) else o).clone() for o in self.case.outputs]


def same(a, b):
    import torch
    return a[0] == b[0] and len(a[1]) == len(b[1]) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


def alone(v, E, case, decoys=False, extra=()):
    """the case alone on the null stream of E"""
    run = Run(v, case, decoys)
    v.torch.cuda.synchronize()
    run.ret = case.call(E, run.ptrs(extra), 0)
    E.stream_sync(0)
    return run.result()


# ---- (a) stream order is the only order -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name,variant", SC.case_ids(), ids=["%s%s" % (n[len("cofhe_hip_"):], "-" + x.replace(" ", "_") if x else "") for n, x in SC.case_ids()])
def test_stream_order_is_the_only_order(v, holder, name, variant):
    """On one non-blocking stream: the holder, then identity views that copy the real inputs over buffers of decoys, then the
    entry, reading those buffers.  An entry that launches a kernel, a copy or a memset on another stream -- itself or through a
    nested call that drops the stream -- runs it before the holder has finished and computes on the decoys.  The result equals
    the entry's result alone on the null stream, and the decoys' result there differs.  view_records and gather_records read the
    holder's own output buffer, pre-filled with decoy records, since they cannot vouch for themselves"""
    E = v.E
    case = SC.TABLE[name](v, variant)
    want = alone(v, E, case, extra=[holder.want_dev] if case.reads_holder else ())
    if not case.no_inputs:
        off = alone(v, E, case, decoys=True, extra=[holder.decoy] if case.reads_holder else ())
        assert not same(off, want), "the decoys give the same result: the case proves nothing"
    run = Run(v, case, decoys=True)
    holder.reset()
    v.torch.cuda.synchronize()
    with streams(E, 1) as (S,):
        holder.enqueue(E, S)
        if case.syncs:
            busy(E, S)
        run.fill_on(E, S)
        run.ret = case.call(E, run.ptrs([holder.out] if case.reads_holder else ()), S)
        if not case.syncs:
            busy(E, S)
        E.stream_sync(S)
    assert same(run.result(), want)
    holder.check(E)


# ---- (b) the workspace goes from stream to stream --------------------------------------------------------------------------------

def oracle_pow(v, E, case):
    n = case.meta["n"]
    return O.scal_1d(v.d, _pt_bytes([n], case.meta["exps"]), ct_bytes(E, case.inputs[0].t, n))


def oracle_rerand(v, E, case):
    from test_gpu_fresh_randomness import oracle_rerand as rr
    return rr(v.d, v.forms, ct_bytes(E, case.inputs[0].t, case.meta["n"]), case.meta["rs"])


def oracle_add_plain(v, E, cts, n, ms):
    """(c1, c2 o f^m) of n ciphertexts by the oracle"""
    fm = O.scal_1d(v.d, _pt_bytes([n], [m % (1 << v.k) for m in ms]), P.serialize_ciphertext_tensor([n], [(P.identity(v.d), v.forms["f"])] * n))
    return O.add(v.d, ct_bytes(E, cts, n), fm)


def plaintexts(v, out, n):
    ow = (v.k + 31) // 32 + 1
    o = host(out).reshape(n, ow)
    assert not o[:, -1].any()
    return [int.from_bytes(r[:-1].tobytes(), "little") for r in o]


def user_case(v, user):
    """a user of the workspace and what checks its result: an oracle's bytes, the plaintexts, or None for "the same entry alone on
    the null stream of a context of its own" """
    E = v.E
    if user == "part_decrypt":
        pd = SC.b_part_decrypt(v, "", seed=40)
        return pd, lambda res: E.pdr_records_to_bytes(host(res[1][0]), [3]) == c1_powers(v, E, pd.inputs[0].t, 3, pd.meta["share"])
    if user == "rerandomize":
        rr = SC.b_rerandomize(v, "", seed=40)
        return rr, lambda res: ct_bytes(E, res[1][0], 5) == oracle_rerand(v, E, rr)
    if user == "pow_in_place":
        pw = SC.b_pow(v, "in place")
        return pw, lambda res: ct_bytes(E, res[1][0], 3) == oracle_pow(v, E, pw)
    if user in ("decrypt_2", "decrypt_64"):
        n = int(user.split("_")[1])
        dec = SC.b_decrypt(v, "", n=n)
        return dec, lambda res: plaintexts(v, res[1][0], n) == dec.meta["plain"]
    build = {"encrypt": (SC.b_encrypt, ""), "accumulate_tree": (SC.b_accumulate, "tree"), "scal_matmul": (SC.b_scal_matmul, "chains"),
             "pow_fixed_base": (SC.b_pow_fixed_base_records, "")}[user]
    return build[0](v, build[1]), None


USERS = ("part_decrypt", "rerandomize", "encrypt", "pow_in_place", "accumulate_tree", "scal_matmul", "pow_fixed_base", "decrypt_2", "decrypt_64")


def check_user(v, ref_engine, case, check, result):
    if check is not None:
        assert check(result)
    else:
        assert same(result, alone(v, ref_engine, case))


@pytest.mark.parametrize("user", USERS)
def test_workspace_handover(v, holder, ref_engine, user):
    """the holder on A, at once a user of the workspace on B: B waits for the event A's call left, both results are right"""
    E = v.E
    case, check = user_case(v, user)
    alone(v, E, case)                         # warm: the tables this user needs are built before the window opens
    run = Run(v, case)
    holder.reset()
    v.torch.cuda.synchronize()
    with streams(E, 2) as (A, B):
        holder.enqueue(E, A)
        if case.syncs:
            busy(E, A)
        run.ret = case.call(E, run.ptrs(), B)
        if not case.syncs:
            busy(E, A)
        E.stream_sync(A)
        E.stream_sync(B)
    holder.check(E)
    check_user(v, ref_engine, case, check, run.result())


def test_workspace_growth_under_a_running_user(v, holder):
    """a fresh context: the holder on A carves a workspace for 2 ladders; part_decrypt of 40 ciphertexts with distinct c1 on B
    needs a larger one, and ensure_workspace must not free what A is using.  The reallocation synchronises B, which waits for
    A: the window is asserted before it"""
    cts = SC.encryptions(v, 40, 8000)
    e = SC.ints(1, 8001, 960)[0]
    share, out = SC.exps(v, [e]), SC.zeros(v, 40 * REC)
    holder.reset()
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E, streams(E, 2) as (A, B):
        holder.enqueue(E, A)
        busy(E, A)
        E.part_decrypt_records(cts.data_ptr(), share.data_ptr(), out.data_ptr(), 40, stream=B)
        E.stream_sync(A)
        E.stream_sync(B)
        holder.check(E)
        assert E.pdr_records_to_bytes(host(out), [40]) == c1_powers(v, E, cts, 40, e)


def test_three_streams_in_turn(v, holder, ref_engine):
    """A, B, C, A with no host synchronisation in between: the holder, part_decrypt, an in-place power, the accumulation tree"""
    E = v.E
    picks = [user_case(v, u) for u in ("part_decrypt", "pow_in_place", "accumulate_tree")]
    assert not any(case.syncs for case, _ in picks)
    runs = [Run(v, case) for case, _ in picks]
    holder.reset()
    v.torch.cuda.synchronize()
    with streams(E, 3) as (A, B, C_):
        holder.enqueue(E, A)
        for run, s in zip(runs, (B, C_, A)):
            if s == A:
                busy(E, A)
            run.ret = run.case.call(E, run.ptrs(), s)
        for s in (A, B, C_):
            E.stream_sync(s)
    holder.check(E)
    for run, (case, check) in zip(runs, picks):
        check_user(v, ref_engine, case, check, run.result())


# ---- (c) tables built on one stream, read on another ---------------------------------------------------------------------------

def test_table_built_on_one_stream_read_on_another(v):
    """a fresh context: add_plain_records without randomness on A builds the chain and the comb table of f and returns with that
    work queued; the same call on B right after hits the cache and must wait for it"""
    a, b = SC.b_add_plain(v, "deterministic", seed=50), SC.b_add_plain(v, "deterministic", seed=60)
    ra, rb = Run(v, a), Run(v, b)
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E, streams(E, 2) as (A, B):
        a.call(E, ra.ptrs(), A)
        b.call(E, rb.ptrs(), B)
        busy(E, A)
        E.stream_sync(A)
        E.stream_sync(B)
        for case, run in ((a, ra), (b, rb)):
            assert case.meta["mode"] == 1
            want = oracle_add_plain(v, E, case.inputs[0].t, 5, [-m for m in case.meta["ms"]])
            assert ct_bytes(E, run.result()[1][0], 5) == want


def test_eviction_under_a_queued_reader(v, holder):
    """a fresh context with the table of f built: on A the holder, then add_plain_records, queued behind it and reading that
    table; on B pow_fixed_base_many_records with 8 further bases at short exponents (w = 4), which takes all 8 comb slots and
    cycles the 4 chain slots.  A's result is right.  Each of B's calls reads back its longest exponent, so B -- and the host --
    wait for A there: the window is asserted before B's first call"""
    a = SC.b_add_plain(v, "deterministic", seed=70)
    ra = Run(v, a)
    bases = [host(v.fw[i]) for i in range(8, 16)]
    es = SC.exps(v, SC.ints(3, 9000, 40))
    outs = [SC.zeros(v, 3 * REC) for _ in bases]
    holder.reset()
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E, streams(E, 2) as (A, B):
        warm = Run(v, a)
        a.call(E, warm.ptrs(), 0)               # builds the table of f
        E.stream_sync(0)
        a.outputs[0].zero_()
        v.torch.cuda.synchronize()
        holder.enqueue(E, A)
        a.call(E, ra.ptrs(), A)
        busy(E, A)
        for base, out in zip(bases, outs):
            E.pow_fixed_base_many_records(base, es.data_ptr(), out.data_ptr(), 3, stream=B)
        E.stream_sync(A)
        E.stream_sync(B)
        holder.check(E)
        assert ct_bytes(E, ra.result()[1][0], 5) == oracle_add_plain(v, E, a.inputs[0].t, 5, [-m for m in a.meta["ms"]])
        for i, out in zip(range(8, 16), outs):
            n = 3
            base = v.fw[i].repeat(2 * n).contiguous()       # (base, base) as n ciphertexts for the oracle's element-wise power
            want = O.scal_1d(v.d, _pt_bytes([n], SC.ints(3, 9000, 40)), ct_bytes(E, base, n))
            _, w = P.deserialize_ciphertext_tensor(want)
            assert E.pdr_records_to_bytes(host(out), [n]) == P.serialize_form_tensor([n], [c[0] for c in w]), i


def test_decryption_table_shared_with_the_combiner(v):
    """a fresh context: decrypt_records on A with (f, k) builds the table f^(-2^j); combine_part_decryptions_records on B reads
    the same table and takes no part in the workspace handover"""
    dec, comb = SC.b_decrypt(v, "", n=2), SC.b_combine(v, "")
    rd, rc = Run(v, dec), Run(v, comb)
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E, streams(E, 2) as (A, B):
        dec.call(E, rd.ptrs(), A)
        comb.call(E, rc.ptrs(), B)
        busy(E, A)
        E.stream_sync(A)
        E.stream_sync(B)
    assert plaintexts(v, rd.result()[1][0], 2) == dec.meta["plain"]
    assert plaintexts(v, rc.result()[1][0], 3) == comb.meta["plain"]


# ---- (d) the block cache ----------------------------------------------------------------------------------------------------------

def test_free_on_stream_orders_the_reuse(v, holder):
    """a block freed behind the work queued on A, taken again and written on B: what A's copies carried through it arrives"""
    n = 3
    sz = n * REC * 4
    src1, src2, R = SC.forms(v, n, 9100), SC.forms(v, n, 9110), SC.zeros(v, n * REC)
    view = SC.identity_view(v, n)
    holder.reset()
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E, streams(E, 2) as (A, B):
        p = E.malloc(sz)
        holder.enqueue(E, A)
        E.view_records(view, src1.data_ptr(), 0, p, REC, stream=A)
        E.view_records(view, p, 0, R.data_ptr(), REC, stream=A)
        E.free(p, stream=A)
        busy(E, A)
        q = E.malloc(sz)
        assert q == p, "the block was not handed out again: the reuse was not exercised"
        E.view_records(view, src2.data_ptr(), 0, q, REC, stream=B)
        E.stream_sync(A)
        E.stream_sync(B)
        holder.check(E)
        assert v.torch.equal(R, src1)
        assert np.array_equal(E.download(q, sz), host(src2))
        E.free(q)


def want_poly_close(v, E, case):
    n, d, M = case.meta["n"], case.meta["d"], 1 << v.k
    q = [PC.taylor_shift([c % M for c in case.meta["coef"]], e % M, v.k) for e in case.meta["es"]]
    powers = case.inputs[2].t
    acc = None
    for i in range(1, d + 1):
        term = O.scal_1d(v.d, _pt_bytes([n], [q[e][i] for e in range(n)]), ct_bytes(E, powers[(i - 1) * n * CT:i * n * CT], n))
        acc = term if acc is None else O.add(v.d, acc, term)
    fm = O.scal_1d(v.d, _pt_bytes([n], [q[e][0] for e in range(n)]), P.serialize_ciphertext_tensor([n], [(P.identity(v.d), v.forms["f"])] * n))
    return O.add(v.d, acc, fm)


def want_div_close(v, E, case):
    eq = [DC.divfloor((abs(e), e < 0), D, v.k) for e, D in zip(case.meta["es"], case.meta["divs"])]
    return oracle_add_plain(v, E, case.inputs[2].t, case.meta["n"], eq)


def want_divx_close(v, E, case):
    n, rows = case.meta["n"], case.meta["rows"]
    qm = [DX.divmod_centred((abs(e), e < 0), D, v.k, rows) for e, D in zip(case.meta["es"], case.meta["divs"])]
    tuples = case.inputs[2].t.view(n, rows, CT)
    picked = v.torch.stack([tuples[i, qm[i][1]] for i in range(n)]).reshape(-1).contiguous()
    return oracle_add_plain(v, E, picked, n, [q for q, _ in qm])


def test_block_cache_temporaries_across_streams(v, holder):
    """poly_close_records, div_close_records and divx_close_records take their temporaries from the block cache and give them back
    behind their stream's work: alternately on A (behind the holder) and B, 4 rounds, inputs of their own on either stream, all
    against the plain-integer models (the Taylor shift, the floor division, the division with remainder) and the oracle"""
    E = v.E
    kinds = ((SC.b_poly_close, want_poly_close), (SC.b_div_close, want_div_close), (SC.b_divx_close, want_divx_close))
    cases = {(s, i): build(v, "", seed=1000 * (s + 1)) for s in (0, 1) for i, (build, _) in enumerate(kinds)}
    wants = {key: kinds[key[1]][1](v, E, case) for key, case in cases.items()}
    for case in cases.values():
        alone(v, E, case)                     # warm: the table of f
    holder.reset()
    v.torch.cuda.synchronize()
    with streams(E, 2) as (A, B):
        for rnd in range(4):
            runs = {key: Run(v, case) for key, case in cases.items()}
            v.torch.cuda.synchronize()
            if rnd == 0:
                holder.enqueue(E, A)
            for i in range(len(kinds)):
                for s, stream in ((0, A), (1, B)):
                    cases[s, i].call(E, runs[s, i].ptrs(), stream)
                    if rnd == 0 and i == 0 and s == 0:
                        busy(E, A)            # B's first allocation may be A's block, and then waits for A on the host
            E.stream_sync(A)
            E.stream_sync(B)
            for key, case in cases.items():
                assert ct_bytes(E, runs[key].result()[1][0], case.meta["n"]) == wants[key], (rnd, key)
    holder.check(E)


# ---- (e) the flag words -----------------------------------------------------------------------------------------------------------
# The ring has 256 words (ctx.hpp: N_FLAGS): at most 256 flag-using calls of one context may be in flight.  128 are here.

def test_flag_words_of_calls_in_flight(v):
    """64 add_ciphertext_records per stream at 33 ciphertexts, alternating, no host synchronisation: A adds operands that share
    their c1 (the folded route: the flag says "shared"), B operands whose last ciphertext alone differs in c1 (the flag says
    "distinct").  A flag word read by the wrong call folds a tensor that must not be folded, or the reverse"""
    import torch
    E = v.E
    n, rounds = 33, 64
    rnd = lambda seed: torch.tensor(random.Random(seed).choices(range(v.npool), k=n), dtype=torch.int64, device="cuda")      # noqa: E731
    fix = lambda i: torch.full((n,), i, dtype=torch.int64, device="cuda")      # noqa: E731
    last = fix(5)
    last[n - 1] = 7
    ops = {"A": [(v.tensor(torch, v.fw, fix(5), rnd(1 + j)), v.tensor(torch, v.fw, fix(11), rnd(3 + j))) for j in (0, 10)],
           "B": [(v.tensor(torch, v.fw, last, rnd(5 + j)), v.tensor(torch, v.fw, fix(11), rnd(7 + j))) for j in (0, 10)]}
    want = {key: [O.add(v.d, ct_bytes(E, a, n), ct_bytes(E, b, n)) for a, b in pairs] for key, pairs in ops.items()}
    outs = {key: [SC.zeros(v, n * CT) for _ in range(rounds)] for key in ops}
    torch.cuda.synchronize()
    with streams(E, 2) as (A, B):
        for r in range(rounds):
            for key, s in (("A", A), ("B", B)):
                a, b = ops[key][r % 2]
                E.add_ciphertext_records(a.data_ptr(), b.data_ptr(), outs[key][r].data_ptr(), n, stream=s)
        E.stream_sync(A)
        E.stream_sync(B)
    for key in ops:
        got = [ct_bytes(E, outs[key][r], n) for r in range(rounds)]
        for r in range(rounds):
            assert got[r] == want[key][r % 2], (key, r)


# ---- (f) two host threads, one context, a stream each -----------------------------------------------------------------------------

def test_two_host_threads_one_context(v):
    """each thread runs 8 rounds of part_decrypt (2), rerandomize (5), add (33), add_plain (5) on its own stream with its own
    inputs; ctypes drops the GIL for the length of a call.  Every output against oracle values computed before the threads start"""
    import torch
    E = v.E
    rounds = 8

    def work(t):
        seed = 2000 * (t + 1)
        pd, rr, ap = SC.b_part_decrypt(v, "", seed=seed, n=2), SC.b_rerandomize(v, "", seed=seed), SC.b_add_plain(v, "deterministic", seed=seed)
        a, b = SC.cts(v, 33, seed + 90), SC.cts(v, 33, seed + 95)
        want = [c1_powers(v, E, pd.inputs[0].t, 2, pd.meta["share"]), oracle_rerand(v, E, rr), O.add(v.d, ct_bytes(E, a, 33), ct_bytes(E, b, 33)),
                oracle_add_plain(v, E, ap.inputs[0].t, 5, [-m for m in ap.meta["ms"]])]
        outs = [[SC.zeros(v, w) for w in (2 * REC, 5 * CT, 33 * CT, 5 * CT)] for _ in range(rounds)]
        return pd, rr, ap, a, b, want, outs

    jobs = [work(t) for t in range(2)]
    for pd, rr, ap, *_ in jobs:
        for case in (rr, ap):
            alone(v, E, case)                 # warm: the tables of h, pk and f
    errors = []
    torch.cuda.synchronize()

    def body(job, stream):
        pd, rr, ap, a, b, _, outs = job
        r = v.recs
        try:
            for o in outs:
                E.part_decrypt_records(pd.inputs[0].t.data_ptr(), pd.inputs[1].t.data_ptr(), o[0].data_ptr(), 2, stream=stream)
                E.rerandomize_records(rr.inputs[0].t.data_ptr(), rr.inputs[1].t.data_ptr(), r["h"], r["pk"], o[1].data_ptr(), 5, stream=stream)
                E.add_ciphertext_records(a.data_ptr(), b.data_ptr(), o[2].data_ptr(), 33, stream=stream)
                E.add_plain_records(ap.inputs[0].t.data_ptr(), ap.inputs[1].t.data_ptr(), r["f"], o[3].data_ptr(), 5, v.k, 1, stream=stream)
            E.stream_sync(stream)
        except Exception as exc:              # noqa: BLE001 -- reported by the main thread
            errors.append(exc)

    with streams(E, 2) as ss:
        threads = [threading.Thread(target=body, args=(job, s)) for job, s in zip(jobs, ss)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    assert errors == []
    for t, (pd, rr, ap, a, b, want, outs) in enumerate(jobs):
        for rnd, o in enumerate(outs):
            got = [E.pdr_records_to_bytes(host(o[0]), [2]), ct_bytes(E, o[1], 5), ct_bytes(E, o[2], 33), ct_bytes(E, o[3], 5)]
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, (t, rnd, ("part_decrypt", "rerandomize", "add", "add_plain")[i])


# ---- (g) the life of a stream -----------------------------------------------------------------------------------------------------

def test_a_destroyed_stream_is_forgotten(v, holder):
    """a fresh context: the holder on A, then stream_destroy(A), which returns after the work.  New streams until one has A's
    handle value (16 tries at the most): a user of the workspace on it must not be taken for the workspace's last user, and must
    not wait for an event whose stream is gone"""
    case = SC.b_part_decrypt(v, "", seed=80)
    run = Run(v, case)
    holder.reset()
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E:
        A = E.stream_create(nonblocking=1)
        made = []
        try:
            holder.enqueue(E, A)
            busy(E, A)
        finally:
            E.stream_destroy(A)
        try:
            holder.check(E)                   # destroy returned after the work: no further synchronisation
            for _ in range(16):
                made.append(E.stream_create(nonblocking=1))
                if made[-1] == A:
                    break
                if len(made) == 3:
                    E.stream_destroy(made.pop(0))
            S = made[-1]
            reused = "the handle was reused" if S == A else "the handle was NOT reused in 16 tries: the wait was not put to the test"
            assert E.stream_query(S) == 0, reused
            run.ret = case.call(E, run.ptrs(), S)
            E.stream_sync(S)
            assert E.stream_query(S) == 0, reused
            got = E.pdr_records_to_bytes(host(run.result()[1][0]), [3])
            assert got == c1_powers(v, E, case.inputs[0].t, 3, case.meta["share"]), reused
            holder.check(E)
        finally:
            for s in made:
                E.stream_destroy(s)


def test_blocks_freed_behind_a_destroyed_stream_come_back(v):
    """a block freed behind a stream's work, the stream destroyed, the block taken again, four times over: the event the block
    cache kept named the destroyed stream, and cofhe_hip_malloc's wait for it came back as a stream-capture error of the HIP
    runtime (first seen in (a), whose cases run on a stream each) until stream_destroy let go of those events"""
    n = 3
    sz = n * REC * 4
    src = SC.forms(v, n, 9200)
    view = SC.identity_view(v, n)
    v.torch.cuda.synchronize()
    with fresh_engine(v) as E:
        for _ in range(4):
            p = E.malloc(sz)
            A = E.stream_create(nonblocking=1)
            try:
                E.view_records(view, src.data_ptr(), 0, p, REC, stream=A)
                E.free(p, stream=A)
            finally:
                E.stream_destroy(A)
            q = E.malloc(sz)
            assert q == p
            assert np.array_equal(E.download(q, sz), host(src))
            E.free(q)


def test_stream_entries_refuse_null_arguments(v):
    from cofhe_amd import engine as eng
    E, L = v.E, v.E.L
    s, b = C.c_void_p(), C.c_int(7)
    assert L.cofhe_hip_stream_create(None, 1, C.byref(s)) == eng.COFHE_HIP_EINVAL
    assert L.cofhe_hip_stream_create(E.ctx, 1, None) == eng.COFHE_HIP_EINVAL
    assert L.cofhe_hip_stream_destroy(None, None) == eng.COFHE_HIP_EINVAL
    assert L.cofhe_hip_stream_query(None, None, C.byref(b)) == eng.COFHE_HIP_EINVAL
    assert L.cofhe_hip_stream_query(E.ctx, None, None) == eng.COFHE_HIP_EINVAL
    assert s.value is None and b.value == 7
    assert L.cofhe_hip_stream_destroy(E.ctx, None) == 0          # null stream: nothing to do
    E.stream_destroy(0)
    assert E.stream_query(0) == 0                                 # the null stream, idle
    blocking = E.stream_create(nonblocking=0)
    try:
        assert blocking and E.stream_query(blocking) == 0
    finally:
        E.stream_destroy(blocking)
