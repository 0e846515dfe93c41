"""GPU: what every cofhe_hip_*_records entry point of cofhe_amd/csrc/abi.hip refuses (or accepts as empty) before it launches
anything, as a table: the return code and the text of cofhe_hip_last_error for each case, compared with
tests/golden/abi_refusals.json, which was recorded from the library before its host-side scaffold was folded into shared helpers.

Per entry: each pointer the entry tests null in turn at a count of 1, each output aliased to each input it is checked against,
the zero count with every pointer null, one case per range clause, and two precedence cases (a bad range together with a null
pointer, a null pointer together with an overlap) that pin the order of the checks.

A case is in the table only if the entry's code returns before any kernel launch: a pointer the entry accepts as null (d_r,
h_record and pk_record of add_plain_records, d_fill of the view entries) is not a case, entries without a null test have no null
cases, and no row has a fully valid argument set.  All device pointers are slots of one zero-filled allocation, the outputs at the
lowest addresses, so that an input whose size a range case inflates never reaches an output."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_json
from gpu_inputs import P, _device_status_stays_clear, engine  # noqa: F401
from test_gpu_fresh_randomness import setup

pytestmark = pytest.mark.gpu
GOLDEN = "abi_refusals.json"
SLOT = 1 << 16                               # bytes per device pointer: the largest valid tensor of the table has 5 376
K = 64
N36 = (1 << 36) + 1                          # one more item than the comb, the lookups and pow_dot take
N24 = (1 << 24) + 1                          # one more element than tuples of up to 4096 rows take
WORK = 1 << 40                               # beyond 2^31 - 1 workgroups of any kernel here
VIEW_BYTES = 8 + 8 * 8 * 2 + 8 * 8 + 4 * 8 * 8 + 8 * 8 * 2          # sizeof(cofhe_hip_view)


def O(name):
    return (name, "out")


def I(name):
    return (name, "in")


def H(name):
    return (name, "host")


def V(name, value):
    return (name, "val", value)


def G(name, **fields):
    """a cofhe_hip_conv2d_shape (11 fields) or cofhe_hip_conv2d_geometry (14) argument; never null but in its own null case"""
    return (name, "geom", fields)


SHAPE = dict(B=1, H=2, W=2, C=1, kh=1, kw=1, Co=1, sh=1, sw=1, ph=0, pw=0)
GEOM = dict(SHAPE, dh=1, dw=1, groups=1)
GEOM_ORDER = ("B", "H", "W", "C", "kh", "kw", "Co", "sh", "sw", "ph", "pw", "dh", "dw", "groups")

K_RANGES = [("k=0", dict(kbits=0)), ("k=640", dict(kbits=640))]
DIVX_RANGES = K_RANGES + [("rows=0", dict(rows=0)), ("rows=4097", dict(rows=4097)), ("n_div=0", dict(n_div=0)), ("n_div=2", dict(n_div=2)),
                          ("n", dict(n=N24))]
LUT_RANGES = [("bits=0", dict(bits=0)), ("bits=13", dict(bits=13)), ("n_tab=0", dict(n_tab=0)), ("n_tab=2", dict(n_tab=2))]
SPLINE_RANGES = K_RANGES + [("bits=0", dict(bits=0)), ("d=0", dict(d=0)), ("d=9", dict(d=9)), ("shift", dict(shift=K)),
                            ("tuple", dict(bits=12, d=1)), ("n_tab=0", dict(n_tab=0)), ("n_tab=2", dict(n_tab=2)), ("n", dict(n=N24))]
CMP_RANGES = K_RANGES + [("bits=1", dict(bits=1)), ("bits=65", dict(bits=65)), ("digit_bits=0", dict(digit_bits=0)),
                         ("digit_bits=9", dict(digit_bits=9)), ("digits=12", dict(bits=12, digit_bits=1)),
                         ("n", dict(n=(1 << 36) // (11 << 8) + 1))]
CONV_RANGES = [("sh=0", dict(sh=0)), ("pad", dict(ph=1)), ("filter", dict(kh=3))]
GROUP_RANGES = CONV_RANGES + [("dh=0", dict(dh=0)), ("groups=0", dict(groups=0)), ("groups=2", dict(groups=2))]

# name -> (arguments after ctx and before stream, the overrides of the zero count, the pointers the entry tests null,
#          the (output, input) pairs its overlap test covers, the range cases)
ENTRIES = {
    "validate_records": ([I("d_records"), V("n_records", 1), H("all_valid")], dict(n_records=0), ["all_valid"], [],
                         [("work", dict(n_records=WORK))]),
    "compose_records": ([I("d_a"), I("d_b"), O("d_out"), V("n", 1)], dict(n=0), [], [], [("work", dict(n=WORK))]),
    "compose_wide_records": ([I("d_a"), I("d_b"), O("d_out"), V("n", 1), V("reps", 1), H("fallbacks")], dict(n=0), [], [],
                             [("work", dict(n=1 << 31))]),
    "add_ciphertext_records": ([I("d_a"), I("d_b"), O("d_out"), V("n_ct", 1)], dict(n_ct=0), [], [], [("n", dict(n_ct=(1 << 40) + 1))]),
    "sub_ciphertext_records": ([I("d_a"), I("d_b"), O("d_out"), V("n_ct", 1)], dict(n_ct=0), [], [], [("n", dict(n_ct=(1 << 40) + 1))]),
    "invert_records": ([I("d_in"), O("d_out"), V("n_records", 1)], dict(n_records=0), ["d_in", "d_out"], [], []),
    "pow_records": ([I("d_base"), I("d_exp"), O("d_out"), V("n_ct", 1)], dict(n_ct=0), [], [], [("work", dict(n_ct=WORK))]),
    "pow_form_records": ([I("d_base"), I("d_exp"), O("d_out"), V("n_forms", 1)], dict(n_forms=0), [], [], [("work", dict(n_forms=WORK))]),
    "accumulate_records": ([I("d_x"), I("d_zero"), O("d_out"), V("n", 1), V("m", 1), V("p", 1)], dict(n=0), [], [],
                           [("work", dict(n=1 << 20, p=1 << 20))]),
    "scal_matmul_records": ([I("d_cts"), I("d_exp"), I("d_zero"), O("d_out"), V("n", 1), V("m", 1), V("p", 1)], dict(n=0), [], [],
                            [("work", dict(n=1 << 20, p=1 << 20))]),
    "part_decrypt_records": ([I("d_cts"), I("d_share"), O("d_out"), V("n_ct", 1)], dict(n_ct=0), [], [], []),
    "decrypt_records": ([I("d_cts"), I("d_sk"), H("f_record"), O("d_out"), V("n_ct", 1), V("kbits", K)], dict(n_ct=0), [], [], []),
    "encrypt_records": ([I("d_plain"), I("d_c1_pkr"), H("f_record"), O("d_out"), V("n_ct", 1), V("kbits", K)], dict(n_ct=0), [], [], []),
    "pow_fixed_base_records": ([V("n", 1), H("base_records"), H("exp_records"), O("d_out")], dict(n=0),
                               ["base_records", "exp_records", "d_out"], [], [("n=5", dict(n=5))]),
    "pow_fixed_base_many_records": ([H("base_record"), I("d_exps"), O("d_out"), V("n", 1)], dict(n=0), ["base_record", "d_exps", "d_out"], [],
                                    [("n", dict(n=N36))]),
    "encrypt_fresh_records": ([I("d_plain"), I("d_r"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"), V("n_ct", 1), V("kbits", K)],
                              dict(n_ct=0), ["d_plain", "d_r", "h_record", "pk_record", "f_record", "d_out"], [],
                              K_RANGES + [("n", dict(n_ct=N36))]),
    "rerandomize_records": ([I("d_cts"), I("d_r"), H("h_record"), H("pk_record"), O("d_out"), V("n_ct", 1)], dict(n_ct=0),
                            ["d_cts", "d_r", "h_record", "pk_record", "d_out"], [], [("n", dict(n_ct=N36))]),
    "add_plain_records": ([I("d_cts"), I("d_plain"), I("d_r"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"), V("n_ct", 1),
                           V("kbits", K), V("mode", 0)], dict(n_ct=0), ["d_cts", "d_plain", "f_record", "d_out"], [],
                          [("mode=3", dict(mode=3)), ("mode=-1", dict(mode=-1))] + K_RANGES + [("n", dict(n_ct=N36))]),
    "matmul_plain_ct_records": ([I("d_s"), I("d_cts"), I("d_zero"), O("d_out"), V("n", 1), V("m", 1), V("p", 1)], dict(n=0), [],
                                [("d_out", "d_cts"), ("d_out", "d_s"), ("d_out", "d_zero")], [("m=2^21", dict(m=1 << 21))]),
    "conv2d_plain_ct_records": ([I("d_w"), I("d_cts"), I("d_zero"), O("d_out"), G("shape", **SHAPE)], dict(Co=0), ["shape"],
                                [("d_out", "d_cts"), ("d_out", "d_w"), ("d_out", "d_zero")], CONV_RANGES),
    "conv2d_grouped_plain_ct_records": ([I("d_w"), I("d_cts"), I("d_zero"), O("d_out"), G("geometry", **GEOM)], dict(Co=0), ["geometry"],
                                        [("d_out", "d_cts"), ("d_out", "d_w"), ("d_out", "d_zero")], GROUP_RANGES),
    "sum_pool2d_records": ([I("d_cts"), I("d_zero"), O("d_out"), G("geometry", **GEOM)], dict(C=0), ["geometry"],
                           [("d_out", "d_cts"), ("d_out", "d_zero")], CONV_RANGES + [("dh=0", dict(dh=0))]),
    "matmul_plain_plain_records": ([I("d_a"), I("d_b"), O("d_out"), V("n", 1), V("m", 1), V("p", 1), V("kbits", K)], dict(n=0), [],
                                   [("d_out", "d_a"), ("d_out", "d_b")], K_RANGES + [("k=641", dict(kbits=641))]),
    "conv2d_plain_plain_records": ([I("d_img"), I("d_w"), O("d_out"), G("geometry", **GEOM), V("kbits", K)], dict(Co=0), ["geometry"],
                                   [("d_out", "d_img"), ("d_out", "d_w")],
                                   GROUP_RANGES + [("groups=C", dict(C=2, Co=2, groups=2))] + K_RANGES + [("k=641", dict(kbits=641))]),
    "conv2d_ct_filters_records": ([I("d_img_exps"), I("d_filters_cts"), I("d_zero"), O("d_out"), G("geometry", **GEOM)], dict(Co=0), ["geometry"],
                                  [("d_out", "d_img_exps"), ("d_out", "d_filters_cts"), ("d_out", "d_zero")],
                                  GROUP_RANGES + [("groups=C", dict(C=2, Co=2, groups=2))]),
    "pow_dot_records": ([I("d_bases"), I("d_exps"), O("d_out"), V("n_ct", 1), V("d", 1)], dict(n_ct=0), ["d_bases", "d_exps", "d_out"],
                        [("d_out", "d_bases"), ("d_out", "d_exps")], [("d=0", dict(d=0)), ("d=9", dict(d=9)), ("n", dict(n_ct=N36))]),
    "poly_shift_records": ([I("d_coef"), I("d_x"), O("d_q"), V("n", 1), V("d", 1), V("kbits", K)], dict(n=0), ["d_coef", "d_x", "d_q"],
                           [("d_q", "d_coef"), ("d_q", "d_x")], K_RANGES + [("k=641", dict(kbits=641)), ("d=9", dict(d=9)), ("work", dict(n=WORK))]),
    "poly_close_records": ([I("d_coef"), I("d_e"), I("d_powers"), H("f_record"), O("d_out"), V("n_ct", 1), V("d", 1), V("kbits", K)], dict(n_ct=0),
                           ["d_coef", "d_e", "d_powers", "f_record", "d_out"], [("d_out", "d_powers"), ("d_out", "d_coef"), ("d_out", "d_e")],
                           [("d=0", dict(d=0)), ("d=9", dict(d=9)), ("k=641", dict(kbits=641))] + K_RANGES + [("n", dict(n_ct=N36))]),
    "divfloor_plain_records": ([I("d_v"), I("d_div"), V("n_div", 1), O("d_q"), V("n", 1), V("kbits", K)], dict(n=0), ["d_v", "d_div", "d_q"],
                               [("d_q", "d_v"), ("d_q", "d_div")],
                               K_RANGES + [("n_div=0", dict(n_div=0)), ("n_div=2", dict(n_div=2)), ("work", dict(n=WORK))]),
    "div_close_records": ([I("d_e"), I("d_div"), V("n_div", 1), I("d_rq"), H("f_record"), O("d_out"), V("n_ct", 1), V("kbits", K)], dict(n_ct=0),
                          ["d_e", "d_div", "d_rq", "f_record", "d_out"], [("d_out", "d_rq"), ("d_out", "d_e"), ("d_out", "d_div")],
                          K_RANGES + [("n_div=0", dict(n_div=0)), ("n_div=2", dict(n_div=2)), ("n", dict(n_ct=N36))]),
    "divmod_plain_records": ([I("d_v"), I("d_div"), V("n_div", 1), O("d_q"), O("d_rem"), V("n", 1), V("rows", 2), V("kbits", K)], dict(n=0),
                             ["d_v", "d_div", "d_q", "d_rem"],
                             [("d_q", "d_v"), ("d_q", "d_div"), ("d_rem", "d_v"), ("d_rem", "d_div"), ("d_rem", "d_q")], DIVX_RANGES),
    "divx_rows_records": ([I("d_r"), I("d_div"), V("n_div", 1), O("d_out"), V("n", 1), V("rows", 2), V("kbits", K)], dict(n=0),
                          ["d_r", "d_div", "d_out"], [("d_out", "d_r"), ("d_out", "d_div")], DIVX_RANGES),
    "divx_tuples_records": ([I("d_r"), I("d_div"), V("n_div", 1), I("d_rho"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"), V("n", 1),
                             V("rows", 2), V("kbits", K)], dict(n=0), ["d_r", "d_div", "d_rho", "h_record", "pk_record", "f_record", "d_out"],
                            [("d_out", "d_r"), ("d_out", "d_div"), ("d_out", "d_rho")], DIVX_RANGES),
    "divx_close_records": ([I("d_e"), I("d_div"), V("n_div", 1), I("d_tuples"), V("rows", 2), H("f_record"), O("d_out"), V("n", 1), V("kbits", K)],
                           dict(n=0), ["d_e", "d_div", "d_tuples", "f_record", "d_out"],
                           [("d_out", "d_tuples"), ("d_out", "d_e"), ("d_out", "d_div")], DIVX_RANGES),
    "lut_rotate_records": ([I("d_table"), V("n_tab", 1), I("d_r"), O("d_out"), V("n", 1), V("bits", 1)], dict(n=0), ["d_table", "d_r", "d_out"],
                           [("d_out", "d_table"), ("d_out", "d_r")], LUT_RANGES + [("n", dict(n=N36))]),
    "lut_tuples_records": ([I("d_table"), V("n_tab", 1), I("d_r"), I("d_rho"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"), V("n", 1),
                            V("bits", 1), V("kbits", K)], dict(n=0), ["d_table", "d_r", "d_rho", "h_record", "pk_record", "f_record", "d_out"],
                           [("d_out", "d_table"), ("d_out", "d_r"), ("d_out", "d_rho")],
                           LUT_RANGES + [("bits>k", dict(bits=2, kbits=1)), ("k=0", dict(kbits=0)), ("k=640", dict(kbits=640)),
                                         ("n", dict(n=N36)), ("n 2^bits", dict(n=1 << 36))]),
    "lut_select_records": ([I("d_e"), I("d_tuples"), O("d_out"), V("n", 1), V("bits", 1)], dict(n=0), ["d_e", "d_tuples", "d_out"],
                           [("d_out", "d_e"), ("d_out", "d_tuples")], [("bits=0", dict(bits=0)), ("bits=13", dict(bits=13)), ("n", dict(n=N36))]),
    "view_records": ([("view", "view", [2]), I("d_src"), I("d_fill"), O("d_dst"), V("words", 4)], dict(view=[0]), ["view", "d_src", "d_dst"],
                     [("d_dst", "d_src"), ("d_dst", "d_fill")], [("words=0", dict(words=0))]),
    "gather_records": ([I("d_src"), V("n_src", 1), I("d_index"), I("d_fill"), O("d_dst"), V("n_out", 1), V("words", 4)], dict(n_out=0),
                       ["d_src", "d_index", "d_dst"], [("d_dst", "d_src"), ("d_dst", "d_index"), ("d_dst", "d_fill")],
                       [("words=0", dict(words=0)), ("n_src", dict(n_src=0xFFFFFFFF)), ("n_out", dict(n_out=(1 << 48) + 1))]),
    "spline_rows_records": ([I("d_pieces"), V("n_tab", 1), I("d_r"), O("d_out"), V("n", 1), V("bits", 1), V("shift", 0), V("d", 1), V("kbits", K)],
                            dict(n=0), ["d_pieces", "d_r", "d_out"], [("d_out", "d_pieces"), ("d_out", "d_r")], SPLINE_RANGES),
    "spline_tuples_records": ([I("d_pieces"), V("n_tab", 1), I("d_r"), I("d_rho"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"),
                               V("n", 1), V("bits", 1), V("shift", 0), V("d", 1), V("kbits", K)], dict(n=0),
                              ["d_pieces", "d_r", "d_rho", "h_record", "pk_record", "f_record", "d_out"],
                              [("d_out", "d_pieces"), ("d_out", "d_r"), ("d_out", "d_rho")], SPLINE_RANGES),
    "spline_powers_records": ([I("d_e"), O("d_out"), V("n", 1), V("d", 1), V("kbits", K)], dict(n=0), ["d_e", "d_out"], [("d_out", "d_e")],
                              K_RANGES + [("d=0", dict(d=0)), ("d=9", dict(d=9)), ("n", dict(n=N24))]),
    "spline_close_records": ([I("d_e"), I("d_tuples"), O("d_out"), V("n", 1), V("bits", 1), V("shift", 0), V("d", 1), V("kbits", K)], dict(n=0),
                             ["d_e", "d_tuples", "d_out"], [("d_out", "d_e"), ("d_out", "d_tuples")],
                             [r for r in SPLINE_RANGES if not r[0].startswith("n_tab")]),
    "cmp_rows_records": ([I("d_r"), O("d_out"), V("n", 1), V("bits", 2), V("digit_bits", 1), V("kbits", K)], dict(n=0), ["d_r", "d_out"],
                         [("d_out", "d_r")], CMP_RANGES),
    "cmp_tuples_records": ([I("d_r"), I("d_rho"), H("h_record"), H("pk_record"), H("f_record"), O("d_out"), V("n", 1), V("bits", 2),
                            V("digit_bits", 1), V("kbits", K)], dict(n=0), ["d_r", "d_rho", "h_record", "pk_record", "f_record", "d_out"],
                           [("d_out", "d_r"), ("d_out", "d_rho")], CMP_RANGES),
    "cmp_close_records": ([I("d_e"), I("d_tuples"), O("d_out"), O("d_wrap"), V("n", 1), V("bits", 2), V("digit_bits", 1), V("kbits", K)], dict(n=0),
                          ["d_e", "d_tuples", "d_out", "d_wrap"],
                          [("d_out", "d_e"), ("d_out", "d_tuples"), ("d_wrap", "d_e"), ("d_wrap", "d_tuples"), ("d_wrap", "d_out")], CMP_RANGES),
}


def cases_of(name):
    """[(case id, {argument: value or None}, {field overrides})]: what to null and what to override, on top of the valid base"""
    args, zero, nulls, aliases, ranges = ENTRIES[name]
    pointers = [a[0] for a in args if a[1] in ("in", "out", "host")]
    out = [("zero count, pointers null", {p: None for p in pointers}, zero)]
    out += [("null %s" % p, {p: None}, {}) for p in nulls]
    out += [("%s = %s" % (o, i), {o: i}, {}) for o, i in aliases]
    out += [("range %s" % label, {}, over) for label, over in ranges]
    if ranges and nulls:
        out.append(("range %s and null %s" % (ranges[0][0], nulls[0]), {nulls[0]: None}, ranges[0][1]))
    for p in nulls:
        pair = next(((o, i) for o, i in aliases if p not in (o, i)), None)
        if pair:
            out.append(("null %s and %s = %s" % (p, pair[0], pair[1]), {p: None, pair[0]: pair[1]}, {}))
            break
    return out


class Arena:
    """one zero-filled device allocation cut into slots, the outputs first; host records of zeros; one engine"""

    def __init__(self, E, torch):
        self.E = E
        self.buf = torch.zeros(16 * SLOT + 256, dtype=torch.uint8, device="cuda")
        self.base = (self.buf.data_ptr() + 255) & ~255
        self.host = np.zeros(4 * 168, dtype=np.uint32)
        self.keep = []

    def view(self, shape):
        v = C.create_string_buffer(VIEW_BYTES)
        ext, perm = (C.c_uint64 * 8)(*shape), (C.c_uint32 * 8)(*range(len(shape)))
        assert self.E.L.cofhe_hip_view_permute(ext, len(shape), perm, v) == 0
        return v

    def call(self, name, nulled, over):
        args = ENTRIES[name][0]
        slots = {a[0]: i for i, a in enumerate([a for a in args if a[1] == "out"] + [a for a in args if a[1] == "in"])}
        ptr = {}
        for a in args:
            if a[1] in ("in", "out"):
                ptr[a[0]] = self.base + slots[a[0]] * SLOT
            elif a[1] == "host":
                ptr[a[0]] = self.host.ctypes.data
        argv = []
        for a in args:
            nm, kind = a[0], a[1]
            if kind == "val":
                argv.append(over.get(nm, a[2]))
                continue
            if nm in nulled:
                argv.append(ptr[nulled[nm]] if nulled[nm] else None)
            elif kind == "geom":
                f = dict(a[2], **{k: v for k, v in over.items() if k in a[2]})
                g = (C.c_uint32 * len(f))(*[f[k] for k in GEOM_ORDER if k in f])
                self.keep.append(g)
                argv.append(C.addressof(g))
            elif kind == "view":
                v = self.view(over.get(nm, a[2]))
                self.keep.append(v)
                argv.append(C.addressof(v))
            else:
                argv.append(ptr[nm])
        fn = getattr(self.E.L, "cofhe_hip_" + name)
        rc = fn(self.E.ctx, *argv, None)
        return [rc, self.E.L.cofhe_hip_last_error().decode() if rc else ""]


@pytest.fixture(scope="module")
def arena():
    import torch
    E = engine(setup(load_json("params_tiny_k8.json"))[0])
    a = Arena(E, torch)
    yield a
    torch.cuda.synchronize()


def record(arena):
    """the whole table as the golden file holds it: {entry: {case: [return code, message]}}"""
    return {name: {cid: arena.call(name, nulled, over) for cid, nulled, over in cases_of(name)} for name in ENTRIES}


def test_table_covers_the_golden_file():
    want = load_json(GOLDEN)
    assert sorted(want) == sorted(ENTRIES)
    for name in ENTRIES:
        assert sorted(want[name]) == sorted(c[0] for c in cases_of(name)), name
        assert not any(rc == 0 and "zero count" not in cid for cid, (rc, _) in want[name].items()), "a row with a valid argument set: " + name


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refusals_match_the_recorded_table(arena, name):
    want = load_json(GOLDEN)[name]
    for cid, nulled, over in cases_of(name):
        assert arena.call(name, nulled, over) == want[cid], "%s: %s" % (name, cid)
