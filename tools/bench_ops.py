"""Per-operation timings of every entry point of the path, tensors resident in HBM (run through
gpurun; one JSON line per operation, copied to profiles/).  Sizes follow SURVEY.md section 8(d):
C2 matadd 128x128, C3 scal_matmul 256^3 (ramp exponents) and with 128-bit exponents (smaller n),
C5 matadd 1024x1024, 1-D scal with k-bit exponents, negation, decryption, threshold decryption,
accumulation of the ct x ct product.  --conv-only: only the depthwise convolution and the sum pooling, each against the
block-diagonal dense filter through the ungrouped entry (the way these layers were written before the convolution had groups),
the two alternating in one run; --out FILE also writes those lines to FILE.  --poly-only: only the polynomial evaluation, by the
same method: cofhe_hip_pow_dot_records against the ladders and additions it replaces, and the one-opened-value protocol against
chained Beaver products (through local_bench); written to profiles/r12_poly/poly_time.json, or to --out FILE.  --div-only: only
the division by public divisors: k_plain_divfloor alone from its "profile_kernels" spans, the closing step next to a decryption,
and the protocol through local_bench with the kernel's share of it; written to profiles/r13_div/div_time.json, or to --out FILE.
--lut-only: only the table lookups: k_lut_select next to a device-to-device copy of the same bytes, the parts of a ReLU over 256
elements (tuple generation, decryption, selection), and the protocol through local_bench next to the degree-3 polynomial of the
same run; written to profiles/r14_lut/lut_time.json, or to --out FILE.  --view-only: only the rearrangements of resident tensors:
k_view_records (identity, transpose, window taps) and k_gather_records next to k_lut_select and a device-to-device copy of the same
bytes; written to --out FILE when given."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench import SplitMix64, exp_records, form_record, hx

sys.path.insert(0, os.path.join(ROOT, "tests"))

from gpu_inputs import encrypt_tensor_gpu
from cofhe_amd import Engine

prm = json.load(open(os.path.join(ROOT, "tests/golden/params_s128_k128.json")))
K = prm["k"]
eng = Engine(hx(prm["delta"]))
dev = torch.device("cuda", 0)
rng = SplitMix64(7)
QUICK = "--quick" in sys.argv
SKIP = set(os.environ.get("OPS_SKIP", "").split(","))       # diagnostics: leave out "big" (1024x1024) and / or "k256"


def timed(fn, reps=1):
    fn()                                  # warm-up (also builds cached tables)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def emit(op, shape, sec, units, unit, **extra):
    d = {"op": op, "shape": shape, "ms": round(sec * 1e3, 3), "rate": round(units / sec, 1), "unit": unit}
    d.update(extra)
    print(json.dumps(d), flush=True)


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)


def fresh(n):
    return encrypt_tensor_gpu(eng, torch, prm, [rng.bits(K) for _ in range(n)], rng.bits(960), dev)


# ---- depthwise convolution and sum pooling against the block-diagonal dense filter -------------------------------------------
def conv_groups_ops(runs=5):
    """"conv2d_depthwise": a 3 x 3 depthwise layer over (1, 28, 28, 64), pad 1, int8 weights; "sum_pool2d": 2 x 2 windows at stride 2
    over the same image.  Each against the dense [kh, kw, C, C] filter that is zero outside the diagonal through
    conv2d_plain_ct_records without groups, which gives the same records (checked).  Alternating, `runs` windows each (a quarter of a second of calls
    or more per window) after a warm-up of both; the median and the extremes of each, and the ratio of the medians"""
    image = (1, 28, 28, 64)
    C_ = image[3]
    cts, zero = fresh(int(np.prod(image))), fresh(1)
    lines = []
    for op, kernel, stride, pad, ones in (("conv2d_depthwise", (3, 3), (1, 1), (1, 1), False), ("sum_pool2d", (2, 2), (2, 2), (0, 0), True)):
        taps = kernel[0] * kernel[1]
        wg = [1] * (taps * C_) if ones else [int(rng.bits(8)) - 128 for _ in range(taps * C_)]
        dense = [wg[t * C_ + co] if ci == co else 0 for t in range(taps) for ci in range(C_) for co in range(C_)]
        dwg, dwd = dev_i32(exp_records(wg)), dev_i32(exp_records(dense))
        ho, wo = eng.conv2d_out_shape(image, (*kernel, 1, C_), stride, pad, (1, 1), C_)
        out_g = torch.zeros(ho * wo * C_ * 336, dtype=torch.int32, device=dev)
        out_d = torch.zeros_like(out_g)
        if ones:
            grouped = lambda: eng.sum_pool2d_records(cts.data_ptr(), zero.data_ptr(), out_g.data_ptr(), image, kernel, stride, pad)  # noqa: E731
        else:
            grouped = lambda: eng.conv2d_plain_ct_records(dwg.data_ptr(), cts.data_ptr(), zero.data_ptr(), out_g.data_ptr(), image,  # noqa: E731
                                                          (*kernel, 1, C_), stride, pad, groups=C_)
        dense_fn = lambda: eng.conv2d_plain_ct_records(dwd.data_ptr(), cts.data_ptr(), zero.data_ptr(), out_d.data_ptr(), image,  # noqa: E731
                                                       (*kernel, C_, C_), stride, pad)
        for route in (0, 1, 2):
            eng.set_option("conv_route", route)
            grouped(), dense_fn()
            torch.cuda.synchronize()
            same = bool(torch.equal(out_g, out_d))
            # enough calls per timed window for a quarter of a second of work, from one call of each timed alone
            rg, rd = (max(3, int(0.25 / timed(fn)) + 1) for fn in (grouped, dense_fn))
            tg, td = [], []
            for _ in range(runs):
                tg.append(timed(grouped, reps=rg))
                td.append(timed(dense_fn, reps=rd))
            eng.set_option("conv_route", 0)
            med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
            d = {"op": op, "image": list(image), "kernel": list(kernel), "stride": list(stride), "pad": list(pad), "conv_route": route,
                 "grouped_ms": round(med(tg) * 1e3, 3), "grouped_ms_min_max": [round(min(tg) * 1e3, 3), round(max(tg) * 1e3, 3)],
                 "dense_block_diagonal_ms": round(med(td) * 1e3, 3), "dense_ms_min_max": [round(min(td) * 1e3, 3), round(max(td) * 1e3, 3)],
                 "dense_over_grouped": round(med(td) / med(tg), 3), "same_records": same, "runs": runs, "calls_per_window": [rg, rd], "device_status": eng.device_status()}
            print(json.dumps(d), flush=True)
            lines.append(d)
    return lines


if "--conv-only" in sys.argv:
    res = conv_groups_ops()
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0 if all(r["same_records"] and r["device_status"] == 0 for r in res) else 1)

# ---- polynomial evaluation: the shared-squarings ladder against the composed route, the protocol against chained products ----
def poly_ops(runs=5):
    """"pow_dot": cofhe_hip_pow_dot_records against d calls of cofhe_hip_pow_records plus d - 1 cofhe_hip_add_ciphertext_records on
    the same operands, E = 4096, d in {2, 4}, full k-bit exponents, equal output records (checked).  Alternating, `runs` windows
    each (a quarter of a second of calls or more per window) after a warm-up of both; the median and the extremes of each, and
    the ratio of the medians.  "poly_activation": the host harness's comparison of evaluate_polynomial_ciphertext_tensor
    (degree 3) with two chained multiply_ciphertext_tensors with direct differences, E = 256, single-key client (local_bench
    poly_activation 256 <runs> alternates the two in its own process and prints the line)"""
    import subprocess
    E = 4096
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = []
    for d in (2, 4):
        bases = torch.cat([fresh(E) for _ in range(d)]).contiguous()
        ex = dev_i32(exp_records([rng.bits(K) | (1 << (K - 1)) for _ in range(d * E)]))
        ct_bytes, ex_bytes = E * 336 * 4, E * 32 * 4
        out_d, out_c = torch.zeros(E * 336, dtype=torch.int32, device=dev), torch.zeros(E * 336, dtype=torch.int32, device=dev)
        terms = torch.zeros(d * E * 336, dtype=torch.int32, device=dev)

        def dot():
            eng.pow_dot_records(bases.data_ptr(), ex.data_ptr(), out_d.data_ptr(), E, d)

        def composed():
            for i in range(d):
                eng.pow_records(bases.data_ptr() + i * ct_bytes, ex.data_ptr() + i * ex_bytes, terms.data_ptr() + i * ct_bytes, E)
            eng.add_ciphertext_records(terms.data_ptr(), terms.data_ptr() + ct_bytes, out_c.data_ptr(), E)
            for i in range(2, d):
                eng.add_ciphertext_records(out_c.data_ptr(), terms.data_ptr() + i * ct_bytes, out_c.data_ptr(), E)

        dot(), composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_d, out_c))
        rd, rc = (max(3, int(0.25 / timed(fn)) + 1) for fn in (dot, composed))
        td, tc = [], []
        for _ in range(runs):
            td.append(timed(dot, reps=rd))
            tc.append(timed(composed, reps=rc))
        line = {"op": "pow_dot", "E": E, "d": d, "exponent_bits": K, "pow_dot_ms": round(med(td) * 1e3, 3),
                "pow_dot_ms_min_max": [round(min(td) * 1e3, 3), round(max(td) * 1e3, 3)], "composed_ms": round(med(tc) * 1e3, 3),
                "composed_ms_min_max": [round(min(tc) * 1e3, 3), round(max(tc) * 1e3, 3)], "composed_over_pow_dot": round(med(tc) / med(td), 3),
                "predicted_by_composition_count": round((d * (K + K / 3) + d - 1) / (K + d * K / 3), 2), "same_records": same, "runs": runs,
                "calls_per_window": [rd, rc], "device_status": eng.device_status()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del bases, ex, out_d, out_c, terms
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "poly_activation", "256", str(runs)], capture_output=True, text=True, cwd=os.environ.get("TMPDIR", "/tmp"))
    line = {"op": "poly_activation", "same_records": False, "device_status": 0, "exit_status": r.returncode}
    for ln in r.stdout.splitlines():
        if ln.startswith("compare_json: "):
            line.update(json.loads(ln[len("compare_json: "):]))
            line["same_records"] = bool(line.pop("agree")) and r.returncode == 0
    print(json.dumps(line), flush=True)
    lines.append(line)
    return lines


if "--poly-only" in sys.argv:
    res = poly_ops()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r12_poly", "poly_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    sys.exit(0 if all(r["same_records"] and r["device_status"] == 0 for r in res) else 1)

# ---- division by public divisors: the kernel alone, the closing step, the protocol ------------------------------------------
def div_ops(runs=5):
    """"plain_divfloor": k_plain_divfloor alone at E = 16384 and E = 256, k-bit numerators, divisors of 16 bits (the word route of
    mp_divrem) and of 64 bits (its long division), from the spans of "profile_kernels" (20 launches each after a warm-up) next
    to the wall clock of the call.  "div_close": cofhe_hip_div_close_records at E = 256 by the wall clock, its kernel's span, and
    cofhe_hip_decrypt_records over the same 256 ciphertexts for scale.  "divide": divide_ciphertext_tensor_by_plaintext over 256
    elements through the host harness, single-key client, pair generation and the decryption included (local_bench divide 256
    <runs> prints the line), and the share of it that the kernel's two launches (r_q of the pairs, e_q of the opened values) take"""
    import subprocess
    lines = []
    f_rec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
    kernel_ms = {}
    for E in (16384, 256):
        v = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
        q = torch.zeros(E * 32, dtype=torch.int32, device=dev)
        for dbits in (16, 64):
            dv = dev_i32(exp_records([rng.bits(dbits) | (1 << (dbits - 1))]))
            call = lambda: eng.divfloor_plain_records(v.data_ptr(), dv.data_ptr(), 1, q.data_ptr(), E, K)  # noqa: E731
            wall = timed(call, reps=20)
            eng.profile_read("k_plain_divfloor", clear=True)
            eng.set_option("profile_kernels", 1)
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            eng.set_option("profile_kernels", 0)
            ms, launches = eng.profile_read("k_plain_divfloor", clear=True)
            kernel_ms[(E, dbits)] = ms / launches
            line = {"op": "plain_divfloor", "E": E, "kbits": K, "divisor_bits": dbits, "kernel_ms": round(ms / launches, 4), "launches": launches,
                    "call_wall_ms": round(wall * 1e3, 4), "elements_per_s": round(E / (ms / launches) * 1e3, 1), "device_status": eng.device_status()}
            print(json.dumps(line), flush=True)
            lines.append(line)
    E = 256
    rq, out = fresh(E), torch.zeros(E * 336, dtype=torch.int32, device=dev)
    e = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
    dv = dev_i32(exp_records([7]))
    close = lambda: eng.div_close_records(e.data_ptr(), dv.data_ptr(), 1, rq.data_ptr(), f_rec, out.data_ptr(), E, K)  # noqa: E731
    t_close = [timed(close, reps=10) for _ in range(runs)]
    dsk = dev_i32(exp_records([hx(prm["sk"])]))
    pt = torch.zeros(E * ((K + 31) // 32 + 1), dtype=torch.int32, device=dev)
    t_dec = [timed(lambda: eng.decrypt_records(out.data_ptr(), dsk.data_ptr(), f_rec, pt.data_ptr(), E, K), reps=10) for _ in range(runs)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    line = {"op": "div_close", "E": E, "kbits": K, "div_close_ms": round(med(t_close) * 1e3, 3),
            "div_close_ms_min_max": [round(min(t_close) * 1e3, 3), round(max(t_close) * 1e3, 3)], "kernel_ms": round(kernel_ms[(E, 16)], 4),
            "kernel_share_of_close": round(kernel_ms[(E, 16)] / (med(t_close) * 1e3), 4), "decrypt_ms": round(med(t_dec) * 1e3, 3),
            "decrypt_ms_min_max": [round(min(t_dec) * 1e3, 3), round(max(t_dec) * 1e3, 3)], "runs": runs, "device_status": eng.device_status()}
    print(json.dumps(line), flush=True)
    lines.append(line)
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "divide", "256", str(runs)], capture_output=True, text=True, cwd=os.environ.get("TMPDIR", "/tmp"))
    line = {"op": "divide", "device_status": 0, "exit_status": r.returncode, "agree": "agree: yes" in r.stdout}
    for ln in r.stdout.splitlines():
        if ln.startswith("divide_json: "):
            line.update(json.loads(ln[len("divide_json: "):]))
            line["kernel_share_of_protocol"] = round(2 * kernel_ms[(256, 16)] / line["divide_ms"], 5)
    print(json.dumps(line), flush=True)
    lines.append(line)
    return lines


if "--div-only" in sys.argv:
    res = div_ops()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r13_div", "div_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    sys.exit(0 if all(r["device_status"] == 0 and r.get("exit_status", 0) == 0 and r.get("agree", True) for r in res) else 1)

# ---- table lookups: the selection next to a plain copy, the parts of a ReLU, the protocol ------------------------------------
def lut_ops(runs=5):
    """"lut_select": cofhe_hip_lut_select_records at E = 16384, b = 8 (a tuple buffer of E 2^b 1344 bytes = 5.6 GB of arbitrary
    words: the kernel moves bytes) next to a contiguous device-to-device copy of the same E 1344 bytes (torch's copy_ of a
    contiguous tensor, which is one hipMemcpyAsync), both by device events around 16 calls, alternating, `runs` windows each.
    Every call of a window reads another source: the select another set of opened values, the copy another slice of the tuple
    buffer, 16 x 22 MB in all, more than the 256 MiB Infinity Cache keeps.  "lut_select_large": the same buffer read as E = 262144
    elements at b = 4, 352 MB each way per call, 32 calls a window, where the time of a launch no longer shows.  "lut_rotate": the rows of 256 elements at b = 8.
    "relu_parts": the three device steps of a ReLU over 256 elements at b = 8 by the wall clock: the tuples (rotation and 65536
    fresh encryptions), the decryption of the 256 opened values, the selection.  "relu": relu_ciphertext_tensor over 256
    elements through the host harness (local_bench lookup 256 <runs>), and "poly_activation" the degree-3 polynomial over 256
    elements by the same harness in the same run"""
    import subprocess
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    lines = []
    f_rec, h_rec, pk_rec = (form_record(hx(prm[n]["a"]), hx(prm[n]["b"]), hx(prm[n]["c"])) for n in ("f", "h", "pk"))
    E, b, CTW, SETS = 16384, 8, 336, 16
    tuples = torch.empty((E << b) * CTW, dtype=torch.int32, device=dev).random_()
    es = [dev_i32(exp_records([rng.bits(K) for _ in range(E)])) for _ in range(SETS)]
    out, dst = torch.zeros(E * CTW, dtype=torch.int32, device=dev), torch.zeros(E * CTW, dtype=torch.int32, device=dev)
    srcs = [tuples[j * 16 * E * CTW:(j * 16 + 1) * E * CTW] for j in range(SETS)]      # 16 slices of E ciphertexts, 350 MB apart

    def window(fn):
        fn(0)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for j in range(SETS):
            fn(j)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / SETS

    sel = lambda j: eng.lut_select_records(es[j].data_ptr(), tuples.data_ptr(), out.data_ptr(), E, b)  # noqa: E731
    cpy = lambda j: dst.copy_(srcs[j])  # noqa: E731
    sel(3)
    torch.cuda.synchronize()
    # the opened values are below 2^k with sign word 0: the entry is word 0's low byte
    e3 = es[3].cpu().view(E, 32)[:, 0].to(torch.int64) & 255
    want = tuples.view(E << b, CTW)[(torch.arange(E) << b).to(dev) + e3.to(dev)]
    same = bool(torch.equal(out.view(E, CTW), want))
    del want
    ts, tc = [], []
    for _ in range(runs):
        ts.append(window(sel))
        tc.append(window(cpy))
    nbytes = E * CTW * 4
    line = {"op": "lut_select", "E": E, "bits": b, "bytes_moved_each_way": nbytes, "select_ms": round(med(ts), 4),
            "select_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "copy_ms": round(med(tc), 4),
            "copy_ms_min_max": [round(min(tc), 4), round(max(tc), 4)], "select_over_copy": round(med(ts) / med(tc), 3),
            "select_GB_per_s_read_plus_write": round(2 * nbytes / med(ts) / 1e6, 1), "same_records": same, "runs": runs, "calls_per_window": SETS,
            "device_status": eng.device_status()}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del srcs, out, dst, es
    # the same buffer read as 16 times the elements at b = 4: 352 MB each way per call, where a launch no longer shows
    E2, b2, SETS2 = E << 4, b - 4, 4
    es2 = []
    for _ in range(SETS2):
        rec = np.zeros((E2, 32), dtype=np.uint32)
        rec[:, :4] = np.random.default_rng(len(es2)).integers(0, 1 << 32, (E2, 4), dtype=np.uint64).astype(np.uint32)
        es2.append(dev_i32(rec.reshape(-1)))
    out, dst = torch.zeros(E2 * CTW, dtype=torch.int32, device=dev), torch.zeros(E2 * CTW, dtype=torch.int32, device=dev)
    srcs = [tuples[j * 4 * E2 * CTW:(j * 4 + 1) * E2 * CTW] for j in range(SETS2)]

    def window2(fn, rounds=8):
        fn(0)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for i in range(rounds * SETS2):
            fn(i % SETS2)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / (rounds * SETS2)

    sel2 = lambda j: eng.lut_select_records(es2[j].data_ptr(), tuples.data_ptr(), out.data_ptr(), E2, b2)  # noqa: E731
    cpy2 = lambda j: dst.copy_(srcs[j])  # noqa: E731
    ts, tc = [], []
    for _ in range(runs):
        ts.append(window2(sel2))
        tc.append(window2(cpy2))
    nbytes = E2 * CTW * 4
    line = {"op": "lut_select_large", "E": E2, "bits": b2, "bytes_moved_each_way": nbytes, "select_ms": round(med(ts), 4),
            "select_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "copy_ms": round(med(tc), 4),
            "copy_ms_min_max": [round(min(tc), 4), round(max(tc), 4)], "select_over_copy": round(med(ts) / med(tc), 3),
            "select_GB_per_s_read_plus_write": round(2 * nbytes / med(ts) / 1e6, 1), "copy_GB_per_s_read_plus_write": round(2 * nbytes / med(tc) / 1e6, 1),
            "runs": runs, "calls_per_window": 8 * SETS2, "device_status": eng.device_status()}
    print(json.dumps(line), flush=True)
    lines.append(line)
    del tuples, srcs, out, dst, es2
    E = 256
    table = dev_i32(exp_records([v if v < 128 else 0 for v in range(1 << b)]))
    r = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
    rho = dev_i32(exp_records([rng.bits(960) for _ in range(E << b)]))
    rows = torch.zeros((E << b) * 32, dtype=torch.int32, device=dev)
    tup = torch.zeros((E << b) * CTW, dtype=torch.int32, device=dev)
    out = torch.zeros(E * CTW, dtype=torch.int32, device=dev)
    e = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
    dsk = dev_i32(exp_records([hx(prm["sk"])]))
    pt = torch.zeros(E * ((K + 31) // 32 + 1), dtype=torch.int32, device=dev)
    t_rot = [timed(lambda: eng.lut_rotate_records(table.data_ptr(), 1, r.data_ptr(), rows.data_ptr(), E, b), reps=20) for _ in range(runs)]
    t_tup = [timed(lambda: eng.lut_tuples_records(table.data_ptr(), 1, r.data_ptr(), rho.data_ptr(), h_rec, pk_rec, f_rec, tup.data_ptr(), E, b, K),
                   reps=2) for _ in range(runs)]
    t_sel = [timed(lambda: eng.lut_select_records(e.data_ptr(), tup.data_ptr(), out.data_ptr(), E, b), reps=20) for _ in range(runs)]
    t_dec = [timed(lambda: eng.decrypt_records(out.data_ptr(), dsk.data_ptr(), f_rec, pt.data_ptr(), E, K), reps=5) for _ in range(runs)]
    line = {"op": "lut_rotate", "E": E, "bits": b, "rotate_ms": round(med(t_rot) * 1e3, 4), "runs": runs, "device_status": eng.device_status()}
    print(json.dumps(line), flush=True)
    lines.append(line)
    line = {"op": "relu_parts", "E": E, "bits": b, "kbits": K, "tuples_ms": round(med(t_tup) * 1e3, 3),
            "tuples_ms_min_max": [round(min(t_tup) * 1e3, 3), round(max(t_tup) * 1e3, 3)], "fresh_encryptions": E << b,
            "decrypt_ms": round(med(t_dec) * 1e3, 3), "decrypt_ms_min_max": [round(min(t_dec) * 1e3, 3), round(max(t_dec) * 1e3, 3)],
            "select_ms": round(med(t_sel) * 1e3, 4), "select_ms_min_max": [round(min(t_sel) * 1e3, 4), round(max(t_sel) * 1e3, 4)],
            "tuple_bytes": (E << b) * CTW * 4, "runs": runs, "device_status": eng.device_status()}
    print(json.dumps(line), flush=True)
    lines.append(line)
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    for mode, tag, op in (("lookup", "lookup_json: ", "relu"), ("poly_activation", "compare_json: ", "poly_activation")):
        p = subprocess.run([exe, mode, "256", str(runs)], capture_output=True, text=True, cwd=os.environ.get("TMPDIR", "/tmp"))
        line = {"op": op, "device_status": 0, "exit_status": p.returncode, "agree": "agree: yes" in p.stdout if mode == "lookup" else None}
        for ln in p.stdout.splitlines():
            if ln.startswith(tag):
                line.update(json.loads(ln[len(tag):]))
        print(json.dumps(line), flush=True)
        lines.append(line)
    return lines


if "--lut-only" in sys.argv:
    res = lut_ops()
    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "r14_lut", "lut_time.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1)
    sys.exit(0 if all(r["device_status"] == 0 and r.get("exit_status", 0) == 0 and r.get("agree") is not False and r.get("same_records", True)
                      for r in res) else 1)

# ---- rearranging resident tensors: k_view_records and k_gather_records next to k_lut_select and a copy --------------------------
def view_ops(runs=5):
    """"view_records" (an identity view, a 128 x 128 transpose and the 3 x 3 window taps with padding 1 of a 1 x 32 x 32 x 16 image)
    and "gather_records" (a random permutation) on 16384 ciphertexts of arbitrary words, each next to cofhe_hip_lut_select_records
    selecting the same number of ciphertexts (b = 1) and a contiguous device-to-device copy of the same output bytes, by device
    events around 16 calls, alternating, `runs` windows each.  Every call of a window reads another of 16 source buffers (352 MB
    in all, more than the Infinity Cache keeps)."""
    from cofhe_amd import engine as E_
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    E, CTW, SETS = 16384, 336, 16
    pool = torch.empty(SETS * 2 * E * CTW, dtype=torch.int32, device=dev).random_()        # also the b = 1 tuples of lut_select
    srcs = [pool[j * 2 * E * CTW:(j * 2 + 1) * E * CTW] for j in range(SETS)]
    fill = torch.empty(CTW, dtype=torch.int32, device=dev).random_()
    perm = np.random.default_rng(1).permutation(E).astype(np.uint32)
    dperm = dev_i32(perm)

    def window(fn):
        fn(0)
        torch.cuda.synchronize()
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for j in range(SETS):
            fn(j)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) / SETS

    def exps(n, seed):
        rec = np.zeros((n, 32), dtype=np.uint32)
        rec[:, 0] = np.random.default_rng(seed).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        return dev_i32(rec.reshape(-1))

    lines = []
    views = [("identity", E_.view_permute([E], [0])), ("transpose_128x128", E_.view_permute([128, 128], [1, 0])),
             ("window_taps_3x3_pad1_1x32x32x16", E_.view_window_taps((1, 32, 32, 16), (3, 3), (1, 1), (1, 1)))]
    cases = [("view_records", name, v, E_.view_check(v)[1]) for name, v in views] + [("gather_records", "random_permutation", None, E)]
    for op, name, v, n_out in cases:
        out, dst = torch.zeros(n_out * CTW, dtype=torch.int32, device=dev), torch.zeros(n_out * CTW, dtype=torch.int32, device=dev)
        reps = n_out // E                                    # the copy and the select move the same output bytes
        tup = pool if reps == 1 else torch.empty(2 * n_out * CTW, dtype=torch.int32, device=dev).random_()
        es = [exps(n_out, j) for j in range(4)]
        big = None if reps == 1 else [tup[(j % 2) * n_out * CTW:((j % 2) + 1) * n_out * CTW] for j in range(SETS)]
        if v is not None:
            run = lambda j: eng.view_records(v, srcs[j].data_ptr(), fill.data_ptr(), out.data_ptr(), CTW)  # noqa: E731
        else:
            run = lambda j: eng.gather_records(srcs[j].data_ptr(), E, dperm.data_ptr(), 0, out.data_ptr(), E, CTW)  # noqa: E731
        sel = lambda j: eng.lut_select_records(es[j % 4].data_ptr(), tup.data_ptr(), dst.data_ptr(), n_out, 1)  # noqa: E731
        cpy = (lambda j: dst.copy_(srcs[j])) if reps == 1 else (lambda j: dst.copy_(big[j]))  # noqa: E731
        run(3)
        torch.cuda.synchronize()
        if v is None:
            same = bool(torch.equal(out.view(E, CTW), srcs[3].view(E, CTW)[torch.from_numpy(perm.astype(np.int64)).to(dev)]))
        elif name == "identity":
            same = bool(torch.equal(out, srcs[3]))
        elif name.startswith("transpose"):
            same = bool(torch.equal(out.view(128, 128, CTW), srcs[3].view(128, 128, CTW).transpose(0, 1)))
        else:
            img = torch.nn.functional.pad(srcs[3].view(32, 32, 16, CTW), (0, 0, 0, 0, 1, 1, 1, 1))
            img[0, :], img[-1, :], img[:, 0], img[:, -1] = fill, fill, fill, fill
            same = all(bool(torch.equal(out.view(3, 3, 32, 32, 16, CTW)[dy, dx], img[dy:dy + 32, dx:dx + 32])) for dy in range(3) for dx in range(3))
        tv, ts, tc = [], [], []
        for _ in range(runs):
            tv.append(window(run))
            ts.append(window(sel))
            tc.append(window(cpy))
        nbytes = n_out * CTW * 4
        line = {"op": op, "case": name, "ciphertexts_out": n_out, "bytes_written": nbytes, "ms": round(med(tv), 4),
                "ms_min_max": [round(min(tv), 4), round(max(tv), 4)], "lut_select_ms": round(med(ts), 4),
                "lut_select_ms_min_max": [round(min(ts), 4), round(max(ts), 4)], "copy_ms": round(med(tc), 4),
                "copy_ms_min_max": [round(min(tc), 4), round(max(tc), 4)], "over_lut_select": round(med(tv) / med(ts), 3),
                "over_copy": round(med(tv) / med(tc), 3), "same_records": same, "runs": runs, "calls_per_window": SETS,
                "device_status": eng.device_status()}
        print(json.dumps(line), flush=True)
        lines.append(line)
        del out, dst, tup, es, big
    return lines


if "--view-only" in sys.argv:
    res = view_ops()
    if "--out" in sys.argv:
        path = sys.argv[sys.argv.index("--out") + 1]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as fh:
            json.dump(res, fh, indent=1)
    sys.exit(0 if all(r["device_status"] == 0 and r["same_records"] for r in res) else 1)

# ---- matadd C2 / C5 ---------------------------------------------------------------------------
for side in ((128,) if (QUICK or "big" in SKIP) else (128, 1024)):
    E = side * side
    a, b = fresh(E), fresh(E)
    out = torch.empty_like(a)
    sec = timed(lambda: eng.compose_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), 2 * E), reps=10)
    emit("add_ciphertext_tensors", [side, side], sec, E, "ciphertext-ops/s", kernel="k_compose_wg")
    # the ciphertext-level entry: both operands come from encrypt_tensor (one r each), so c1 o c1' is folded
    sec = timed(lambda: eng.add_ciphertext_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), E), reps=10)
    emit("add_ciphertext_tensors, shared c1 folded (cofhe_hip_add_ciphertext_records)", [side, side], sec, E, "ciphertext-ops/s",
         kernel="k_c1_distinct + k_add_ct + k_c1_spread")
    del a, b, out

# ---- C5's second parameter set: security 128, k = 256 (examples/node.cpp:33-34), |Delta| = 2344 bits ----
if not QUICK and "k256" not in SKIP:
    prm2 = json.load(open(os.path.join(ROOT, "tests/golden/params_s128_k256.json")))
    eng2 = Engine(hx(prm2["delta"]))
    E2 = 128 * 128
    a = encrypt_tensor_gpu(eng2, torch, prm2, [rng.bits(256) for _ in range(E2)], rng.bits(960), dev)
    b = encrypt_tensor_gpu(eng2, torch, prm2, [rng.bits(256) for _ in range(E2)], rng.bits(960), dev)
    out = torch.empty_like(a)
    sec = timed(lambda: eng2.compose_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), 2 * E2), reps=10)
    emit("add_ciphertext_tensors, k = 256 parameters", [128, 128], sec, E2, "ciphertext-ops/s", kernel="k_compose_wg",
         delta_bits=(-hx(prm2["delta"])).bit_length())
    del a, b, out
    if "big" not in SKIP:       # C5: 1024 x 1024 at the k = 256 parameter set
        E3 = 1024 * 1024
        a = encrypt_tensor_gpu(eng2, torch, prm2, [rng.bits(256) for _ in range(E3)], rng.bits(960), dev)
        b = encrypt_tensor_gpu(eng2, torch, prm2, [rng.bits(256) for _ in range(E3)], rng.bits(960), dev)
        out = torch.empty_like(a)
        sec = timed(lambda: eng2.compose_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), 2 * E3), reps=3)
        emit("add_ciphertext_tensors, k = 256 parameters (C5)", [1024, 1024], sec, E3, "ciphertext-ops/s", kernel="k_compose_wg")
        sec = timed(lambda: eng2.add_ciphertext_records(a.data_ptr(), b.data_ptr(), out.data_ptr(), E3), reps=3)
        emit("add_ciphertext_tensors, k = 256 parameters (C5), shared c1 folded", [1024, 1024], sec, E3, "ciphertext-ops/s")
        del a, b, out
    del eng2

# ---- PCIe-inclusive: serialised host bytes in, serialised host bytes out -------------------------
E = 128 * 128
a, b = fresh(E), fresh(E)
ha = eng.records_to_bytes(a.cpu().numpy().view(np.uint32), [128, 128])
hb = eng.records_to_bytes(b.cpu().numpy().view(np.uint32), [128, 128])
t0 = time.perf_counter()
for _ in range(3):
    hc = eng.add_ciphertext_tensors(ha, hb)
sec = (time.perf_counter() - t0) / 3
emit("add_ciphertext_tensors, host bytes in/out (PCIe + GPU (de)serialisation)", [128, 128], sec, E, "ciphertext-ops/s",
     bytes_in=len(ha) + len(hb), bytes_out=len(hc))
del a, b

# ---- 1-D scal with k-bit exponents, negation (2^k - 1) ------------------------------------------
E = 128 * 128
cts = fresh(E)
out = torch.empty_like(cts)
ex = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
sec = timed(lambda: eng.pow_records(cts.data_ptr(), ex.data_ptr(), out.data_ptr(), E))
emit("scal_ciphertext_tensors 1-D, %d-bit exponents" % K, [E], sec, E, "ciphertexts/s", kernel="k_pow")
ex = dev_i32(exp_records([(1 << K) - 1] * E))
sec = timed(lambda: eng.pow_records(cts.data_ptr(), ex.data_ptr(), out.data_ptr(), E))
emit("negate_ciphertext_tensor (exponent 2^k - 1)", [E], sec, E, "ciphertexts/s", kernel="k_pow")

# ---- differences, inverses and plaintext addends (affine.hip, the comb's kinds 3 and 4) -----------------
other = fresh(E)
sec = timed(lambda: eng.sub_ciphertext_records(cts.data_ptr(), other.data_ptr(), out.data_ptr(), E), reps=10)
emit("sub_ciphertext_tensors, shared c1 folded (cofhe_hip_sub_ciphertext_records)", [E], sec, E, "ciphertext-ops/s",
     kernel="k_c1_distinct + k_sub_ct + k_c1_spread")
sec = timed(lambda: eng.invert_records(cts.data_ptr(), out.data_ptr(), 2 * E), reps=10)
emit("invert_ciphertext_tensor (cofhe_hip_invert_records)", [E], sec, E, "ciphertexts/s", kernel="k_invert_records")
f_rec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
h_rec = form_record(hx(prm["h"]["a"]), hx(prm["h"]["b"]), hx(prm["h"]["c"]))
pk_rec = form_record(hx(prm["pk"]["a"]), hx(prm["pk"]["b"]), hx(prm["pk"]["c"]))
pm = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
sec = timed(lambda: eng.add_plain_records(cts.data_ptr(), pm.data_ptr(), f_rec, out.data_ptr(), E, K, 0), reps=3)
emit("add_plaintext_tensor (cofhe_hip_add_plain_records, no randomness)", [E], sec, E, "ciphertexts/s", kernel="k_comb_first + k_compose_pairs tree")
pr = dev_i32(exp_records([rng.bits(960) for _ in range(E)]))
sec = timed(lambda: eng.add_plain_records(cts.data_ptr(), pm.data_ptr(), f_rec, out.data_ptr(), E, K, 0, d_r=pr.data_ptr(), h_record=h_rec,
                                          pk_record=pk_rec), reps=3)
emit("add_plaintext_tensor with fresh randomness (cofhe_hip_add_plain_records, d_r)", [E], sec, E, "ciphertexts/s",
     kernel="k_comb_first + k_compose_pairs tree")
# the division by a public divisor: the signed floor division on exponent records alone, and the closing step on [r_q]
pdiv, pquot = dev_i32(exp_records([(1 << 64) + 13])), torch.zeros(E * 32, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.divfloor_plain_records(pm.data_ptr(), pdiv.data_ptr(), 1, pquot.data_ptr(), E, K), reps=10)
emit("divide_plaintext_tensor (cofhe_hip_divfloor_plain_records, 65-bit divisor)", [E], sec, E, "elements/s", kernel="k_plain_divfloor")
sec = timed(lambda: eng.div_close_records(pm.data_ptr(), pdiv.data_ptr(), 1, cts.data_ptr(), f_rec, out.data_ptr(), E, K), reps=3)
emit("div_close_ciphertext_tensor (cofhe_hip_div_close_records)", [E], sec, E, "ciphertexts/s",
     kernel="k_plain_divfloor + k_comb_first + k_compose_pairs tree")
del pdiv, pquot
# a table lookup at b = 4: the rows of the tuples and the closing copy (the tuples' ciphertexts: E 2^4 of arbitrary words)
lbits = 4
ltab, lrows = dev_i32(exp_records(list(range(1 << lbits)))), torch.zeros((E << lbits) * 32, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.lut_rotate_records(ltab.data_ptr(), 1, pm.data_ptr(), lrows.data_ptr(), E, lbits), reps=10)
emit("lut_rotate_plaintext_tensor (cofhe_hip_lut_rotate_records, b = 4)", [E, 1 << lbits], sec, E << lbits, "records/s", kernel="k_lut_rotate")
ltup = torch.empty((E << lbits) * 336, dtype=torch.int32, device=dev).random_()
sec = timed(lambda: eng.lut_select_records(pm.data_ptr(), ltup.data_ptr(), out.data_ptr(), E, lbits), reps=10)
emit("lut_select_ciphertext_tensor (cofhe_hip_lut_select_records, b = 4)", [E], sec, E, "ciphertexts/s", kernel="k_lut_select")
del ltab, lrows, ltup
ha, hb = (eng.records_to_bytes(t.cpu().numpy().view(np.uint32), [128, 128]) for t in (cts, other))
t0 = time.perf_counter()
hc = eng.sub_ciphertext_tensors(ha, hb)
emit("sub_ciphertext_tensors, host bytes in/out (cofhe_hip_sub_ciphertext_tensors_bytes)", [128, 128], time.perf_counter() - t0, E, "ciphertext-ops/s")
from gpu_inputs import _pt_bytes  # noqa: E402
hp_ = _pt_bytes([128, 128], [rng.bits(K) for _ in range(E)])
t0 = time.perf_counter()
hc = eng.add_plaintext_tensor(ha, hp_, f_rec, K, 0)
emit("add_plaintext_tensor, host bytes in/out (cofhe_hip_add_plaintext_tensor_bytes)", [128, 128], time.perf_counter() - t0, E, "ciphertext-ops/s")
del other, pm, pr, ha, hb, hc, hp_

# ---- encryption with given randomness (fixed-base f^m) --------------------------------------------
pl = dev_i32(exp_records([rng.bits(K) for _ in range(E)]))
fr_ = lambda o: form_record(hx(o["a"]), hx(o["b"]), hx(o["c"]))
hp = dev_i32(np.concatenate([fr_(prm["h"]), fr_(prm["pk"])]))       # stand-ins for h^r, pk^r
enc = torch.empty(E * 336, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.encrypt_records(pl.data_ptr(), hp.data_ptr(), fr_(prm["f"]), enc.data_ptr(), E, K))
emit("encrypt_tensor (h^r, pk^r given)", [E], sec, E, "ciphertexts/s", kernel="k_encrypt_select + k_gather_signed + k_compose_pairs tree + k_zip_ciphertexts")
# the whole call: h^r and pk^r through the fixed-base tables of the context (first use builds them), then k_encrypt
r_ex = exp_records([rng.bits(960)])
hp2 = torch.empty(2 * 168, dtype=torch.int32, device=dev)


def encrypt_whole():
    eng.pow_fixed_base_records(np.concatenate([fr_(prm["h"]), fr_(prm["pk"])]), np.concatenate([r_ex, r_ex]), hp2.data_ptr())
    eng.encrypt_records(pl.data_ptr(), hp2.data_ptr(), fr_(prm["f"]), enc.data_ptr(), E, K)


t0 = time.perf_counter()
encrypt_whole()
torch.cuda.synchronize()
first = time.perf_counter() - t0
sec = timed(encrypt_whole, reps=3)
emit("encrypt_tensor, whole call incl. h^r and pk^r (fixed-base tables)", [E], sec, E, "ciphertexts/s",
     kernel="fixed-base tree for h^r, pk^r + the element tree", first_call_ms=round(first * 1e3, 1),
     first_call_note="builds the tables h^(2^j), pk^(2^j): one chain of ~1000 squarings each (k_square_chain)")
for E1 in (1, 64):
    pl1 = dev_i32(exp_records([rng.bits(K) for _ in range(E1)]))
    enc1 = torch.empty(E1 * 336, dtype=torch.int32, device=dev)

    def enc_small():
        eng.pow_fixed_base_records(np.concatenate([fr_(prm["h"]), fr_(prm["pk"])]), np.concatenate([r_ex, r_ex]), hp2.data_ptr())
        eng.encrypt_records(pl1.data_ptr(), hp2.data_ptr(), fr_(prm["f"]), enc1.data_ptr(), E1, K)
    sec = timed(enc_small, reps=3)
    emit("encrypt_tensor, whole call incl. h^r and pk^r (fixed-base tables)", [E1], sec, E1, "ciphertexts/s")
del enc, pl

# ---- decryption / threshold decryption ---------------------------------------------------------
frec = form_record(hx(prm["f"]["a"]), hx(prm["f"]["b"]), hx(prm["f"]["c"]))
sk = hx(prm["sk"])
dsk = dev_i32(exp_records([sk]))
ow = (K + 31) // 32 + 1
pt = torch.zeros(E * ow, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.decrypt_records(cts.data_ptr(), dsk.data_ptr(), frec, pt.data_ptr(), E, K))
flags = pt.cpu().numpy().reshape(E, ow)[:, -1]
emit("decrypt_tensor", [E], sec, E, "ciphertexts/s", kernel="k_wnaf_digits + k_pow_shared + k_decrypt",
     error_flags=int(np.count_nonzero(flags)), first_flagged=[int(i) for i in np.nonzero(flags)[0][:8]], device_status=eng.device_status())
if np.count_nonzero(flags) and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
    bad = np.nonzero(flags)[0][:64]
    np.save(os.path.join(ROOT, "gpurun_out", "bad_cts.npy"), cts.cpu().numpy().view(np.uint32).reshape(E, 336)[bad])
    np.save(os.path.join(ROOT, "gpurun_out", "bad_idx.npy"), bad)
# 2-of-2 additive split of sk: s0 - s1 = sk
s1 = rng.bits(960)
s0 = sk + s1
parts = torch.zeros(2 * E * 168, dtype=torch.int32, device=dev)
d0, d1 = dev_i32(exp_records([s0])), dev_i32(exp_records([s1]))
sec = timed(lambda: eng.part_decrypt_records(cts.data_ptr(), d0.data_ptr(), parts.data_ptr(), E))
emit("part_decrypt_tensor", [E], sec, E, "ciphertexts/s", kernel="k_wnaf_digits + k_pow_shared")
eng.part_decrypt_records(cts.data_ptr(), d1.data_ptr(), parts.data_ptr() + E * 168 * 4, E)
pt2 = torch.zeros(E * ow, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.combine_part_decryptions_records(cts.data_ptr(), parts.data_ptr(), [1, -1], frec, pt2.data_ptr(), E, K))
emit("combine_part_decryption_results_tensor (2 parts)", [E], sec, E, "ciphertexts/s", kernel="k_decrypt")
emit("threshold == plain decryption", [E], 1.0, 1, "check", equal=bool(torch.equal(pt, pt2)))
del parts, pt, pt2

# ---- accumulation of the ct x ct matrix product -------------------------------------------------
n, m, p = 16, 64, 16
x = fresh(n * m * p)
zero = fresh(1)
acc = torch.empty(n * p * 336, dtype=torch.int32, device=dev)
sec = timed(lambda: eng.accumulate_records(x.data_ptr(), zero.data_ptr(), acc.data_ptr(), n, m, p))
emit("accumulate (ct x ct matmul)", [n, m, p], sec, n * m * p, "ciphertext-ops/s", kernel="k_compose_pairs (tree; k_accumulate chains for large n*p)")
del x, acc

# ---- plaintext-matrix x ciphertext-matrix: C3 ---------------------------------------------------
# (8, 64, 64) is the reference's own default shape (benchmarks/local.cpp: scal_matmul 8 64 64)
shapes = [(8, 64, 64, "ramp"), (64, 64, 64, "ramp")] if QUICK else [(8, 64, 64, "ramp"), (64, 64, 64, "ramp"), (256, 256, 256, "ramp"), (32, 256, 256, "k-bit")]
for (n, m, p, kind) in shapes:
    cts = fresh(n * m)
    if kind == "ramp":
        evals = [j * p + k + 1 for j in range(m) for k in range(p)]       # benchmarks/local.cpp:171-174
    else:
        evals = [rng.bits(K) for _ in range(m * p)]
    ex = dev_i32(exp_records(evals))
    out = torch.empty(n * p * 336, dtype=torch.int32, device=dev)
    sec = timed(lambda: eng.scal_matmul_records(cts.data_ptr(), ex.data_ptr(), zero.data_ptr(), out.data_ptr(), n, m, p))
    emit("scal_ciphertext_tensors 2-D, %s exponents" % kind, [n, m, p], sec, n * p, "output-ciphertexts/s",
         macs_per_s=round(n * m * p / sec, 1), kernel="k_wnaf_digits + k_pow_table + k_scal_matmul_wnaf")
    del cts, out

# ---- depthwise convolution, sum pooling -----------------------------------------------------------
conv_groups_ops(runs=3)
