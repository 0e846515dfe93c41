"""The convolution's two routes, measured: "conv_route" 1 (direct: one table over the image, level 0 reads its leaves from it)
against 2 (gather: the patch matrix written out, then the matrix product unchanged -- the baseline, which is the workaround a
caller had before).  HIP events on the launch stream (Engine.time_stream), one warm-up, the median of RUNS runs with minimum
and maximum; each (case, route) in a process of its own, so that neither the block cache nor the grow-only workspace of one
run is there for the next.  Weights: 8-bit, and k-bit (the Beaver-style case, where the table dominates).  "same" padding,
stride 1.

Recorded next to the time: the window width (pinned to what the library's cost model gives for the route, so that the plan
below is the one that ran), the workspace total of that plan (cofhe_hip_workspace_plan "conv2d" / "scal_matmul_tree"), the
patch buffer of the gather route, and the device memory the process holds after the runs beyond what it held before them
(workspace + block cache: the level buffers, the patch matrix).

    python tools/gpu_conv_time.py [--out profiles/r10_conv] [--cases 1x32x32x16:3x3x16:8,...] [--runs 5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CT_BYTES = 2 * 168 * 4
DEFAULT_CASES = "1x32x32x16:3x3x16:8,1x32x32x16:3x3x16:k,8x28x28x32:3x3x32:8,8x28x28x32:3x3x32:k"


def model_width(uses, bits):
    """the library's choice (abi.hip: wnaf_auto_width) while the tables fit: minimise 2^(w-2) + uses bits / (w + 1)"""
    best, w = uses * bits / 3.0, 2
    for cand in range(3, 9):
        cost = (1 << (cand - 2)) + uses * bits / (cand + 1.0)
        if cost < best:
            best, w = cost, cand
    return w


def child(case, route, runs):
    import numpy as np
    import torch
    from bench import SplitMix64, exp_records, hx
    from cofhe_amd import Engine, engine
    from gpu_inputs import encrypt_tensor_gpu
    img, ker, bits = case.split(":")
    B, H, W, Cin = (int(v) for v in img.split("x"))
    kh, kw, Co = (int(v) for v in ker.split("x"))
    torch.cuda.init()
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k = prm["k"]
    nbits = k if bits == "k" else int(bits)
    E = Engine(hx(prm["delta"]))
    dev = torch.device("cuda", 0)
    rng = SplitMix64(1010)
    image, filters, stride, pad = (B, H, W, Cin), (kh, kw, Cin, Co), (1, 1), (kh // 2, kw // 2)
    ho, wo = engine.conv2d_out_shape(image, filters, stride, pad)
    n, m, p = B * ho * wo, kh * kw * Cin, Co
    cts = encrypt_tensor_gpu(E, torch, prm, [rng.bits(k) for _ in range(B * H * W * Cin)], rng.bits(960), dev)
    zero = encrypt_tensor_gpu(E, torch, prm, [0], rng.bits(960), dev)
    wv = [(rng.bits(nbits) | (1 << (nbits - 1))) * (1 if rng.bits(1) else -1) for _ in range(m * p)]
    dw = torch.from_numpy(exp_records(wv).view(np.int32)).to(dev)
    out = torch.zeros(n * p * 336, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    reuse = -(-kh // stride[0]) * -(-kw // stride[1])
    w = model_width(reuse * p if route == 1 else p, nbits)
    E.set_option("conv_route", route)
    E.set_option("wnaf_width", w)
    E.set_option("profile_kernels", 1)
    free0 = torch.cuda.mem_get_info()[0]
    fn = lambda: E.conv2d_plain_ct_records(dw.data_ptr(), cts.data_ptr(), zero.data_ptr(), out.data_ptr(), image, filters, stride, pad)      # noqa: E731
    fn()
    E.stream_sync()
    spans = {name: E.profile_read(name)[1] for name in ("k_conv_level0", "k_gather_patches", "k_tree_level", "k_pow_table")}
    E.profile_read("k_conv_level0", clear=True)
    E.set_option("profile_kernels", 0)
    ts = [E.time_stream(fn) for _ in range(runs)]
    held = free0 - torch.cuda.mem_get_info()[0]
    plan = engine.workspace_plan("conv2d", B, H, W, Cin, kh, kw, Co, *stride, *pad, nbits, w) if route == 1 else \
        engine.workspace_plan("scal_matmul_tree", n, m, p, nbits, w)
    res = {"case": case, "route": "direct" if route == 1 else "gather", "n_m_p": [n, m, p], "weight_bits": nbits, "wnaf_width": w,
           "ms": [round(statistics.median(ts), 3), round(min(ts), 3), round(max(ts), 3)], "runs": runs,
           "workspace_plan_bytes": plan[1], "table_bytes": plan[0][0][2], "patch_buffer_bytes": 0 if route == 1 else n * m * CT_BYTES,
           "device_bytes_held_after": int(held), "spans_of_one_call": spans, "device_status": E.device_status(clear=True),
           "checksum": int(out.to(torch.int64).sum().item())}
    print("RESULT " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_conv"))
    ap.add_argument("--cases", default=DEFAULT_CASES)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--child", nargs=2, metavar=("CASE", "ROUTE"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], int(a.child[1]), a.runs)
        return
    os.makedirs(a.out, exist_ok=True)
    res = {"statistic": "median [min, max] ms of RUNS runs after a warm-up, HIP events on the launch stream, one process per (case, route)", "cases": []}
    ok = True
    for case in a.cases.split(","):
        for route in (1, 2):
            if not ok:
                break
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, str(route), "--runs", str(a.runs)], capture_output=True,
                               text=True, timeout=900)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
            if r.returncode != 0 or not line:             # a failed child: nothing more is started on the GPU
                res["cases"].append({"case": case, "route": route, "exit": r.returncode, "stderr": r.stderr[-2000:]})
                ok = False
                break
            res["cases"].append(json.loads(line[0][7:]))
            print(line[0][7:], flush=True)
    by = {}
    for c in res["cases"]:
        if "ms" in c:
            by.setdefault(c["case"], {})[c["route"]] = c
    res["summary"] = {case: {"direct_over_gather_time": round(v["direct"]["ms"][0] / v["gather"]["ms"][0], 3),
                             "same_output": v["direct"]["checksum"] == v["gather"]["checksum"]}
                      for case, v in by.items() if len(v) == 2}
    with open(os.path.join(a.out, "conv_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res["summary"]))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
