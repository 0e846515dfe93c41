"""The plaintext-left matrix product and the matrix Beaver triplets, measured.

1. Transpose overhead: cofhe_hip_matmul_plain_ct_records (s n x m, cts m x p) against cofhe_hip_scal_matmul_records on the
   operands already transposed -- the very product the former runs between its three transposes.  HIP events on the launch
   stream (Engine.time_stream), one warm-up per side, the median of RUNS runs with minimum and maximum, the sides alternated
   in one process.  The bytes the three transposes move are recorded, and the largest of the three is timed alone: the call
   with an inner dimension of zero fills out^T with Enc(0) and transposes it.
2. Matrix flow against element flow of the ciphertext x ciphertext matrix product: local_bench ciphertext_matmul_matrix runs
   both on the same inputs and prints the opened values and the host wall clock of each; the counts 2 n m p and n m + m p are
   recorded next to the times.

    python tools/gpu_matmul_left_time.py [--out profiles/r09_matmul_left] [--sizes 64x64x64,256x256x256] [--flows 8,16]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import SplitMix64, exp_records, hx  # noqa: E402
from cofhe_amd import Engine  # noqa: E402
from gpu_inputs import encrypt_tensor_gpu  # noqa: E402

RUNS = 5
CT_BYTES, EXP_BYTES = 2 * 168 * 4, 32 * 4


def stats(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def transpose_overhead(E, prm, sizes):
    k = prm["k"]
    rng = SplitMix64(909)
    dev = torch.device("cuda", 0)
    P = lambda t: t.data_ptr()      # noqa: E731
    out = {}
    for n, m, p in sizes:
        cts = encrypt_tensor_gpu(E, torch, prm, [rng.bits(k) for _ in range(m * p)], rng.bits(960), dev)          # m x p
        zero = encrypt_tensor_gpu(E, torch, prm, [0], rng.bits(960), dev)
        s_host = exp_records([rng.bits(k) for _ in range(n * m)]).reshape(n, m, 32)                               # n x m
        s = torch.from_numpy(np.ascontiguousarray(s_host).view(np.int32)).to(dev)
        # the operands of the ciphertext-left call: cts^T (p x m) and s^T (m x n), transposed here once, outside the timing
        cts_t = cts.view(m, p, 336).transpose(0, 1).contiguous()
        s_t = s.view(n, m, 32).transpose(0, 1).contiguous()
        res_l = torch.zeros(n * p * 336, dtype=torch.int32, device=dev)
        res_r = torch.zeros_like(res_l)
        sides = {"plain_left": lambda: E.matmul_plain_ct_records(P(s), P(cts), P(zero), P(res_l), n, m, p),
                 "ct_left_on_transposed": lambda: E.scal_matmul_records(P(cts_t), P(s_t), P(zero), P(res_r), p, m, n)}
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        same = torch.equal(res_l.view(n, p, 336), res_r.view(p, n, 336).transpose(0, 1))
        ts = {name: [] for name in sides}
        for _ in range(RUNS):
            for name, fn in sides.items():
                ts[name].append(E.time_stream(fn))
        one = {name: stats(v) for name, v in ts.items()}
        # reads + writes of the three transposes: 2 m p and 2 n p form records, n m exponent records
        one["transposed_bytes"] = 2 * (CT_BYTES * (m * p + n * p) + EXP_BYTES * n * m)
        one["zero_fill_and_result_transpose_alone"] = stats([E.time_stream(lambda: E.matmul_plain_ct_records(0, 0, P(zero), P(res_l), n, 0, p))
                                               for _ in range(RUNS + 1)][1:])
        lo, hi = one["ct_left_on_transposed"][1], one["ct_left_on_transposed"][2]
        one["plain_left_median_within_ct_left_spread"] = bool(lo <= one["plain_left"][0] <= hi)
        one["outputs_equal"] = bool(same)
        out["%dx%dx%d" % (n, m, p)] = one
        print("%dx%d . %dx%d: %s  status %d" % (n, m, m, p, json.dumps(one), E.device_status(clear=True)), flush=True)
        del cts, cts_t, s, s_t, res_l, res_r
        torch.cuda.empty_cache()
    return out


def flows(sizes, out_dir):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    res = {}
    for n in sizes:
        r = subprocess.run([exe, "ciphertext_matmul_matrix", str(n), str(n), str(n)], cwd=out_dir, capture_output=True, text=True, timeout=300)
        got = {f: (int(c), float(ms)) for f, c, ms in re.findall(r"(element|matrix) flow: decrypted_elements (\d+), ([0-9.e+-]+) ms", r.stdout)}
        one = {"exit": r.returncode, "agree": "agree: yes" in r.stdout,
               "predicted_opened": {"element": 2 * n ** 3, "matrix": 2 * n * n}}
        for f, (c, ms) in got.items():
            one[f] = {"opened": c, "wall_ms": round(ms, 2)}
        if len(got) == 2 and got["matrix"][1] > 0:
            one["time_ratio_element_over_matrix"] = round(got["element"][1] / got["matrix"][1], 2)
            one["opened_ratio_element_over_matrix"] = round(got["element"][0] / got["matrix"][0], 2)
        res["%dx%dx%d" % (n, n, n)] = one
        print("flows %d^3: %s" % (n, json.dumps(one)), flush=True)
        if r.returncode != 0:                    # a failed child: nothing more is started on the GPU
            one["stderr"] = r.stderr[-2000:]
            break
    for name in ("local_bench_absdelta.txt",):
        try:
            os.remove(os.path.join(out_dir, name))
        except OSError:
            pass
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_matmul_left"))
    ap.add_argument("--sizes", default="64x64x64,256x256x256")
    ap.add_argument("--flows", default="8,16")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    res = {"runs": RUNS, "statistic": "median [min, max] ms, HIP events on the launch stream, sides alternated"}
    if a.flows:
        res["flows"] = flows([int(x) for x in a.flows.split(",")], a.out)          # child processes first: nothing else holds the GPU
    if a.sizes and all(one["exit"] == 0 for one in res.get("flows", {}).values()):
        torch.cuda.init()
        prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
        E = Engine(hx(prm["delta"]))
        res["params"] = prm["name"]
        res["transpose_overhead"] = transpose_overhead(E, prm, [tuple(int(v) for v in x.split("x")) for x in a.sizes.split(",")])
        res["device_status"] = E.device_status(clear=True)
    with open(os.path.join(a.out, "matmul_left_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
