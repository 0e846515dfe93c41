"""The convolution with ciphertext filters, measured.

1. Gather against transposition: cofhe_hip_conv2d_ct_filters_records (plaintext image, ciphertext filters) against
   cofhe_hip_matmul_plain_ct_records on the patch matrix of the same layer, gathered on the host outside the timing -- the same
   product, with the n x m exponent matrix transposed on the device instead of written transposed in the first place.  HIP events
   on the launch stream (Engine.time_stream), one warm-up per side, the median of RUNS runs with minimum and maximum, the sides
   alternated in one process; the outputs are compared.
2. The whole flow: local_bench conv2d_ciphertext on the layer with `--flow-runs` timed passes; its conv2d_ciphertext_json line
   (triplet generation, opening, the three closing terms, the total) is recorded next to the opened-value counts.

    python tools/gpu_conv_ct_time.py [--out profiles/conv_ct] [--layer 1x32x32x16,3x3,32,1] [--flow-runs 3]
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
from conv_cases import im2col, out_extents  # noqa: E402
from gpu_inputs import encrypt_tensor_gpu  # noqa: E402

RUNS = 5


def stats(v):
    return [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)]


def gather_against_transpose(E, prm, image, kernel, co, pad):
    k = prm["k"]
    rng = SplitMix64(1212)
    dev = torch.device("cuda", 0)
    P = lambda t: t.data_ptr()      # noqa: E731
    stride = (1, 1)
    ho, wo = out_extents(image, kernel, stride, pad)
    n, m, p = image[0] * ho * wo, kernel[0] * kernel[1] * image[3], co
    filters = (kernel[0], kernel[1], image[3], co)
    cts = encrypt_tensor_gpu(E, torch, prm, [rng.bits(k) for _ in range(m * p)], rng.bits(960), dev)              # [kh, kw, C, Co] = m x p
    zero = encrypt_tensor_gpu(E, torch, prm, [0], rng.bits(960), dev)
    img_host = exp_records([rng.bits(k) for _ in range(int(np.prod(image)))]).reshape(-1, 32)
    idx = im2col(image, kernel, stride, pad).reshape(-1)                                                        # n m pixel indices, -1: padding
    patch_host = np.where((idx >= 0)[:, None], img_host[np.maximum(idx, 0)], 0).astype(np.uint32)
    img = torch.from_numpy(np.ascontiguousarray(img_host).view(np.int32)).to(dev)
    patches = torch.from_numpy(np.ascontiguousarray(patch_host).view(np.int32)).to(dev)
    res_c = torch.zeros(n * p * 336, dtype=torch.int32, device=dev)
    res_m = torch.zeros_like(res_c)
    sides = {"conv2d_ct_filters": lambda: E.conv2d_ct_filters_records(P(img), P(cts), P(zero), P(res_c), image, filters, stride, pad),
             "matmul_plain_ct_on_gathered_patches": lambda: E.matmul_plain_ct_records(P(patches), P(cts), P(zero), P(res_m), n, m, p)}
    for fn in sides.values():
        fn()
    torch.cuda.synchronize()
    same = torch.equal(res_c, res_m)
    ts = {name: [] for name in sides}
    for run in range(RUNS):
        for name in (list(sides) if run % 2 == 0 else list(sides)[::-1]):      # neither side always runs behind the other
            ts[name].append(E.time_stream(sides[name]))
    one = {name: stats(v) for name, v in ts.items()}
    # the gather on its own, from the kernel's span (the transpositions it stands in for carry none)
    E.profile_read("k_gather_patch_exponents", clear=True)
    E.set_option("profile_kernels", 1)
    sides["conv2d_ct_filters"]()
    torch.cuda.synchronize()
    one["k_gather_patch_exponents_ms"] = round(E.profile_read("k_gather_patch_exponents")[0], 4)
    E.set_option("profile_kernels", 0)
    E.profile_read("k_gather_patch_exponents", clear=True)
    one.update({"n": n, "m": m, "p": p, "outputs_equal": bool(same),
                "padding_fraction_of_patch_matrix": round(float((idx < 0).mean()), 4)})
    return one


def flow(layer_args, runs, out_dir):
    exe = os.path.join(ROOT, "cofhe_amd", "host", "local_bench")
    r = subprocess.run([exe, "conv2d_ciphertext", *layer_args, "0", "3", str(runs)], cwd=out_dir, capture_output=True, text=True, timeout=900)
    one = {"exit": r.returncode, "agree": "agree: yes" in r.stdout}
    got = re.search(r"conv2d_ciphertext_json: (\{.*\})", r.stdout)
    if got:
        one["phases"] = json.loads(got.group(1))
    counts = re.search(r"2 n m p = (\d+) .* n m \+ m p = (\d+) ", r.stdout)
    if counts:
        one["element_triplets_would_open"], one["matrix_triplet_would_open"] = int(counts.group(1)), int(counts.group(2))
    if r.returncode != 0:
        one["stderr"] = r.stderr[-2000:]
    for name in os.listdir(out_dir):
        if name.startswith("local_bench_cconv_") or name == "local_bench_absdelta.txt":
            os.remove(os.path.join(out_dir, name))
    return one


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_ct"))
    ap.add_argument("--layer", default="1x32x32x16,3x3,32,1", help="image BxHxWxC, kernel khxkw, Co, pad (both axes); stride 1")
    ap.add_argument("--flow-runs", type=int, default=3)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    img_s, ker_s, co_s, pad_s = a.layer.split(",")
    image, kernel, co, pad = tuple(int(v) for v in img_s.split("x")), tuple(int(v) for v in ker_s.split("x")), int(co_s), int(pad_s)
    res = {"layer": a.layer, "runs": RUNS, "statistic": "median [min, max] ms, HIP events on the launch stream, sides alternated"}
    if a.flow_runs:
        # the child process first: nothing else holds the GPU
        args = [str(v) for v in (*image, *kernel, co, 1, 1, pad, pad, 1, 1)]
        res["flow"] = flow(args, a.flow_runs, a.out)
    if res.get("flow", {"exit": 0})["exit"] == 0:
        torch.cuda.init()
        prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
        E = Engine(hx(prm["delta"]))
        res["params"] = prm["name"]
        res["gather_against_transpose"] = gather_against_transpose(E, prm, image, kernel, co, (pad, pad))
        res["device_status"] = E.device_status(clear=True)
    with open(os.path.join(a.out, "conv_ct_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
