#!/usr/bin/env python3
"""tools/spline_close_time.py -> the closing step of a spline (cofhe_hip_spline_close_records: k_spline_powers + k_spline_close)
next to the composition that gives the same bytes without the fused kernel: the powers, a device-to-device gather of the d + 1
selected ciphertexts, cofhe_hip_pow_dot_records and one cofhe_hip_add_ciphertext_records.

    python tools/spline_close_time.py [--n 256 16384] [--bits 5] [--shift 11] [--degree 2] [--runs 3] [--out FILE]

k = 128 (tests/golden/params_s128_k128.json).  The tuple buffer holds n 2^bits (d + 1) ciphertexts drawn from a pool of 4096 fresh
encryptions; the opened values are uniform in Z/2^k.  Per size: both legs once as a warm-up and byte-compared, then `runs`
alternating windows of `reps` calls each, host clock around a drained device.  The gather's index is computed on the host
beforehand and is not timed.  One JSON line per size: medians, [min, max], and the spread of each leg."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REC = 168
CT = 2 * REC


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--bits", type=int, default=5)
    ap.add_argument("--shift", type=int, default=11)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import exp_records, form_record, hx
    torch.cuda.init()
    from cofhe_amd import Engine
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k, b, t, d = prm["k"], a.bits, a.shift, a.degree
    E = Engine(hx(prm["delta"]))
    recs = {name: form_record(hx(prm[name]["a"]), hx(prm[name]["b"]), hx(prm[name]["c"])) for name in ("h", "pk", "f")}
    rng = random.Random(19)
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()      # noqa: E731
    npool = 4096
    pool = torch.zeros(npool * CT, dtype=torch.int32, device="cuda")
    bound = hx(prm["exponent_bound"])
    E.encrypt_fresh_records(dev(exp_records([rng.getrandbits(k) for _ in range(npool)])).data_ptr(),
                            dev(exp_records([rng.randrange(bound) for _ in range(npool)])).data_ptr(), recs["h"], recs["pk"], recs["f"],
                            pool.data_ptr(), npool, k)
    torch.cuda.synchronize()
    lines = []
    for n in a.n:
        m = (n << b) * (d + 1)
        gen = torch.Generator(device="cuda").manual_seed(n)
        tuples = pool.view(npool, CT)[torch.randint(0, npool, (m,), device="cuda", generator=gen)].contiguous()
        es = [rng.getrandbits(k) for _ in range(n)]
        de = dev(exp_records(es))
        sel = [(i << b) + ((e >> t) & ((1 << b) - 1)) for i, e in enumerate(es)]
        # power-major indices of the bases q_1 .. q_d, then those of the constant terms
        idx = torch.tensor([s * (d + 1) + c for c in range(1, d + 1) for s in sel] + [s * (d + 1) for s in sel], device="cuda")
        powers = torch.zeros(n * d * 32, dtype=torch.int32, device="cuda")
        prod, out_a, out_b = (torch.zeros(n * CT, dtype=torch.int32, device="cuda") for _ in range(3))

        def fused():
            E.spline_close_records(de.data_ptr(), tuples.data_ptr(), out_a.data_ptr(), n, b, t, d, k)

        def composed():
            E.spline_powers_records(de.data_ptr(), powers.data_ptr(), n, d, k)
            g = tuples.view(m, CT)[idx]                                  # the d + 1 selected ciphertexts, gathered device to device
            torch.cuda.synchronize()                                     # torch's stream and the library's are not the same stream
            E.pow_dot_records(g.data_ptr(), powers.data_ptr(), prod.data_ptr(), n, d)
            E.add_ciphertext_records(prod.data_ptr(), g.data_ptr() + 4 * d * n * CT, out_b.data_ptr(), n)

        fused()
        composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a, out_b))
        reps = max(1, 4096 // n)
        ms = {"fused": [], "composed": []}
        for _ in range(a.runs):
            for name, fn in (("fused", fused), ("composed", composed)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / reps)
        row = {"n": n, "bits": b, "shift": t, "degree": d, "k": k, "reps": reps, "runs": a.runs, "same_bytes": same}
        for name, v in ms.items():
            row[name + "_ms"] = statistics.median(v)
            row[name + "_ms_min_max"] = [min(v), max(v)]
            row[name + "_spread_ms"] = max(v) - min(v)
        row["status"] = E.device_status(clear=True)
        lines.append(json.dumps(row))
        print("spline_close_json: " + lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not all(json.loads(ln)["same_bytes"] and json.loads(ln)["status"] == 0 for ln in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
