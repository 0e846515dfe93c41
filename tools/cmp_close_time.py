#!/usr/bin/env python3
"""tools/cmp_close_time.py -> the closing step of a comparison's first round (cofhe_hip_cmp_close_records: k_cmp_close) next to the
existing kernels that give the same bytes: cofhe_hip_lut_select_records copies the entry that every digit of a threshold selects
into a buffer [2, E, n] (the tuple read as E n lookup rows of 2^d entries; one call per threshold), and
cofhe_hip_accumulate_records multiplies the n entries of each of the 2 E rows, starting from the principal form.

    python tools/cmp_close_time.py [--n 256 16384] [--bits 32] [--digit-bits 6] [--runs 3] [--out FILE]

k = 128 (tests/golden/params_s128_k128.json).  The tuple buffer holds E n 2^d ciphertexts drawn from a pool of 4096 fresh
encryptions; the opened values are uniform in Z/2^k.  Per size: both legs once as a warm-up and byte-compared, then `runs`
alternating windows of `reps` calls each, host clock around a drained device.  The digit records of the baseline are computed on
the host beforehand and are not timed.  One JSON line per size: medians, [min, max], and the spread of each leg."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

REC = 168
CT = 2 * REC


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[256, 16384])
    ap.add_argument("--bits", type=int, default=32)
    ap.add_argument("--digit-bits", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import pyref as P
    from bench import exp_records, form_record, hx
    torch.cuda.init()
    from cofhe_amd import Engine
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k, bits, d = prm["k"], a.bits, a.digit_bits
    nd = -(-bits // d)
    delta = hx(prm["delta"])
    E = Engine(delta)
    recs = {name: form_record(hx(prm[name]["a"]), hx(prm[name]["b"]), hx(prm[name]["c"])) for name in ("h", "pk", "f")}
    rng = random.Random(20)
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()      # noqa: E731
    npool = 4096
    pool = torch.zeros(npool * CT, dtype=torch.int32, device="cuda")
    dm, dr = dev(exp_records([rng.getrandbits(k) for _ in range(npool)])), dev(exp_records([rng.randrange(hx(prm["exponent_bound"])) for _ in range(npool)]))
    E.encrypt_fresh_records(dm.data_ptr(), dr.data_ptr(), recs["h"], recs["pk"], recs["f"], pool.data_ptr(), npool, k)
    one = P.identity(delta)
    zero = dev(np.tile(form_record(one.a, one.b, one.c), 2))
    torch.cuda.synchronize()
    lines = []
    for n in a.n:
        m = n * (nd << d)
        gen = torch.Generator(device="cuda").manual_seed(n)
        tuples = pool.view(npool, CT)[torch.randint(0, npool, (m,), device="cuda", generator=gen)].contiguous()
        es = [rng.getrandbits(k) for _ in range(n)]
        de = dev(exp_records(es))
        M = 1 << bits
        th = [(((M >> 1) - e) % M, (-e) % M) for e in es]
        digits = [dev(exp_records([(t[s] >> (j * d)) & ((1 << d) - 1) for t in th for j in range(nd)])) for s in (0, 1)]
        out_a, wrap = torch.zeros(2 * n * CT, dtype=torch.int32, device="cuda"), torch.zeros(n * 32, dtype=torch.int32, device="cuda")
        picked, out_b = torch.zeros(2 * n * nd * CT, dtype=torch.int32, device="cuda"), torch.zeros(2 * n * CT, dtype=torch.int32, device="cuda")

        def fused():
            E.cmp_close_records(de.data_ptr(), tuples.data_ptr(), out_a.data_ptr(), wrap.data_ptr(), n, bits, d, k)

        def composed():
            for s in (0, 1):
                E.lut_select_records(digits[s].data_ptr(), tuples.data_ptr(), picked.data_ptr() + 4 * s * n * nd * CT, n * nd, d)
            E.accumulate_records(picked.data_ptr(), zero.data_ptr(), out_b.data_ptr(), 2 * n, nd, 1)

        fused()
        composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(out_a.view(n, 2, CT), out_b.view(2, n, CT).permute(1, 0, 2)))
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
        row = {"n": n, "bits": bits, "digit_bits": d, "digits": nd, "k": k, "reps": reps, "runs": a.runs, "same_bytes": same}
        for name, v in ms.items():
            row[name + "_ms"] = statistics.median(v)
            row[name + "_ms_min_max"] = [min(v), max(v)]
            row[name + "_spread_ms"] = max(v) - min(v)
        row["status"] = E.device_status(clear=True)
        lines.append(json.dumps(row))
        print("cmp_close_json: " + lines[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    if not all(json.loads(ln)["same_bytes"] and json.loads(ln)["status"] == 0 for ln in lines):
        sys.exit(1)


if __name__ == "__main__":
    main()
