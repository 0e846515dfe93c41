"""Differences and plaintext addends: time cofhe_hip_sub_ciphertext_records against cofhe_hip_add_ciphertext_records (the same
body plus a sign flip) and against the route it replaces (cofhe_hip_pow_records by 2^k - 1, then an addition), and
cofhe_hip_add_plain_records with and without randomness against an encryption followed by an addition
(cofhe_hip_encrypt_records / cofhe_hip_encrypt_fresh_records + cofhe_hip_add_ciphertext_records).  HIP events on the launch
stream, a warm-up, the median of RUNS runs with the sides of a comparison alternated in one process; min and max are kept so
that a difference can be set against the spread.

    python tools/gpu_affine_time.py [OUT.json] [--sizes 1024,16384]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import SplitMix64, exp_records, form_record, hx  # noqa: E402
from cofhe_amd import Engine  # noqa: E402
from gpu_inputs import encrypt_tensor_gpu  # noqa: E402

RUNS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--sizes", default="1024,16384")
    a = ap.parse_args()
    torch.cuda.init()
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k = prm["k"]
    rec = {n: form_record(hx(prm[n]["a"]), hx(prm[n]["b"]), hx(prm[n]["c"])) for n in ("h", "pk", "f")}
    E = Engine(hx(prm["delta"]))
    rng = SplitMix64(11)
    dev = torch.device("cuda", 0)
    res = {"params": prm["name"], "k": k, "runs": RUNS, "statistic": "median [min, max] ms, HIP events, sides alternated", "sizes": {}}

    def dev_i32(arr):
        return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32)).to(dev)

    def alternate(sides):
        """sides: name -> callable; one warm-up each, then RUNS rounds over all sides in turn"""
        for fn in sides.values():
            fn()
        ts = {name: [] for name in sides}
        for _ in range(RUNS):
            for name, fn in sides.items():
                ts[name].append(E.time_stream(fn))
        return {name: [round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4)] for name, v in ts.items()}

    for n in [int(x) for x in a.sizes.split(",")]:
        x = encrypt_tensor_gpu(E, torch, prm, [rng.bits(k) for _ in range(n)], rng.bits(960), dev)      # one r each: shared c1
        y = encrypt_tensor_gpu(E, torch, prm, [rng.bits(k) for _ in range(n)], rng.bits(960), dev)
        idx = torch.randperm(n, device="cuda")
        xd = x.view(n, 336).clone()
        xd[:, :168] = y.view(n, 336)[idx, 168:]                  # distinct c1: no folding
        xd = xd.reshape(-1).contiguous()
        out, tmp = torch.empty_like(x), torch.empty_like(x)
        minus_one = dev_i32(exp_records([(1 << k) - 1] * n))
        ms = dev_i32(exp_records([rng.bits(k) for _ in range(n)]))
        rs = dev_i32(exp_records([rng.bits(960) for _ in range(n)]))
        hp = dev_i32(np.concatenate([rec["h"], rec["pk"]]))       # stand-ins for h^r, pk^r of the shared-r encryption
        P = lambda t: t.data_ptr()      # noqa: E731

        def negate_add():
            E.pow_records(P(y), P(minus_one), P(tmp), n)
            E.add_ciphertext_records(P(x), P(tmp), P(out), n)

        def encrypt_add():
            E.encrypt_records(P(ms), P(hp), rec["f"], P(tmp), n, k)
            E.add_ciphertext_records(P(x), P(tmp), P(out), n)

        def encrypt_fresh_add():
            E.encrypt_fresh_records(P(ms), P(rs), rec["h"], rec["pk"], rec["f"], P(tmp), n, k)
            E.add_ciphertext_records(P(x), P(tmp), P(out), n)

        one = {}
        one["shared_c1"] = alternate({"add": lambda: E.add_ciphertext_records(P(x), P(y), P(out), n),
                                      "sub": lambda: E.sub_ciphertext_records(P(x), P(y), P(out), n)})
        one["distinct_c1"] = alternate({"add": lambda: E.add_ciphertext_records(P(xd), P(y), P(out), n),
                                        "sub": lambda: E.sub_ciphertext_records(P(xd), P(y), P(out), n)})
        one["difference"] = alternate({"sub": lambda: E.sub_ciphertext_records(P(x), P(y), P(out), n), "negate_then_add": negate_add,
                                       "negate_alone": lambda: E.pow_records(P(y), P(minus_one), P(tmp), n),
                                       "invert_records": lambda: E.invert_records(P(y), P(tmp), 2 * n)})
        one["plaintext_addend"] = alternate({
            "add_plain": lambda: E.add_plain_records(P(x), P(ms), rec["f"], P(out), n, k, 0),
            "encrypt_then_add": encrypt_add,
            "add_plain_fresh_r": lambda: E.add_plain_records(P(x), P(ms), rec["f"], P(out), n, k, 0, d_r=P(rs), h_record=rec["h"],
                                                             pk_record=rec["pk"]),
            "encrypt_fresh_then_add": encrypt_fresh_add})
        res["sizes"][str(n)] = one
        print("n=%d: %s  status %d" % (n, json.dumps(one), E.device_status(clear=True)), flush=True)
        del x, y, xd, out, tmp
        torch.cuda.empty_cache()
    res["device_status"] = E.device_status(clear=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
