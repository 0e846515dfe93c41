#!/usr/bin/env python3
"""tools/divide_exact_time.py -> the kernels of the exact division by small divisors next to the lookup kernels that move the same
bytes, and one exact truncation split into its phases next to the inexact one.

    python tools/divide_exact_time.py [--n 16384] [--rows 256] [--trunc-n 256] [--runs 3] [--out FILE]

k = 128 (tests/golden/params_s128_k128.json).  Three JSON lines:

  select: cofhe_hip_divx_close_records (D = rows = 2^b) and cofhe_hip_lut_select_records (bits = b) on the same tuple buffer of
    n rows ciphertexts, drawn from a pool of 4096 fresh encryptions, and the same opened values; the kernels' own spans
    ("profile_kernels": k_divx_select, k_plain_divmod, k_lut_select) over `runs` alternating calls.  For D = 2^b the remainder is
    the lookup index, so the lookup's output plus the plaintext addend of the quotients must be the closing step's bytes.
  rows: cofhe_hip_divx_rows_records (k_divx_prep + k_divx_rows) and cofhe_hip_lut_rotate_records (k_lut_rotate, one table) at the
    same n and rows: the same number of output records.
  truncate: an exact truncation by 2^8 over trunc-n elements in three phases -- tuple generation (divx_tuples_records and the
    fresh encryption of the masks), opening (the difference, its decryption, the read-back) and closing (divx_close_records) --
    next to the same phases of the inexact division pair (divfloor_plain_records and two fresh encryptions; div_close_records);
    host clock around a drained device, medians of `runs`."""
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
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--rows", type=int, default=256)
    ap.add_argument("--trunc-n", type=int, default=256)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    from bench import exp_records, form_record, hx
    torch.cuda.init()
    from cofhe_amd import Engine
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k, n, rows = prm["k"], a.n, a.rows
    bits = rows.bit_length() - 1
    assert rows == 1 << bits and 1 <= bits <= 12, "rows is a power of two: the lookup kernels are the yardstick"
    delta, bound = hx(prm["delta"]), hx(prm["exponent_bound"])
    E = Engine(delta)
    recs = {name: form_record(hx(prm[name]["a"]), hx(prm[name]["b"]), hx(prm[name]["c"])) for name in ("h", "pk", "f")}
    sk = hx(prm["sk"])
    rng = random.Random(22)
    dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()      # noqa: E731
    zeros = lambda words: torch.zeros(words, dtype=torch.int32, device="cuda")      # noqa: E731
    med = lambda v: {"ms": statistics.median(v), "ms_min_max": [min(v), max(v)]}      # noqa: E731
    lines = []

    def spans(names):
        got = {nm: E.profile_read(nm) for nm in names}
        E.profile_read(names[0], clear=True)                    # clearing drops every span, whatever its name
        return got

    # ---- select ----
    npool = 4096
    pool = zeros(npool * CT)
    dm, dr = dev(exp_records([rng.getrandbits(k) for _ in range(npool)])), dev(exp_records([rng.randrange(bound) for _ in range(npool)]))
    E.encrypt_fresh_records(dm.data_ptr(), dr.data_ptr(), recs["h"], recs["pk"], recs["f"], pool.data_ptr(), npool, k)
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(n)
    tuples = pool.view(npool, CT)[torch.randint(0, npool, (n * rows,), device="cuda", generator=gen)].contiguous()
    de = dev(exp_records([rng.getrandbits(k) for _ in range(n)]))
    dd = dev(exp_records([rows]))
    out_x, out_l, q, rem = zeros(n * CT), zeros(n * CT), zeros(n * 32), zeros(n)
    names = ("k_divx_select", "k_plain_divmod", "k_lut_select")
    E.set_option("profile_kernels", 1)
    ms = {nm: [] for nm in names}
    for run in range(a.runs + 1):                      # the first pass warms up and is dropped
        E.divx_close_records(de.data_ptr(), dd.data_ptr(), 1, tuples.data_ptr(), rows, recs["f"], out_x.data_ptr(), n, k)
        E.lut_select_records(de.data_ptr(), tuples.data_ptr(), out_l.data_ptr(), n, bits)
        torch.cuda.synchronize()
        for nm, (total, launches) in spans(names).items():
            assert launches == 1, nm
            if run:
                ms[nm].append(total)
    E.divmod_plain_records(de.data_ptr(), dd.data_ptr(), 1, q.data_ptr(), rem.data_ptr(), n, rows, k)
    E.add_plain_records(out_l.data_ptr(), q.data_ptr(), recs["f"], out_l.data_ptr(), n, k, mode=0)
    torch.cuda.synchronize()
    spans(("k_plain_divmod",))
    row = {"what": "select", "n": n, "rows": rows, "k": k, "runs": a.runs, "bytes_moved": 2 * n * CT * 4,
           "same_bytes": bool(torch.equal(out_x, out_l))}
    for nm in names:
        row[nm] = med(ms[nm])
    lines.append(row)
    print("divide_exact_json: " + json.dumps(row), flush=True)
    del tuples, pool

    # ---- rows ----
    dr_n = dev(exp_records([rng.getrandbits(k) for _ in range(n)]))
    table = dev(exp_records([rng.getrandbits(k) for _ in range(rows)]))
    out_r, out_t = zeros(n * rows * 32), zeros(n * rows * 32)
    names = ("k_divx_prep", "k_divx_rows", "k_lut_rotate")
    ms = {nm: [] for nm in names}
    for run in range(a.runs + 1):
        E.divx_rows_records(dr_n.data_ptr(), dd.data_ptr(), 1, out_r.data_ptr(), n, rows, k)
        E.lut_rotate_records(table.data_ptr(), 1, dr_n.data_ptr(), out_t.data_ptr(), n, bits)
        torch.cuda.synchronize()
        for nm, (total, launches) in spans(names).items():
            assert launches == 1, nm
            if run:
                ms[nm].append(total)
    E.set_option("profile_kernels", 0)
    row = {"what": "rows", "n": n, "rows": rows, "k": k, "runs": a.runs, "bytes_stored": n * rows * 128}
    for nm in names:
        row[nm] = med(ms[nm])
    lines.append(row)
    print("divide_exact_json: " + json.dumps(row), flush=True)
    del out_r, out_t

    # ---- truncate by 2^8, phase by phase ----
    tn, D = a.trunc_n, 256
    M = 1 << k
    xs = [rng.choice((1, -1)) * rng.getrandbits(40) % M for _ in range(tn)]
    rs = [rng.getrandbits(k) for _ in range(tn)]
    dxs, drs, dD = dev(exp_records(xs)), dev(exp_records(rs)), dev(exp_records([D]))
    rho = lambda m: dev(exp_records([rng.randrange(bound) for _ in range(m)]))      # noqa: E731
    rho_x, rho_r, rho_q, rho_t = rho(tn), rho(tn), rho(tn), rho(tn * D)
    dsk = dev(exp_records([sk]))
    ow = (k + 31) // 32 + 1
    cx, cr, crq, diff, out = zeros(tn * CT), zeros(tn * CT), zeros(tn * CT), zeros(tn * CT), zeros(tn * CT)
    tup, rq, opened, e_recs = zeros(tn * D * CT), zeros(tn * 32), zeros(tn * ow), zeros(tn * 32)
    fresh = lambda m, r, o, cnt: E.encrypt_fresh_records(m.data_ptr(), r.data_ptr(), recs["h"], recs["pk"], recs["f"], o.data_ptr(), cnt, k)      # noqa: E731
    fresh(dxs, rho_x, cx, tn)

    def opening():
        E.sub_ciphertext_records(cx.data_ptr(), cr.data_ptr(), diff.data_ptr(), tn)
        E.decrypt_records(diff.data_ptr(), dsk.data_ptr(), recs["f"], opened.data_ptr(), tn, k)
        w = opened.cpu().numpy().view(np.uint32).reshape(tn, ow)                     # the read-back of the opened values
        es = [int.from_bytes(r_[:-1].tobytes(), "little") for r_ in w]
        e_recs.copy_(dev(exp_records(es)))
        return es

    def exact_gen():
        fresh(drs, rho_r, cr, tn)
        E.divx_tuples_records(drs.data_ptr(), dD.data_ptr(), 1, rho_t.data_ptr(), recs["h"], recs["pk"], recs["f"], tup.data_ptr(), tn, D, k)

    def exact_close():
        E.divx_close_records(e_recs.data_ptr(), dD.data_ptr(), 1, tup.data_ptr(), D, recs["f"], out.data_ptr(), tn, k)

    def pair_gen():
        fresh(drs, rho_r, cr, tn)
        E.divfloor_plain_records(drs.data_ptr(), dD.data_ptr(), 1, rq.data_ptr(), tn, k)
        fresh(rq, rho_q, crq, tn)

    def pair_close():
        E.div_close_records(e_recs.data_ptr(), dD.data_ptr(), 1, crq.data_ptr(), recs["f"], out.data_ptr(), tn, k)

    def decrypted():
        E.decrypt_records(out.data_ptr(), dsk.data_ptr(), recs["f"], opened.data_ptr(), tn, k)
        w = opened.cpu().numpy().view(np.uint32).reshape(tn, ow)
        return [int.from_bytes(r_[:-1].tobytes(), "little") for r_ in w]

    centred = lambda v: v - M if v >> (k - 1) else v      # noqa: E731
    want = [(centred(x) // D) % M for x in xs]
    ms = {nm: [] for nm in ("exact_tuples", "exact_opening", "exact_closing", "pair_pairs", "pair_opening", "pair_closing")}
    off = {"exact": 0, "pair": 0}
    for run in range(a.runs + 1):
        for leg, phases in (("exact", (("tuples", exact_gen), ("opening", opening), ("closing", exact_close))),
                            ("pair", (("pairs", pair_gen), ("opening", opening), ("closing", pair_close)))):
            for nm, fn in phases:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if run:
                    ms[leg + "_" + nm].append((time.perf_counter() - t0) * 1e3)
            errs = [(w_ - y) % M for w_, y in zip(want, decrypted())]
            assert set(errs) <= ({0} if leg == "exact" else {0, 1}), leg
            off[leg] = sum(errs)
    row = {"what": "truncate", "n": tn, "shift": 8, "k": k, "runs": a.runs, "fresh_encryptions_exact": tn * (D + 1), "fresh_encryptions_pair": 2 * tn,
           "one_less_exact": off["exact"], "one_less_pair": off["pair"]}
    for nm, v in ms.items():
        row[nm] = med(v)
    row["status"] = E.device_status(clear=True)
    lines.append(row)
    print("divide_exact_json: " + json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(json.dumps(ln) for ln in lines) + "\n")
    if not lines[0]["same_bytes"] or lines[-1]["status"] != 0:
        sys.exit(1)


if __name__ == "__main__":
    main()
