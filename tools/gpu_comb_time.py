"""Fresh randomness per ciphertext: time the comb entry points (cofhe_hip_encrypt_fresh_records, cofhe_hip_rerandomize_records,
cofhe_hip_pow_fixed_base_many_records) with HIP events on the launch stream, median of RUNS runs after a warm-up, against the
per-element k_pow ladder (cofhe_hip_pow_form_records over the 2n forms h, pk) and today's shared-r
cofhe_hip_encrypt_records, alternating in one process; first use of a table timed on its own; a width sweep.

    python tools/gpu_comb_time.py [OUT.json] [--sizes 1,64,1024,16384,262144] [--widths 6,8,10] [--ladder-max 16384]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench import exp_records, form_record, hx  # noqa: E402
from cofhe_amd import Engine  # noqa: E402

RUNS = 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None)
    ap.add_argument("--sizes", default="1,64,1024,16384,262144")
    ap.add_argument("--widths", default="6,8,10")
    ap.add_argument("--ladder-max", type=int, default=16384)
    a = ap.parse_args()
    torch.cuda.init()
    prm = json.load(open(os.path.join(ROOT, "tests", "golden", "params_s128_k128.json")))
    k, bound = prm["k"], hx(prm["exponent_bound"])
    rec = {n: form_record(hx(prm[n]["a"]), hx(prm[n]["b"]), hx(prm[n]["c"])) for n in ("h", "pk", "f")}
    sizes = [int(x) for x in a.sizes.split(",")]
    widths = [int(x) for x in a.widths.split(",")]
    rng = np.random.default_rng(7)
    res = {"params": prm["name"], "k": k, "exponent_bits": bound.bit_length() - 1, "runs": RUNS, "statistic": "median ms, HIP events",
           "first_use": {}, "sizes": {}, "width_sweep": {}}

    def dev(arr):
        return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()

    def rand_exps(n, bits):
        words = rng.integers(0, 1 << 32, size=(n, 32), dtype=np.uint64).astype(np.uint32)
        top = bits // 32
        words[:, top] &= (1 << (bits % 32)) - 1
        words[:, top + 1:] = 0
        return words.reshape(-1)

    # first use of a (base, w): a context of its own, so that nothing is cached
    for w in widths:
        E = Engine(hx(prm["delta"]))
        E.set_option("comb_width", w)
        dm, dr = dev(rand_exps(1, k)), dev(rand_exps(1, 965))
        out = torch.zeros(2 * 168, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.encrypt_fresh_records(dm.data_ptr(), dr.data_ptr(), rec["h"], rec["pk"], rec["f"], out.data_ptr(), 1, k)
        E.stream_sync()
        first = (time.perf_counter() - t0) * 1e3
        E.set_option("profile_kernels", 1)
        E.profile_read("k_comb_table", clear=True)
        E2 = Engine(hx(prm["delta"]))      # table levels alone, without the chains: a second context, its chains built first
        E2.set_option("comb_width", w)
        E2.set_option("profile_kernels", 1)
        f = rec["f"]
        E2.pow_fixed_base_record(f, exp_records([3]), out.data_ptr())      # builds f's chain only
        E2.stream_sync()
        E2.profile_read("k_comb_table", clear=True)
        E2.pow_fixed_base_many_records(f, dr.data_ptr(), out.data_ptr(), 1)
        E2.stream_sync()
        tab_ms, tab_launches = E2.profile_read("k_comb_table", clear=True)
        res["first_use"][str(w)] = {"encrypt_fresh_first_call_ms_wall": round(first, 2), "table_levels_ms_one_base": round(tab_ms, 3),
                                    "table_level_launches": tab_launches,
                                    "table_mb": round((992 // w + 1) * (1 << (w - 1)) * 672 / 1e6, 2)}
        print("first use w=%d: %s" % (w, res["first_use"][str(w)]), flush=True)
        E2.close()
        E.close()

    E = Engine(hx(prm["delta"]))

    def timed(fn):
        fn()
        ts = [E.time_stream(fn) for _ in range(RUNS)]
        return statistics.median(ts)

    for n in sizes:
        ms = dev(rand_exps(n, k))
        rs = dev(rand_exps(n, 965))
        out = torch.zeros(n * 2 * 168, dtype=torch.int32, device="cuda")
        one = {}
        E.set_option("comb_width", 0)
        one["encrypt_fresh_ms"] = timed(lambda: E.encrypt_fresh_records(ms.data_ptr(), rs.data_ptr(), rec["h"], rec["pk"], rec["f"], out.data_ptr(), n, k))
        one["rerandomize_ms"] = timed(lambda: E.rerandomize_records(out.data_ptr(), rs.data_ptr(), rec["h"], rec["pk"], out.data_ptr(), n))
        o1 = torch.zeros(n * 168, dtype=torch.int32, device="cuda")

        def comb_powers():
            E.pow_fixed_base_many_records(rec["h"], rs.data_ptr(), o1.data_ptr(), n)
            E.pow_fixed_base_many_records(rec["pk"], rs.data_ptr(), o1.data_ptr(), n)
        one["comb_powers_h_pk_ms"] = timed(comb_powers)
        if n <= a.ladder_max:
            # alternating: ladder route (2n forms), shared-r encryption, comb powers again
            bases = dev(np.tile(np.concatenate([rec["h"], rec["pk"]]), n))
            r2 = dev(np.repeat(np.ascontiguousarray(rs.cpu().numpy().view(np.uint32)).reshape(n, 32), 2, axis=0).reshape(-1))
            lo = torch.zeros(n * 2 * 168, dtype=torch.int32, device="cuda")
            hp = torch.zeros(2 * 168, dtype=torch.int32, device="cuda")
            E.pow_form_records(bases[: 2 * 168].data_ptr(), r2[: 64].data_ptr(), hp.data_ptr(), 2)
            lad, shr, cmb = [], [], []
            E.pow_form_records(bases.data_ptr(), r2.data_ptr(), lo.data_ptr(), 2 * n)
            for _ in range(RUNS):
                lad.append(E.time_stream(lambda: E.pow_form_records(bases.data_ptr(), r2.data_ptr(), lo.data_ptr(), 2 * n)))
                shr.append(E.time_stream(lambda: E.encrypt_records(ms.data_ptr(), hp.data_ptr(), rec["f"], out.data_ptr(), n, k)))
                cmb.append(E.time_stream(comb_powers))
            one["ladder_powers_h_pk_ms"] = statistics.median(lad)
            one["shared_r_encrypt_ms"] = statistics.median(shr)
            one["comb_powers_h_pk_ms_alternating"] = statistics.median(cmb)
            one["comb_speedup_over_ladder"] = round(one["ladder_powers_h_pk_ms"] / one["comb_powers_h_pk_ms_alternating"], 2)
            del bases, r2, lo
        one = {kk: (round(v, 3) if isinstance(v, float) else v) for kk, v in one.items()}
        res["sizes"][str(n)] = one
        print("n=%d: %s  status %d" % (n, one, E.device_status(clear=True)), flush=True)
        del ms, rs, out, o1
        torch.cuda.empty_cache()

    for n in [x for x in sizes if x >= 1024]:
        ms = dev(rand_exps(n, k))
        rs = dev(rand_exps(n, 965))
        out = torch.zeros(n * 2 * 168, dtype=torch.int32, device="cuda")
        sw = {}
        for w in widths:
            E.set_option("comb_width", w)
            sw[str(w)] = {"encrypt_fresh_ms": round(timed(lambda: E.encrypt_fresh_records(ms.data_ptr(), rs.data_ptr(), rec["h"], rec["pk"], rec["f"],
                                                                                           out.data_ptr(), n, k)), 3),
                          "rerandomize_ms": round(timed(lambda: E.rerandomize_records(out.data_ptr(), rs.data_ptr(), rec["h"], rec["pk"],
                                                                                       out.data_ptr(), n)), 3)}
        E.set_option("comb_width", 0)
        res["width_sweep"][str(n)] = sw
        print("width sweep n=%d: %s  status %d" % (n, sw, E.device_status(clear=True)), flush=True)
        del ms, rs, out
        torch.cuda.empty_cache()
    res["device_status"] = E.device_status(clear=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
