#!/usr/bin/env python3
"""Host verifier against the batched device verifier, in one process on one GPU.

Proves the metric-config segment (synth_fibonacci(419000), 4.19 M steps, default PcsConfig) and two smaller ones once, then times

  host    cm_verify_run   (cm_verify_proof per proof in a loop, then the chain check; the chain check fails on copies of one proof
                          AFTER every proof has been verified, so the time is the n verifications)
  device  cm_verify_many  (one batch)

at n = 1, 8 and 64, for copies of the metric proof and for a mix of the three sizes: 3 untimed calls, then the median of --repeats
(at least 10).  Prints ms per proof for both, the ratio, and the device call's split (host planning, upload, kernels, download of
the result words: cm_verify_many_timing) — as a table and as one JSON line.

    python tools/verify_bench.py [--repeats 10] [--fib-n 419000] [--out profiles/verify_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cairo_m_amd import Backend  # noqa: E402
from cairo_m_amd.lib import synth_fibonacci, verify_many, verify_many_timing, verify_run  # noqa: E402


def median_ms(fn, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--fib-n", type=int, default=419_000)
    ap.add_argument("--mix", type=int, nargs=2, default=[7, 40_000], help="the two other sizes of the mixed batch")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1, 8, 64])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    repeats = max(args.repeats, 10)
    B = Backend(0)
    proofs = {}
    for n in [args.fib_n] + list(args.mix):
        inp = synth_fibonacci(n)
        proofs[n] = B.prove(inp)
        inp.free()
        assert proofs[n].verify() == (0, ""), n
    rows = []
    for kind in ("copies", "mix"):
        for n in args.sizes:
            pool = [proofs[args.fib_n]] if kind == "copies" else [proofs[k] for k in [args.fib_n] + list(args.mix)]
            batch = [pool[i % len(pool)] for i in range(n)]
            assert verify_many(batch, lib=B.L) == [(0, "")] * n

            def host():
                rc, msg = verify_run(batch, lib=B.L)
                assert rc == 0 or "verification failed" not in msg, msg     # (copies do not chain: every proof was verified first)

            split = {"plan": [], "upload": [], "kernels": [], "download": []}

            def device():
                verify_many(batch, lib=B.L)
                for k, v in verify_many_timing(B.L).items():
                    split[k].append(v)

            h = median_ms(host, repeats)
            d = median_ms(device, repeats)
            row = {"batch": kind, "n": n, "host_ms_per_proof": h / n, "device_ms_per_proof": d / n, "host_over_device": h / d,
                   "device_split_ms": {k: statistics.median(v[-repeats:]) for k, v in split.items()}}
            rows.append(row)
            s = row["device_split_ms"]
            print("%-6s n=%-3d host %8.3f ms/proof   device %8.3f ms/proof   host/device %6.2f   device call: plan %.2f upload %.2f "
                  "kernels %.2f download %.2f ms" % (kind, n, row["host_ms_per_proof"], row["device_ms_per_proof"], row["host_over_device"],
                                                    s["plan"], s["upload"], s["kernels"], s["download"]), flush=True)
    result = {"tool": "verify_bench", "fib_n": args.fib_n, "mix": args.mix, "repeats": repeats, "warmup": 3,
              "proof_words": {str(k): int(p.words().size) for k, p in proofs.items()}, "rows": rows}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for p in proofs.values():
        p.free()


if __name__ == "__main__":
    main()
