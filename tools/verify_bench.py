#!/usr/bin/env python3
"""Host verifier against the batched device verifier, in one process on one GPU.

Proves the metric-config segment (synth_fibonacci(419000), 4.19 M steps, default PcsConfig) and two smaller ones once, then times

  host    cm_verify_run   (cm_verify_proof per proof in a loop, then the chain check; the chain check fails on copies of one proof
                          AFTER every proof has been verified, so the time is the n verifications)
  device  cm_verify_many  (one batch)

  arith   cm_verify_many_ex with CM_VERIFY_ARITH_ON_DEVICE  (one batch; the public LogUp sum and the OODS check on the GPU too)

at n = 1, 8 and 64, for copies of the metric proof and for a mix of the three sizes, and at n = 1 and 8 for a proof whose public
program has 2^12 cells (all_opcodes_program(1) padded with data cells behind its last instruction — the VM takes padded images):
3 untimed calls, then the median of --repeats (at least 10).  Prints ms per proof for each, the ratio, and each device call's
split (host planning, upload, kernels, download of the result words: cm_verify_many_timing) — as a table and as one JSON line.
Per proof kind it also times the host's initial_logup_sum alone (cm_public_logup_sum_host on the proof's public data): the part
of the planning time that the public program scales.

    python tools/verify_bench.py [--repeats 10] [--fib-n 419000] [--arith both] [--out profiles/verify_bench.json]

--arith host leaves the new mode out (a library built before it has no cm_verify_many_ex).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cairo_m_amd import Backend  # noqa: E402
from cairo_m_amd.lib import (public_logup_sum_host, public_sum_job, synth_fibonacci, verify_many, verify_many_timing,  # noqa: E402
                             verify_run, vm_run)

LARGE = "program_4096"


def large_program_input(n_cells=1 << 12):
    """all_opcodes_program(1) with data cells behind it up to n_cells cells (cairo_m_amd/workloads.py): every cell is public"""
    from cairo_m_amd.workloads import all_opcodes_program, padded_program
    return vm_run(padded_program(all_opcodes_program(1)[0], n_cells), entry_pc=0, args=(), n_returns=0)


def logup_host_ms(proof, L, repeats):
    """median ms of the host's initial_logup_sum on this proof's public data (any relation words: the cost does not depend on them)"""
    import numpy as np
    w = [int(x) for x in proof.words()]
    i = 6 + 5 * w[5]
    head, i = w[i:i + 7], i + 7
    lists = []
    for _ in range(3):
        lists.append(np.array(w[i + 1:i + 1 + 7 * w[i]], dtype=np.uint32))
        i += 1 + 7 * w[i]
    rel = np.random.default_rng(1).integers(1, 2**31 - 1, size=544, dtype=np.uint32)
    job = public_sum_job(head, lists[0], lists[1], lists[2], rel)
    present = int(sum(x.reshape(-1, 7)[:, 0].sum() for x in lists if x.size))
    return median_ms(lambda: public_logup_sum_host(job, L), repeats), present


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
    ap.add_argument("--arith", choices=["host", "both"], default="both", help="host: time the default mode only")
    ap.add_argument("--no-large", action="store_true", help="leave the 2^12-cell program batch out")
    ap.add_argument("--plan-split", action="store_true",
                    help="only print, per proof kind, how the host planning time of one proof splits (the library's own marks, 12 calls each)")
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
    if not args.no_large:
        inp = large_program_input()
        proofs[LARGE] = B.prove(inp)
        inp.free()
        assert proofs[LARGE].verify() == (0, ""), LARGE
    if args.plan_split:
        from cairo_m_amd.lib import verify_plan_stats
        os.environ["CM_VERIFY_PLAN_MARKS"] = "1"          # the library prints one line per planned proof on stderr
        for k in [args.fib_n] + ([] if args.no_large else [LARGE]):
            print("plan split of one %s proof, 12 calls:" % k, file=sys.stderr, flush=True)
            for _ in range(12):
                verify_plan_stats([proofs[k]], lib=B.L)
        return
    logup = {}
    for k in ([args.fib_n] + ([] if args.no_large else [LARGE])) if hasattr(B.L, "cm_public_logup_sum_host") else []:
        ms, present = logup_host_ms(proofs[k], B.L, repeats)
        logup[str(k)] = {"present_public_entries": present, "host_initial_logup_sum_ms": ms}
        print("%-12s %5d present public entries: host initial_logup_sum %.3f ms" % (k, present, ms), flush=True)
    rows = []
    for kind in ("copies", "mix") + (() if args.no_large else ("large",)):
        for n in ([s for s in args.sizes if s <= 8] if kind == "large" else args.sizes):
            pool = [proofs[LARGE]] if kind == "large" else [proofs[args.fib_n]] if kind == "copies" else [proofs[k] for k in [args.fib_n] + list(args.mix)]
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

            asplit = {"plan": [], "upload": [], "kernels": [], "download": []}

            def arith():
                verify_many(batch, lib=B.L, arith="device")
                for k, v in verify_many_timing(B.L).items():
                    asplit[k].append(v)

            h = median_ms(host, repeats)
            d = median_ms(device, repeats)
            row = {"batch": kind, "n": n, "host_ms_per_proof": h / n, "device_ms_per_proof": d / n, "host_over_device": h / d,
                   "device_split_ms": {k: statistics.median(v[-repeats:]) for k, v in split.items()}}
            if args.arith == "both":
                assert verify_many(batch, lib=B.L, arith="device") == [(0, "")] * n
                a = median_ms(arith, repeats)
                row.update({"arith_ms_per_proof": a / n, "device_over_arith": d / a,
                            "arith_split_ms": {k: statistics.median(v[-repeats:]) for k, v in asplit.items()}})
            rows.append(row)
            s = row["device_split_ms"]
            print("%-6s n=%-3d host %8.3f ms/proof   device %8.3f ms/proof   host/device %6.2f   device call: plan %.2f upload %.2f "
                  "kernels %.2f download %.2f ms" % (kind, n, row["host_ms_per_proof"], row["device_ms_per_proof"], row["host_over_device"],
                                                    s["plan"], s["upload"], s["kernels"], s["download"]), flush=True)
            if args.arith == "both":
                s = row["arith_split_ms"]
                print("%-6s n=%-3d arith on device %8.3f ms/proof   device/arith %6.2f   call: plan %.2f upload %.2f kernels %.2f "
                      "download %.2f ms" % (kind, n, row["arith_ms_per_proof"], row["device_over_arith"], s["plan"], s["upload"], s["kernels"],
                                            s["download"]), flush=True)
    result = {"tool": "verify_bench", "fib_n": args.fib_n, "mix": args.mix, "repeats": repeats, "warmup": 3, "arith": args.arith,
              "host_logup": logup,
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
