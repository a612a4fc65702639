#!/usr/bin/env python3
"""Peak device memory per proof: the twin of the reference's memory benchmark (fibonacci_prove_peak_mem, sha256_1kb_prove_peak_mem)
plus a 2^24-row segment.  For each workload: three identical lone proofs from a trimmed pool; the third one's cm_proof_memory
(per-phase peaks, driver_allocs), cm_estimate_memory and estimate / peak.  Writes profiles/<set>_mem.json.
    python tools/mem_report.py --set r07 [--skip-big]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", required=True, help="name of the measurement set: profiles/<set>_mem.json")
    ap.add_argument("--fib-n", type=int, default=419_000, help="fibonacci_loop size of the metric config")
    ap.add_argument("--big-fib-n", type=int, default=1_677_000, help="fibonacci_loop whose largest LDE column has 2^24 rows")
    ap.add_argument("--skip-big", action="store_true")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import Proof, estimate_memory, mem_reset_peak, mem_stats, synth_fibonacci, vm_run
    from cairo_m_amd.workloads import sha256_program
    be = Backend(0)
    L = be.L

    def sha_input():
        prog = sha256_program(bytes(range(256)) * 4)          # a 1024-byte message
        return vm_run(prog[0] if isinstance(prog, tuple) else prog, entry_pc=0, args=(), n_returns=0, lib=L)

    loads = [("fibonacci_prove_peak_mem", f"fibonacci_loop n={a.fib_n} (metric config)", lambda: synth_fibonacci(a.fib_n, lib=L)),
             ("sha256_1kb_prove_peak_mem", "SHA-256 of a 1024-byte message", sha_input)]
    if not a.skip_big:
        loads.append(("fibonacci_2pow24_prove_peak_mem", f"fibonacci_loop n={a.big_fib_n} (2^24-row LDE columns)", lambda: synth_fibonacci(a.big_fib_n, lib=L)))
    out = []
    for name, what, make in loads:
        inp = make()
        be.pool_trim()
        dev = be.upload_input(inp)
        est = estimate_memory(view=inp.view, lib=L)
        mem_reset_peak(L)
        runs = []
        for _ in range(3):
            p = be.prove_device(dev)
            st = p.stats()
            runs.append(st["memory"])
            cells = st["cells"]
            p.free()
        third, first = runs[2], runs[0]
        s = mem_stats(L)
        used_cold = first["peak_live_bytes"] - first["start_live_bytes"]
        entry = {"name": name, "unit": "bytes", "value": first["peak_live_bytes"], "workload": what, "cells": cells,
                 "bytes_per_cell": round(first["peak_live_bytes"] / max(cells, 1), 2),
                 "first_proof": first, "third_proof": third, "driver_allocs_third_proof": third["driver_allocs"],
                 "estimate": est.as_dict(), "estimate_over_peak": round(est.working_bytes / max(used_cold, 1), 3),
                 "peak_phase": max(first["phase_peak_live_bytes"], key=first["phase_peak_live_bytes"].get),
                 "process": {"peak_live_bytes": s.peak_live_bytes, "peak_reserved_bytes": s.peak_reserved_bytes,
                             "pinned_host_bytes": s.pinned_host_bytes}}
        print(json.dumps({k: entry[k] for k in ("name", "value", "bytes_per_cell", "estimate_over_peak", "peak_phase", "driver_allocs_third_proof")}), flush=True)
        out.append(entry)
        be.free_input(dev)
        inp.free()
        be.pool_trim()
    path = os.path.join(ROOT, "profiles", f"{a.set}_mem.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
