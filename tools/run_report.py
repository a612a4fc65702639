#!/usr/bin/env python3
"""Measurement of the run layer (header revision 10): wall ms per segment of cm_prove_run against cm_prove_many_segments at
inflight 1 and 4, on (a) fibonacci_loop(419 000) cut into 8 segments (a memory of a few dozen cells) and (b)
scatter_store_program at --cells memory cells cut into 8 (memory-heavy), plus host-to-device bytes per segment and, for (b),
the host time of the segment adapter's tail (CM_ADAPTER_TAIL_LOG lines of adapter_device.hip step 5).

    python tools/run_report.py --baseline cairo_m_amd/libcairom_hip_parent.so --out profiles/<tag>_run_report.json

Every leg is a fresh process (CAIROM_HIP_LIB selects the build, as tools/ab_libs.py does); the baseline build — the parent commit's
library, which only has cm_prove_many_segments — and this build run alternately, `--rounds` times each, in one GPU session.
Inside a process the two entry points are timed in alternating blocks (the style of tools/ab_switch.py)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def leg(a):
    """one process, one build: prints one JSON line"""
    import ctypes as C
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import runner_segment_arrays, synth_fibonacci_segment, vm_segment
    from tests.test_gpu_adapter import scatter_store_program
    be = Backend(0)
    has_run = hasattr(be.L, "cm_prove_run")
    out = {"lib": os.environ.get("CAIROM_HIP_LIB", "in-tree"), "has_run": has_run, "runs": {}}
    for name in a.runs.split(","):
        if name == "a":
            n_steps = 10 * 419_000 + 12
            ms = -(-n_steps // 8)
            segs = [synth_fibonacci_segment(419_000, max_steps=ms, segment=s) for s in range(8)]
        else:
            prog = scatter_store_program(a.cells)
            n_steps = 4 + 7 * a.cells + 1
            ms = -(-n_steps // 8)
            segs = [vm_segment(prog, max_steps=ms, segment=s) for s in range(8)]
        arrs = [runner_segment_arrays(s.view) for s in segs]
        log_bytes = [x["trace"].nbytes + x["memory_trace"].nbytes for x in arrs]
        mem_bytes = [x["initial_memory"].nbytes + x["initial_heap"].nbytes for x in arrs]
        r = {"segments": len(segs), "steps": n_steps,
             "h2d_bytes_per_segment": {"prove_many_segments": (sum(log_bytes) + sum(mem_bytes)) / len(segs),
                                       "prove_run": (sum(log_bytes) + mem_bytes[0]) / len(segs)},
             "memory_cells_at_start_of_last_segment": int(mem_bytes[-1] // 16), "ms_per_segment": {}}
        del arrs
        forms = ["segments"] + (["run"] if has_run else [])
        for inflight in (1, 4):
            times = {f: [] for f in forms}
            for block in range(a.warmup + a.blocks):
                for f in (forms if block % 2 == 0 else forms[::-1]):
                    t0 = time.perf_counter()
                    proofs = be.prove_many_segments(segs, inflight=inflight) if f == "segments" else be.prove_run(segs, inflight=inflight)
                    dt = (time.perf_counter() - t0) * 1e3 / len(segs)
                    for p in proofs:
                        p.free()
                    if block >= a.warmup:
                        times[f].append(dt)
            r["ms_per_segment"][f"inflight{inflight}"] = {f: {"median": statistics.median(v), "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}
                                                          for f, v in times.items()}
        out["runs"][name] = r
        for s in segs:
            s.free()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true", help="worker: time the build CAIROM_HIP_LIB names and print one JSON line")
    ap.add_argument("--baseline", help="the parent commit's libcairom_hip.so")
    ap.add_argument("--runs", default="a,b")
    ap.add_argument("--cells", type=int, default=1 << 20, help="memory cells of run (b)")
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--leg-timeout", type=int, default=500)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    libs = {"new": os.path.join(ROOT, "cairo_m_amd", "libcairom_hip.so")}
    if a.baseline:
        libs["baseline"] = os.path.abspath(a.baseline)
    order = list(libs)
    legs = {k: [] for k in libs}
    tails = []
    for rnd in range(a.rounds):
        for k in (order if rnd % 2 == 0 else order[::-1]):
            env = dict(os.environ, CAIROM_HIP_LIB=libs[k])
            if k == "new":
                env["CM_ADAPTER_TAIL_LOG"] = "1"
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--runs", a.runs, "--cells", str(a.cells), "--blocks", str(a.blocks),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, cwd=ROOT, timeout=a.leg_timeout)
            if p.returncode != 0:      # a failed leg ends the session: nothing more is started on the GPU
                print(k, "leg FAILED", p.returncode, p.stderr[-2000:], file=sys.stderr)
                return 1
            legs[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
            if k == "new":
                rows_ms = [(int(l.split()[3]), float(l.split()[1])) for l in p.stderr.splitlines() if l.startswith("cm_adapter_tail_host_ms")]
                tails.append(rows_ms)
            print(k, "round", rnd, json.dumps({n: r["ms_per_segment"] for n, r in legs[k][-1]["runs"].items()}), flush=True)
    rep = {"cells_b": a.cells, "blocks": a.blocks, "rounds": a.rounds, "legs": legs, "summary": {}}
    for name in a.runs.split(","):
        s = {}
        for inf in ("inflight1", "inflight4"):
            med = lambda k, f: [l["runs"][name]["ms_per_segment"][inf][f]["median"] for l in legs.get(k, []) if f in l["runs"][name]["ms_per_segment"][inf]]
            base = med("baseline", "segments")
            s[inf] = {"baseline_prove_many_segments_ms": base, "baseline_spread_ms": (max(base) - min(base)) if base else None,
                      "new_prove_many_segments_ms": med("new", "segments"), "new_prove_run_ms": med("new", "run")}
        s["h2d_bytes_per_segment"] = legs["new"][0]["runs"][name]["h2d_bytes_per_segment"]
        rep["summary"][name] = s
    if tails:
        big = [ms for t in tails for rows, ms in t if rows >= 2048]
        rep["segment_adapter_host_tail_ms"] = {"segments_with_2048_rows_or_more": len(big), "median": statistics.median(big) if big else None,
                                               "max": max(big) if big else None}
    text = json.dumps(rep, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    print(json.dumps(rep["summary"], indent=1))
    if "segment_adapter_host_tail_ms" in rep:
        print(json.dumps(rep["segment_adapter_host_tail_ms"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
