#!/usr/bin/env python3
"""Measurement of the whole-run check (cm_check_run, cm_link_diff) on the two runs of tools/run_report.py: (a)
fibonacci_loop(419 000) cut into 8 segments (a memory of a few dozen cells) and (b) scatter_store_program at --cells memory
cells cut into 8 (memory-heavy; its links are broken, every segment first-writes fresh cells).

    python tools/run_check_report.py --out profiles/<tag>_run_check_report.json

One process, one GPU session.  Per run, wall ms per segment of Run.check against Run.prove at inflight 1 in alternating blocks
(the style of tools/ab_switch.py); then, with every segment's input resident, cm_link_diff of link i against cm_check_constraints
of segment i, alternating call by call."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="a,b")
    ap.add_argument("--cells", type=int, default=1 << 18, help="memory cells of run (b)")
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--calls", type=int, default=7, help="timed calls per link of the link diff / the segment's check")
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import Run, link_diff, synth_fibonacci_segment, vm_segment
    from tests.test_gpu_adapter import scatter_store_program
    be = Backend(0)
    rep = {"cells_b": a.cells, "blocks": a.blocks, "calls": a.calls, "cap": a.cap, "runs": {}}
    for name in a.runs.split(","):
        if name == "a":
            n_steps = 10 * 419_000 + 12
            mk = lambda s, ms: synth_fibonacci_segment(419_000, max_steps=ms, segment=s)
        else:
            prog = scatter_store_program(a.cells)
            n_steps = 4 + 7 * a.cells + 1
            mk = lambda s, ms: vm_segment(prog, max_steps=ms, segment=s)
        ms = -(-n_steps // 8)
        segs = [mk(s, ms) for s in range(8)]
        r = {"segments": len(segs), "steps": n_steps}
        # ---- the whole run: checked against proved ----
        times = {"check_run": [], "prove_run": []}
        forms = list(times)
        verdict = None
        for block in range(a.warmup + a.blocks):
            for f in (forms if block % 2 == 0 else forms[::-1]):
                run = Run.from_segment(be, segs[0])
                t0 = time.perf_counter()
                if f == "check_run":
                    verdict = run.check(segs, cap=a.cap)
                else:
                    proofs = run.prove(segs, inflight=1)
                dt = (time.perf_counter() - t0) * 1e3 / len(segs)
                run.free()
                if f == "prove_run":
                    for p in proofs:
                        p.free()
                if block >= a.warmup:
                    times[f].append(dt)
        r["ms_per_segment"] = {f: stats(v) for f, v in times.items()}
        r["check_over_prove"] = round(r["ms_per_segment"]["check_run"]["median"] / r["ms_per_segment"]["prove_run"]["median"], 4)
        r["summary"] = verdict.summary
        r["air_status"] = [s.check.status for s in verdict.segments]
        r["link_cells_total"] = [s.link.n_total if s.link else 0 for s in verdict.segments]
        # ---- one link against its segment's check, inputs resident ----
        run = Run.from_segment(be, segs[0])
        devs = [run.adapt_next(s) for s in segs]
        links = []
        for i in range(1, len(devs)):
            t = {"link_diff": [], "check_constraints": []}
            for k in range(2 + a.calls):
                for f in (("link_diff", "check_constraints") if k % 2 == 0 else ("check_constraints", "link_diff")):
                    t0 = time.perf_counter()
                    if f == "link_diff":
                        d = link_diff(devs[i - 1], devs[i], a.cap, lib=be.L)
                    else:
                        be.check(devs[i])
                    dt = (time.perf_counter() - t0) * 1e3
                    if k >= 2:
                        t[f].append(dt)
            links.append({"link": i, "cells_listed": d.n_total, "zero_only": int(d.report.n_zero_only),
                          "link_diff_ms": stats(t["link_diff"]), "check_constraints_ms": stats(t["check_constraints"])})
        r["links"] = links
        r["link_diff_ms_median_of_links"] = round(statistics.median(l["link_diff_ms"]["median"] for l in links), 4)
        r["check_constraints_ms_median_of_links"] = round(statistics.median(l["check_constraints_ms"]["median"] for l in links), 4)
        for d in devs:
            be.free_input(d)
        run.free()
        for s in segs:
            s.free()
        rep["runs"][name] = r
        print(name, json.dumps({k: r[k] for k in ("ms_per_segment", "check_over_prove", "link_diff_ms_median_of_links",
                                                    "check_constraints_ms_median_of_links", "summary")}), flush=True)
    text = json.dumps(rep, indent=1)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
