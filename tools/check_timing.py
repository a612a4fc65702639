#!/usr/bin/env python3
"""Cost of the PCS-free AIR check (cm_check_constraints) against a proof (cm_prove_device) of the same device-resident input, at
the metric config (fibonacci 419 000: 4 190 012 steps) — alternating blocks in ONE process, so that clocks, pools and caches are
shared by both sides — then the per-kernel split of the check (cm_kprof_report, a run of its own after the timed blocks) and, with
--configs4, one check of configs[4] (all_opcodes_program(1_545_000), 2^26 rows).  Every timed call ends in a device synchronise
(both entry points return after their last copy).  Prints one JSON object; --out writes it to a file too.

usage: tools/check_timing.py [--blocks 6] [--per-block 5] [--configs4] [--out profiles/check_timing.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--per-block", type=int, default=5)
    ap.add_argument("--configs4", action="store_true")
    ap.add_argument("--out")
    args = ap.parse_args()
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import synth_fibonacci, vm_segment
    from cairo_m_amd.workloads import all_opcodes_program
    be = Backend(0)
    inp = synth_fibonacci(419_000)
    dev = be.upload_input(inp)

    def check():
        t = time.perf_counter()
        rep = be.check(dev)
        dt = (time.perf_counter() - t) * 1e3
        assert rep.status == 0, rep.message
        return dt

    def prove():
        t = time.perf_counter()
        p = be.prove_device(dev)
        dt = (time.perf_counter() - t) * 1e3
        p.free()
        return dt

    for _ in range(3):   # warm-up: code objects, the device pool's blocks of both shapes
        check()
        prove()
    t_check, t_prove = [], []
    for b in range(args.blocks):
        order = (check, prove) if b % 2 == 0 else (prove, check)
        for f in order:
            dst = t_check if f is check else t_prove
            dst.extend(f() for _ in range(args.per_block))
    out = {"steps": inp.steps, "blocks": args.blocks, "per_block": args.per_block,
           "check_ms": {"median": statistics.median(t_check), "min": min(t_check), "max": max(t_check)},
           "prove_ms": {"median": statistics.median(t_prove), "min": min(t_prove), "max": max(t_prove)}}
    out["check_over_prove"] = out["check_ms"]["median"] / out["prove_ms"]["median"]
    # per-kernel split of the check (timing events on the launch stream: a run of its own)
    be.L.cm_kprof_enable(C.c_int32(1))
    for _ in range(3):
        check()
    buf = C.create_string_buffer(1 << 16)
    be.L.cm_kprof_report(buf, C.c_size_t(len(buf)))
    be.L.cm_kprof_enable(C.c_int32(0))
    try:
        out["check_kprof_3_calls"] = json.loads(buf.value.decode())
    except ValueError:
        out["check_kprof_3_calls"] = buf.value.decode()
    be.free_input(dev)
    inp.free()
    if args.configs4:
        f, t = C.c_uint64(0), C.c_uint64(0)
        be.L.cm_device_mem_info(C.byref(f), C.byref(t))
        if f.value < 150 * 2**30:
            out["configs4"] = "skipped: less than 150 GiB of free HBM"
        else:
            prog, steps = all_opcodes_program(1_545_000)
            hs = vm_segment(prog, entry_pc=0, args=(), n_returns=0)
            d4 = be.adapt_segment(hs)
            hs.free()
            t0 = time.perf_counter()
            rep = be.check(d4)
            first = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            rep = be.check(d4)
            second = (time.perf_counter() - t0) * 1e3
            out["configs4"] = {"steps": steps, "status": rep.status, "check_ms_first": first, "check_ms_second": second}
            be.free_input(d4)
            be.L.cm_pool_trim()
    s = json.dumps(out, indent=1)
    print(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(s + "\n")


if __name__ == "__main__":
    main()
