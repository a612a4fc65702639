#!/usr/bin/env python3
"""Cost of the PCS-free AIR check (cm_check_constraints) against a proof (cm_prove_device) of the same device-resident input, at
the metric config (fibonacci 419 000: 4 190 012 steps) — alternating blocks in ONE process, so that clocks, pools and caches are
shared by both sides — with a third leg, check + relation tracker on a tampered copy of the input (one prev_value changed: the
memory relation is tracked), then the tracker with every relation forced (mask 0xFF) on the valid input, the per-kernel split of
both tracker shapes and of the check (cm_kprof_report, a run of its own after the timed blocks) and, with
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
    from cairo_m_amd.lib import ArrayInput, prover_input_arrays, synth_fibonacci, vm_segment
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

    # the tampered input of tests/test_gpu_track.py: prev_value of the destination access of StoreFpFp row 300 000
    a = prover_input_arrays(inp.view)
    i = int(a["bundles6"][300_000][10]) + 2
    a["data_accesses"][i][2] = (int(a["data_accesses"][i][2]) + 1) % (2**31 - 1)
    bad = ArrayInput(a)
    dev_bad = be.upload_input(bad)

    def track():
        t = time.perf_counter()
        s = be.track_relations(dev_bad)
        dt = (time.perf_counter() - t) * 1e3
        assert s.report.status == 3 and s.n_total == 2, str(s)
        return dt

    def track_all():
        t = time.perf_counter()
        s = be.track_relations(dev, mask=0xFF)
        dt = (time.perf_counter() - t) * 1e3
        assert s.report.status == 0 and s.n_total == 0, str(s)
        return dt

    def kprof(f, calls=3):
        be.L.cm_kprof_enable(C.c_int32(1))
        for _ in range(calls):
            f()
        buf = C.create_string_buffer(1 << 16)
        be.L.cm_kprof_report(buf, C.c_size_t(len(buf)))
        be.L.cm_kprof_enable(C.c_int32(0))
        try:
            rep = json.loads(buf.value.decode())
        except ValueError:
            return buf.value.decode()
        return {k: v for k, v in rep.items() if k.startswith("k_track")}

    def prove():
        t = time.perf_counter()
        p = be.prove_device(dev)
        dt = (time.perf_counter() - t) * 1e3
        p.free()
        return dt

    for _ in range(3):   # warm-up: code objects, the device pool's blocks of both shapes
        check()
        prove()
        track()
    t_check, t_prove, t_track = [], [], []
    legs = [(check, t_check), (prove, t_prove), (track, t_track)]
    for b in range(args.blocks):
        for f, dst in legs[b % 3:] + legs[:b % 3]:
            dst.extend(f() for _ in range(args.per_block))
    track_all()
    t_all = [track_all() for _ in range(args.per_block)]

    def stats(t):
        return {"median": statistics.median(t), "min": min(t), "max": max(t)}
    out = {"steps": inp.steps, "blocks": args.blocks, "per_block": args.per_block,
           "check_ms": stats(t_check), "prove_ms": stats(t_prove), "track_tampered_ms": stats(t_track), "track_all_relations_ms": stats(t_all)}
    out["check_over_prove"] = out["check_ms"]["median"] / out["prove_ms"]["median"]
    # per-kernel split of the tracker (bytes = algorithmic; k_track_net moves 32 bytes per record: records = bytes / 32 / calls)
    out["track_tampered_kprof_3_calls"] = kprof(track)
    out["track_all_relations_kprof_3_calls"] = kprof(track_all)
    for key in ("track_tampered_kprof_3_calls", "track_all_relations_kprof_3_calls"):
        k = out[key]
        if isinstance(k, dict) and "k_track_net" in k:
            out[key.replace("kprof_3_calls", "records")] = int(k["k_track_net"]["bytes"] / 32 / 3)
            ms = sum(v["ms"] for n, v in k.items() if n != "k_track_recover")
            out[key.replace("kprof_3_calls", "gbytes_per_s")] = sum(v["bytes"] for v in k.values()) / ms / 1e6 if ms else None
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
    be.free_input(dev_bad)
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
