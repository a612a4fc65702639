#!/usr/bin/env python3
"""Measurement of the memory openings (cm_run_open_memory, cm_verify_memory_openings, cm_verify_memory_opening) for a maintainer
with a GPU: on an image of --cells cells (locals and a heap, random values) it opens --queries random addresses.

    python tools/open_report.py --out profiles/<set>_open_report.json

One process, one GPU session.  Recorded, wall ms:
  open_first   cm_run_open_memory on a fresh run: the image's tree is built (every cell through the device tree builder), then the
               paths are extracted;
  open_cached  the same call again with the tree cached: upload of the addresses, two launches, download of the records;
  verify_gpu   cm_verify_memory_openings over the records (upload, one launch, download);
  verify_host  a loop of the host cm_verify_memory_opening over the same records in the same process (one ctypes call each).
No threshold: these are first measurements.

    python tools/open_report.py --range --out profiles/<set>_open_range_report.json

The `range` section: on the same image, --queries CONSECUTIVE cells opened and checked as one range (cm_run_open_memory_range with
the image's tree cached, cm_verify_memory_range) against the same cells through cm_run_open_memory + cm_verify_memory_openings,
timed in alternating blocks in one process; medians and the bytes each side returns (16 n + 232 against 136 n).

    python tools/open_report.py --set --out profiles/<set>_open_set_report.json

The `set` section: --queries seeded random cells of the image (repeats dropped) opened and checked as ONE set
(cm_run_open_memory_set with the image's tree cached, cm_verify_memory_set) against the same cells through cm_run_open_memory +
cm_verify_memory_openings, timed in alternating blocks in one process.  It asserts that the set verifies, that a sample of its
sibling words equals the single openings', and that bytes (20 n + 4 m) and hashes (3 n + sum |S_k+1|) are the plan's; it records
open / verify / total medians, bytes returned and hash counts of both sides.  No threshold on the times."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def range_section(a, be, lo, hp):
    from cairo_m_amd.lib import MemOpening, MemRangeOpening
    L = be.L
    n = a.queries
    start = (lo.shape[0] - n) // 2 | 1                                            # odd: the range needs a left sibling at once
    assert start > 0 and start + n <= lo.shape[0], "the range has to lie inside the locals"
    run = be.run_begin(lo, hp, [0, 1, 1, 1, 1, 1])
    addrs = np.arange(start, start + n, dtype=np.uint32)
    ap_, singles, ok_n = addrs.ctypes.data_as(C.c_void_p), (MemOpening * n)(), (C.c_uint8 * n)()
    values = np.zeros((n, 4), dtype=np.uint32)
    vp = values.ctypes.data_as(C.c_void_p)
    rec, ok1, root, root2 = MemRangeOpening(), C.c_uint8(0), C.c_uint32(0), C.c_uint32(0)

    def timed(fn, *args):
        t0 = time.perf_counter()
        rc = fn(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt

    sides = {"range": {"open": lambda: timed(L.cm_run_open_memory_range, run.h, C.c_uint32(start), C.c_uint32(n), vp, C.byref(rec), C.byref(root)),
                       "verify": lambda: timed(L.cm_verify_memory_range, root, C.byref(rec), vp, C.byref(ok1), C.c_uint64(0))},
             "single": {"open": lambda: timed(L.cm_run_open_memory, run.h, ap_, C.c_uint64(n), singles, C.byref(root2)),
                        "verify": lambda: timed(L.cm_verify_memory_openings, root2, singles, C.c_uint64(n), ok_n, C.c_uint64(0))}}
    for side in sides.values():                                                   # the tree is built, the pool and the code objects are warm
        for _ in range(2):
            side["open"](); side["verify"]()
    assert root.value == root2.value and ok1.value == 1 and all(ok_n)
    assert np.array_equal(values, lo[start:start + n])
    assert all(list(singles[i].value) == values[i].tolist() for i in (0, n // 2, n - 1))
    t = {f"{k}_{what}": [] for k in sides for what in ("open", "verify")}
    for _ in range(a.blocks):
        for k, side in sides.items():
            for _ in range(a.calls):
                t[f"{k}_open"].append(side["open"]())
                t[f"{k}_verify"].append(side["verify"]())
    assert ok1.value == 1 and all(ok_n)
    run.free()
    ms = {k: stats(v) for k, v in t.items()}
    rep = {"cells": a.cells, "heap_cells": a.heap, "range": {
        "start": int(start), "n_cells": n, "blocks": a.blocks, "calls_per_block": a.calls, "ms": ms,
        "bytes_returned": {"range": 16 * n + C.sizeof(MemRangeOpening), "single": C.sizeof(MemOpening) * n},
        "total_ms": {k: round(ms[f"{k}_open"]["median"] + ms[f"{k}_verify"]["median"], 4) for k in sides}}}
    r = rep["range"]
    r["single_over_range"] = {what: round(ms[f"single_{what}"]["median"] / ms[f"range_{what}"]["median"], 2) for what in ("open", "verify")}
    r["single_over_range"]["total"] = round(r["total_ms"]["single"] / r["total_ms"]["range"], 2)
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


def set_section(a, be, lo, hp):
    from cairo_m_amd.lib import MemOpening, mem_set_plan
    L = be.L
    n_lo, space = lo.shape[0], 1 << 28
    j = np.unique(np.random.default_rng(2).integers(0, a.cells, a.queries))
    addrs = np.ascontiguousarray(np.where(j < n_lo, j, space - a.heap + (j - n_lo)).astype(np.uint32))   # ascending: the heap lies on top
    n = addrs.shape[0]
    steps, m = mem_set_plan(addrs, L)
    run = be.run_begin(lo, hp, [0, 1, 1, 1, 1, 1])
    ap_, singles, ok_n = addrs.ctypes.data_as(C.c_void_p), (MemOpening * n)(), (C.c_uint8 * n)()
    values, words = np.zeros((n, 4), dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    vp, wp = values.ctypes.data_as(C.c_void_p), words.ctypes.data_as(C.c_void_p)
    need, ok1, got, root, root2 = C.c_uint32(0), C.c_uint8(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)

    def timed(fn, *args):
        t0 = time.perf_counter()
        rc = fn(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt

    sides = {"set": {"open": lambda: timed(L.cm_run_open_memory_set, run.h, ap_, C.c_uint64(n), vp, wp, C.c_uint32(m), C.byref(need), C.byref(root)),
                     "verify": lambda: timed(L.cm_verify_memory_set, root, ap_, C.c_uint64(n), vp, wp, C.c_uint32(m), C.byref(ok1), C.byref(got),
                                             C.c_uint64(0))},
             "single": {"open": lambda: timed(L.cm_run_open_memory, run.h, ap_, C.c_uint64(n), singles, C.byref(root2)),
                        "verify": lambda: timed(L.cm_verify_memory_openings, root2, singles, C.c_uint64(n), ok_n, C.c_uint64(0))}}
    for side in sides.values():                                                   # the tree is built, the pool and the code objects are warm
        for _ in range(2):
            side["open"](); side["verify"]()
    assert root.value == root2.value == got.value and ok1.value == 1 and all(ok_n) and need.value == m
    assert all(list(singles[i].value) == values[i].tolist() for i in (0, n // 2, n - 1))
    # a sample of sibling words against the single openings: word q of depth 28 - k belongs to a node x = addrs[i] >> k
    a_list, q, checked = addrs.tolist(), 0, 0
    for k in range(28):
        x = np.unique(addrs >> k)
        lone = x[~np.isin(x ^ 1, x)]
        assert lone.size == steps[k + 1]["n_siblings"]
        for pos in sorted({0, lone.size // 2, lone.size - 1}) if lone.size else ():
            i = int(np.searchsorted(addrs, int(lone[pos]) << k))
            assert a_list[i] >> k == int(lone[pos]) and int(words[q + pos]) == singles[i].siblings[k], (k, pos)
            checked += 1
        q += lone.size
    assert q == m
    hashes = {"set": 3 * n + sum(s["n_nodes"] for s in steps[1:]), "single": 31 * n}
    bytes_returned = {"set": 20 * n + 4 * m, "single": C.sizeof(MemOpening) * n}
    assert bytes_returned["set"] == addrs.nbytes + values.nbytes + words.nbytes
    t = {f"{k}_{what}": [] for k in sides for what in ("open", "verify")}
    for _ in range(a.blocks):
        for k, side in sides.items():
            for _ in range(a.calls):
                t[f"{k}_open"].append(side["open"]())
                t[f"{k}_verify"].append(side["verify"]())
    assert ok1.value == 1 and all(ok_n)
    run.free()
    ms = {k: stats(v) for k, v in t.items()}
    rep = {"cells": a.cells, "heap_cells": a.heap, "set": {
        "drawn": a.queries, "n_cells": n, "n_siblings": m, "sibling_words_checked": checked, "blocks": a.blocks, "calls_per_block": a.calls,
        "level_launches": sum(1 for s in steps if s["kernel"] == "level"), "ms": ms, "bytes_returned": bytes_returned, "hashes": hashes,
        "total_ms": {k: round(ms[f"{k}_open"]["median"] + ms[f"{k}_verify"]["median"], 4) for k in sides}}}
    r = rep["set"]
    r["single_over_set"] = {what: round(ms[f"single_{what}"]["median"] / ms[f"set_{what}"]["median"], 2) for what in ("open", "verify")}
    r["single_over_set"]["total"] = round(r["total_ms"]["single"] / r["total_ms"]["set"], 2)
    r["single_over_set"]["bytes"] = round(bytes_returned["single"] / bytes_returned["set"], 2)
    r["single_over_set"]["hashes"] = round(hashes["single"] / hashes["set"], 2)
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18)
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--queries", type=int, default=1 << 16)
    ap.add_argument("--runs", type=int, default=3, help="fresh runs (each gives one open_first)")
    ap.add_argument("--calls", type=int, default=5, help="timed calls of the cached opening and of the GPU verifier per run")
    ap.add_argument("--range", action="store_true", help="the range section instead: one range against the same cells one by one")
    ap.add_argument("--set", action="store_true", help="the set section instead: one set of random cells against the same cells one by one")
    ap.add_argument("--blocks", type=int, default=6, help="alternating blocks per side of the range and the set section")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import MemOpening
    be = Backend(0)
    L = be.L
    rng = np.random.default_rng(1)
    p = (1 << 31) - 1
    lo = rng.integers(0, p, (a.cells - a.heap, 4)).astype(np.uint32)
    hp = rng.integers(0, p, (a.heap, 4)).astype(np.uint32)
    lo[0] = [11, 0, 0, 0]
    # half of the queries inside the image, half anywhere in the address space (mostly absent cells)
    inside = np.concatenate([rng.integers(0, lo.shape[0], a.queries // 4), (1 << 28) - 1 - rng.integers(0, a.heap, a.queries // 4)])
    addrs = np.concatenate([inside, rng.integers(0, 1 << 28, a.queries - inside.size)]).astype(np.uint32)
    rng.shuffle(addrs)
    if a.range:
        return range_section(a, be, lo, hp)
    if a.set:
        return set_section(a, be, lo, hp)
    t = {"open_first": [], "open_cached": [], "verify_gpu": [], "verify_host": []}
    n_ok = None
    for r in range(a.runs + 1):                                                   # (run 0 warms the pool and the code objects)
        run = be.run_begin(lo, hp, [0, 1, 1, 1, 1, 1])
        n = addrs.shape[0]
        ap_, buf, again = addrs.ctypes.data_as(C.c_void_p), (MemOpening * n)(), (MemOpening * n)()
        ok, root, root2 = (C.c_uint8 * n)(), C.c_uint32(0), C.c_uint32(0)

        def timed(fn, *args):                                                     # the C call alone, without the Python wrappers' copies
            t0 = time.perf_counter()
            rc = fn(*args)
            dt = (time.perf_counter() - t0) * 1e3
            assert rc == 0, rc
            return dt

        first = timed(L.cm_run_open_memory, run.h, ap_, C.c_uint64(n), buf, C.byref(root))
        cached = [timed(L.cm_run_open_memory, run.h, ap_, C.c_uint64(n), again, C.byref(root2)) for _ in range(a.calls)]
        assert root2.value == root.value and bytes(again) == bytes(buf)
        gpu = [timed(L.cm_verify_memory_openings, root, buf, C.c_uint64(n), ok, C.c_uint64(0)) for _ in range(a.calls)]
        assert all(ok)
        n_ok = n
        root = root.value
        run.free()
        if r == 0:
            continue
        t["open_first"].append(first)
        t["open_cached"] += cached
        t["verify_gpu"] += gpu
        if r == 1:                                                                # the host loop once: it is seconds long
            fn, size, base = L.cm_verify_memory_opening, C.sizeof(MemOpening), C.addressof(buf)
            fn.argtypes = [C.c_uint32, C.c_void_p]
            t0 = time.perf_counter()
            bad = 0
            for i in range(n):
                bad += fn(root, base + i * size)
            t["verify_host"].append((time.perf_counter() - t0) * 1e3)
            fn.argtypes = None
            assert bad == 0
    rep = {"cells": a.cells, "heap_cells": a.heap, "queries": a.queries, "accepted": n_ok, "ms": {k: stats(v) for k, v in t.items()}}
    rep["tree_build_ms"] = round(rep["ms"]["open_first"]["median"] - rep["ms"]["open_cached"]["median"], 4)
    rep["verify_host_over_gpu"] = round(rep["ms"]["verify_host"]["median"] / rep["ms"]["verify_gpu"]["median"], 2)
    rep["us_per_opening"] = {k: round(1e3 * rep["ms"][k]["median"] / a.queries, 4) for k in ("open_cached", "verify_gpu", "verify_host")}
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
