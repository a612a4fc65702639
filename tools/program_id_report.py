#!/usr/bin/env python3
"""Program ids, three routes timed in one process on one GPU (wall clock around each call, the routes alternating block by block):
  device    cm_program_ids: the whole batch in one call (one upload, k_pid_cells, k_pid_tree, one download)
  host      a loop of cm_program_id_entries: the same fold in host code
  tree      a loop of cm_adapter_partial_tree over the same cells with zero ranges: the route without this feature
Shapes: 64 programs of 2^12 cells (a cm_verify_many-sized batch), and 1 program of 2^16 cells.  Every route's ids are compared
before anything is timed.  Writes one JSON document (default profiles/r12_program_id_report.json)."""
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

from cairo_m_amd import Backend                                                  # noqa: E402
from cairo_m_amd.lib import program_entries, program_id                         # noqa: E402

P = (1 << 31) - 1


def programs(n_programs, n_cells, seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_programs):
        v = rng.integers(0, P, size=(n_cells, 4), dtype=np.uint64).astype(np.uint32)
        v[:, 0] |= 1
        v[v >= P] = P - 1
        out.append(program_entries(0, v))
    return out


def tree_route(L, cells, out, cap):
    n, root = C.c_uint64(0), C.c_uint32(0)
    rc = L.cm_adapter_partial_tree(cells.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(cells.shape[0]), C.c_int32(1), (C.c_uint32 * 6)(),
                                   out.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(cap), C.byref(n), C.byref(root))
    assert rc == 0, rc
    return root.value


def measure(B, items, blocks, calls):
    L = B.L
    cells = [np.ascontiguousarray(e[:, 1:6]) for e in items]                    # (address, v0..v3) rows, made outside the timing
    cap = 8 * max(c.shape[0] for c in cells) + 64
    out = np.zeros((cap, 8), dtype=np.uint32)
    routes = {
        "device": lambda: B.program_ids(items).tolist(),
        "host": lambda: [program_id(e, L) for e in items],
        "tree": lambda: [tree_route(L, c, out, cap) for c in cells],
    }
    want = routes["host"]()
    for name, f in routes.items():
        assert f() == want, name                                                # (also the warm-up of every route)
    ms = {name: [] for name in routes}
    for _ in range(blocks):
        for name, f in routes.items():
            for _ in range(calls):
                t0 = time.perf_counter()
                f()
                ms[name].append((time.perf_counter() - t0) * 1e3)
    stat = {name: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)} for name, v in ms.items()}
    med = {name: s["median"] for name, s in stat.items()}
    return {"n_programs": len(items), "cells_per_program": int(items[0].shape[0]), "blocks": blocks, "calls_per_block": calls, "ms": stat,
            "host_over_device": round(med["host"] / med["device"], 2), "tree_over_device": round(med["tree"] / med["device"], 2),
            "tree_over_host": round(med["tree"] / med["host"], 2)}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_program_id_report.json"))
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    a = ap.parse_args()
    B = Backend(0)
    doc = {"batch_64_x_4096": measure(B, programs(64, 1 << 12, 1), a.blocks, a.calls),
           "one_x_65536": measure(B, programs(1, 1 << 16, 2), a.blocks, a.calls)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
