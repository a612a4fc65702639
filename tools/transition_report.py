#!/usr/bin/env python3
"""Measurement of the memory transitions (cm_input_open_transition, cm_verify_memory_transition) for a maintainer with a GPU,
against what did the same job before them: two set openings and two set verifications.

    python tools/transition_report.py --out profiles/<set>_transition_report.json

An image of --cells cells (locals and a heap, random values) and, per shape, a second image that differs in --queries seeded
random cells of it (repeats dropped; 2^16 drawn is the set report's shape, 2^10 the small one).  Both trees come from the host
builder and reach the device as the initial and final tree of one uploaded input.  One process, one GPU session, the two sides
timed in alternating blocks.  Recorded per shape, wall ms of the C calls alone:
  transition_open     cm_input_open_transition + cm_mem_transition_get + cm_mem_transition_free
  two_sets_open       cm_input_open_memory_set under the initial tree, then under the final tree
  transition_verify   cm_verify_memory_transition
  two_sets_verify     cm_verify_memory_set of the old values under the root before, then of the new values under the root after
  one_set_verify      the first of those alone: what one fold costs, for reading the other two
and the bytes each side returns (36 n + 4 m against 2 * (20 n + 4 m)).  It asserts that the transition equals the two set
openings word for word and that both sides accept.  No threshold on the times."""
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


def host_tree(L, addresses, values):
    """cm_adapter_partial_tree over (address, value[4]) rows -> (nodes (n, 8), root)"""
    c = np.ascontiguousarray(np.concatenate([addresses.reshape(-1, 1), values], axis=1).astype(np.uint32))
    cap = 8 * c.shape[0] + 64 * 31
    out = np.zeros((cap, 8), dtype=np.uint32)
    n, root = C.c_uint64(0), C.c_uint32(0)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    rc = L.cm_adapter_partial_tree(p(c), C.c_uint32(c.shape[0]), C.c_int32(1), (C.c_uint32 * 6)(), p(out), C.c_uint64(cap), C.byref(n), C.byref(root))
    assert rc == 0, rc
    return out[:n.value].copy(), root.value


def shape(a, be, cells_a, cells_v, tree0, root0, drawn, seed):
    from cairo_m_amd.lib import ArrayInput, MemTransitionViewC, mem_set_plan
    L = be.L
    rng = np.random.default_rng(seed)
    j = np.unique(rng.integers(0, cells_a.size, drawn))
    addrs = np.ascontiguousarray(cells_a[j])                                      # ascending: cells_a is
    n = addrs.size
    after = cells_v.copy()
    after[j] = rng.integers(1, (1 << 31) - 1, (n, 4)).astype(np.uint32)
    after[j[0]] = 0                                                               # a cell written to zero
    tree1, root1 = host_tree(L, cells_a, after)
    dev = be.upload_input(ArrayInput({"initial_tree": tree0, "final_tree": tree1, "roots": [root0, root1]}))
    steps, m = mem_set_plan(addrs, L)
    ap_ = addrs.ctypes.data_as(C.c_void_p)
    old, new = np.zeros((n, 4), dtype=np.uint32), np.zeros((n, 4), dtype=np.uint32)
    w0, w1 = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint32)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)
    need, r0, r1, ok, ok0, ok1, got = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint8(0), C.c_uint8(0), C.c_uint8(0), C.c_uint32(0)
    both = (C.c_uint32 * 2)()
    view = MemTransitionViewC()
    view.struct_size = C.sizeof(MemTransitionViewC)
    kept = {}

    def timed(*calls):
        t0 = time.perf_counter()
        rcs = [fn(*args) for fn, *args in calls]
        dt = (time.perf_counter() - t0) * 1e3
        assert not any(rcs), rcs
        return dt

    def transition_open(keep=False):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rcs = [L.cm_input_open_transition(dev, ap_, C.c_uint64(n), C.byref(h)), L.cm_mem_transition_get(h, C.byref(view))]
        if keep:
            take = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
            kept.update(old=take(view.old_values, 4 * n), new=take(view.new_values, 4 * n), words=take(view.siblings, view.n_siblings),
                        roots=(view.root_before, view.root_after))
        rcs.append(L.cm_mem_transition_free(h))
        dt = (time.perf_counter() - t0) * 1e3
        assert not any(rcs), rcs
        return dt

    set0 = (L.cm_input_open_memory_set, dev, C.c_uint32(0), ap_, C.c_uint64(n), vp(old), vp(w0), C.c_uint32(m), C.byref(need), C.byref(r0))
    set1 = (L.cm_input_open_memory_set, dev, C.c_uint32(1), ap_, C.c_uint64(n), vp(new), vp(w1), C.c_uint32(m), C.byref(need), C.byref(r1))
    ver0 = (L.cm_verify_memory_set, C.c_uint32(root0), ap_, C.c_uint64(n), vp(old), vp(w0), C.c_uint32(m), C.byref(ok0), C.byref(got), C.c_uint64(0))
    ver1 = (L.cm_verify_memory_set, C.c_uint32(root1), ap_, C.c_uint64(n), vp(new), vp(w0), C.c_uint32(m), C.byref(ok1), C.byref(got), C.c_uint64(0))
    dual = (L.cm_verify_memory_transition, C.c_uint32(root0), C.c_uint32(root1), ap_, C.c_uint64(n), vp(old), vp(new), vp(w0), C.c_uint32(m),
            C.byref(ok), both, C.c_uint64(0))
    sides = {"transition_open": transition_open, "two_sets_open": lambda: timed(set0, set1), "transition_verify": lambda: timed(dual),
             "two_sets_verify": lambda: timed(ver0, ver1), "one_set_verify": lambda: timed(ver0)}
    transition_open(keep=True)
    for _ in range(2):                                                            # the pool and the code objects are warm
        for f in sides.values():
            f()
    assert (r0.value, r1.value) == (root0, root1) == kept["roots"] and need.value == m
    assert np.array_equal(w0, w1) and np.array_equal(kept["words"], w0)           # one list of words serves both trees
    assert np.array_equal(kept["old"], old.reshape(-1)) and np.array_equal(kept["new"], new.reshape(-1))
    assert (ok.value, ok0.value, ok1.value) == (1, 1, 1) and tuple(both) == (root0, root1)
    t = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, f in sides.items():
            for _ in range(a.calls):
                t[k].append(f())
    assert (ok.value, ok0.value, ok1.value) == (1, 1, 1)
    be.free_input(dev)
    ms = {k: stats(v) for k, v in t.items()}
    bytes_returned = {"transition": 36 * n + 4 * m, "two_sets": 2 * (20 * n + 4 * m)}
    med = lambda k: ms[k]["median"]
    return {"drawn": drawn, "n_cells": n, "n_siblings": m, "level_launches": sum(1 for s in steps if s["kernel"] == "level"), "blocks": a.blocks,
            "calls_per_block": a.calls, "ms": ms, "bytes_returned": bytes_returned,
            "two_sets_over_transition": {"bytes": round(bytes_returned["two_sets"] / bytes_returned["transition"], 2),
                                         "open": round(med("two_sets_open") / med("transition_open"), 2),
                                         "verify": round(med("two_sets_verify") / med("transition_verify"), 2)},
            "transition_verify_over_one_set_verify": round(med("transition_verify") / med("one_set_verify"), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18)
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--queries", type=int, nargs="+", default=[1 << 16, 1 << 10], help="cells drawn per shape")
    ap.add_argument("--blocks", type=int, default=6, help="alternating blocks per side")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per block and side")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    be = Backend(0)
    rng = np.random.default_rng(1)
    p = (1 << 31) - 1
    n_lo = a.cells - a.heap
    cells_a = np.concatenate([np.arange(n_lo), (1 << 28) - a.heap + np.arange(a.heap)]).astype(np.uint32)   # ascending: the heap lies on top
    cells_v = rng.integers(0, p, (a.cells, 4)).astype(np.uint32)
    tree0, root0 = host_tree(be.L, cells_a, cells_v)
    rep = {"cells": a.cells, "heap_cells": a.heap, "tree_nodes": int(tree0.shape[0]),
           "shapes": [shape(a, be, cells_a, cells_v, tree0, root0, q, 2 + i) for i, q in enumerate(a.queries)]}
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
