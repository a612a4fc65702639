#!/usr/bin/env python3
"""Measurement of followed memory (cm_mem_image_apply) for a maintainer with a GPU, against what a follower had to do before it:
verify the full transition record on the GPU and build a fresh tree over all cells.

    python tools/image_report.py --out profiles/<set>_image_report.json

An image of --cells cells (locals and a heap, random values) on the GPU and, per shape, an update of --queries seeded random cells
of it (repeats dropped; the shapes of tools/transition_report.py: 2^16 drawn and 2^10 drawn).  One process, one GPU session, the
sides timed in alternating blocks.  Recorded per shape, wall ms of the C calls alone:
  apply_bare          cm_mem_image_apply of (addresses, new values) with both roots given, no old values: what a follower that holds
                      the tree does with 20 n bytes.  The image goes forth (old -> new) and back (new -> old) in turn, so every
                      call is an update of the same cells between the same two roots.
  verify_full         cm_verify_memory_transition of the full record (36 n + 4 m bytes)
  fresh_tree          cm_mem_image_create over every cell of the updated memory: the device tree builder over all cells, which is
                      what cm_run pays on the first opening after an advance
  open_followed       one cm_mem_image_open_memory of --opens cells under the followed image
  open_fresh          the same call under the freshly built image
verify_then_rebuild = verify_full + fresh_tree is the follower's cost before.  It asserts that the followed image and the fresh
one agree in root and node words, that the record the image re-emits verifies, and that both openings are the same bytes.  No
threshold on the times."""
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


def shape(a, be, image, cells_a, cells_v, drawn, seed):
    from cairo_m_amd.lib import MemImage, MemOpening, mem_set_plan, verify_transition
    L = be.L
    rng = np.random.default_rng(seed)
    j = np.unique(rng.integers(0, cells_a.size, drawn))
    addrs = np.ascontiguousarray(cells_a[j])                                      # ascending: cells_a is
    n = addrs.size
    old = np.ascontiguousarray(cells_v[j])
    new = rng.integers(1, (1 << 31) - 1, (n, 4)).astype(np.uint32)
    new[0] = 0                                                                    # a cell written to zero
    after = cells_v.copy()
    after[j] = new
    steps, m = mem_set_plan(addrs, L)
    root0 = image.root
    root1, record = image.apply(addrs, new, old_values=old, root_before=root0, record=True)
    assert verify_transition(record, L) and record.siblings.size == m
    fresh = MemImage.from_cells(np.concatenate([cells_a.reshape(-1, 1), after], axis=1), L)
    assert fresh.root == root1 and np.array_equal(fresh.nodes()[:, :5], image.nodes()[:, :5])
    fresh.free()
    image.apply(addrs, old, root_before=root1, root_after=root0)
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    word = lambda x: C.byref(C.c_uint32(x))
    out, ok, both, h = C.c_uint32(0), C.c_uint8(0), (C.c_uint32 * 2)(), C.c_void_p()
    flat_after = np.ascontiguousarray(after).reshape(-1)
    opens = np.ascontiguousarray(rng.choice(cells_a, a.opens, replace=False).astype(np.uint32))
    rec_f, rec_b, r = (MemOpening * a.opens)(), (MemOpening * a.opens)(), C.c_uint32(0)
    at_new = [False]

    def timed(fn, *args):
        t0 = time.perf_counter()
        rc = fn(*args)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt

    def apply_bare():
        v, rb, ra = (old, root1, root0) if at_new[0] else (new, root0, root1)
        dt = timed(L.cm_mem_image_apply, image.h, p(addrs), p(v), C.c_uint64(n), None, word(rb), word(ra), C.byref(out), None)
        at_new[0] = not at_new[0]
        return dt

    def verify_full():
        return timed(L.cm_verify_memory_transition, C.c_uint32(root0), C.c_uint32(root1), p(addrs), C.c_uint64(n), p(record.old_values),
                     p(record.new_values), p(record.siblings), C.c_uint32(m), C.byref(ok), both, C.c_uint64(0))

    def fresh_tree(keep=False):
        dt = timed(L.cm_mem_image_create, p(cells_a), p(flat_after), C.c_uint64(cells_a.size), C.c_uint32(1), C.byref(h))
        if not keep:
            L.cm_mem_image_free(h)
        return dt

    def open_followed():
        return timed(L.cm_mem_image_open_memory, image.h, p(opens), C.c_uint64(a.opens), rec_f, C.byref(r))

    def open_fresh():
        fresh_tree(keep=True)
        dt = timed(L.cm_mem_image_open_memory, h, p(opens), C.c_uint64(a.opens), rec_b, C.byref(r))
        L.cm_mem_image_free(h)
        return dt

    sides = {"apply_bare": apply_bare, "verify_full": verify_full, "fresh_tree": fresh_tree, "open_followed": open_followed, "open_fresh": open_fresh}
    for _ in range(2):                                                            # the pool and the code objects are warm
        for f in sides.values():
            f()
    assert ok.value == 1 and tuple(both) == (root0, root1)
    t = {k: [] for k in sides}
    for _ in range(a.blocks):
        for k, f in sides.items():
            for _ in range(a.calls):
                t[k].append(f())
    if not at_new[0]:
        apply_bare()
    open_followed()
    open_fresh()
    assert bytes(rec_f) == bytes(rec_b) and r.value == root1                      # the followed image opens like the fresh one
    apply_bare()                                                                  # back at root0 for the next shape
    assert image.root == root0
    ms = {k: stats(v) for k, v in t.items()}
    med = lambda k: ms[k]["median"]
    before = med("verify_full") + med("fresh_tree")
    travel = {"bare_update": 20 * n, "full_transition": 36 * n + 4 * m}
    return {"drawn": drawn, "n_cells": n, "n_siblings": m, "level_launches": sum(1 for s in steps if s["kernel"] == "level"),
            "dirty_records": 3 * n + sum(s["n_nodes"] for s in steps[1:]), "opens": a.opens, "blocks": a.blocks, "calls_per_block": a.calls, "ms": ms,
            "bytes_that_travel": travel, "verify_then_rebuild_ms": round(before, 4),
            "verify_then_rebuild_over_apply": {"time": round(before / med("apply_bare"), 2),
                                               "bytes": round(travel["full_transition"] / travel["bare_update"], 2)},
            "open_fresh_over_open_followed": round(med("open_fresh") / med("open_followed"), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18)
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--queries", type=int, nargs="+", default=[1 << 16, 1 << 10], help="cells drawn per shape")
    ap.add_argument("--opens", type=int, default=64, help="cells of the opening call after the update")
    ap.add_argument("--blocks", type=int, default=6, help="alternating blocks per side")
    ap.add_argument("--calls", type=int, default=5, help="timed calls per block and side")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    from cairo_m_amd.lib import MemImage
    be = Backend(0)
    rng = np.random.default_rng(1)
    p = (1 << 31) - 1
    n_lo = a.cells - a.heap
    cells_a = np.concatenate([np.arange(n_lo), (1 << 28) - a.heap + np.arange(a.heap)]).astype(np.uint32)   # ascending: the heap lies on top
    cells_v = rng.integers(0, p, (a.cells, 4)).astype(np.uint32)
    image = MemImage.from_cells(np.concatenate([cells_a.reshape(-1, 1), cells_v], axis=1), be.L)
    rep = {"cells": a.cells, "heap_cells": a.heap, "tree_nodes": image.stats()["n_nodes"], "image_bytes": image.stats()["bytes"],
           "shapes": [shape(a, be, image, cells_a, cells_v, q, 2 + i) for i, q in enumerate(a.queries)]}
    image.free()
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
