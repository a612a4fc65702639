#!/usr/bin/env python3
"""Measurement of the composed transitions (cm_compose_transitions) for a maintainer with a GPU, against what a follower of a run
does without them: one cm_verify_memory_transition per segment.

    python tools/compose_report.py --out profiles/<set>_compose_report.json

An image of --cells cells (locals and a heap, random values) and a chain of --parts images, each the one before with --part-cells
seeded random cells rewritten, in two overlap regimes: `same` (every part rewrites the same set) and `disjoint` (no two parts
share a cell).  Every tree comes from the host builder; tree i - 1 and tree i reach the device as the initial and final tree of
one uploaded input, whose transition cm_input_open_transition opens: the parts.  Before anything is timed the tool asserts that the
composed record, from the GPU path and from the host path, equals the two set openings of the union under the first and the last
tree word for word, and that the GPU verifier folds it to both roots.  One process, one GPU session, the sides timed in
alternating blocks.  Recorded per regime, wall ms of the C calls alone, as medians:
  compose_device      cm_compose_transitions(device = 1) + cm_mem_transition_get + cm_mem_transition_free
  compose_host        the same with device = 0
  verify_parts        k calls of cm_verify_memory_transition, one per part: what follow_run does
  verify_composed     one call of cm_verify_memory_transition on the composed record
and the bytes of the parts against the bytes of the composed record (36 n + 4 m each).  No threshold on the times."""
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


def regime(a, be, name, cells_a, cells_v, tree0, root0, seed):
    from cairo_m_amd.lib import ArrayInput, MemTransitionViewC, _transition_args, _transition_view, compose_transitions, verify_transition
    L = be.L
    rng = np.random.default_rng(seed)
    k, per = a.parts, a.part_cells
    if name == "same":
        picks = [np.sort(rng.choice(cells_a.size, per, replace=False))] * k
    else:
        perm = rng.permutation(cells_a.size)[:k * per]
        picks = [np.sort(perm[i * per:(i + 1) * per]) for i in range(k)]
    trees, values, parts = [(tree0, root0)], cells_v.copy(), []
    for j in picks:
        values[j] = rng.integers(1, (1 << 31) - 1, (j.size, 4)).astype(np.uint32)
        trees.append(host_tree(L, cells_a, values))
        dev = be.upload_input(ArrayInput({"initial_tree": trees[-2][0], "final_tree": trees[-1][0], "roots": [trees[-2][1], trees[-1][1]]}))
        parts.append(be.open_transition(dev, cells_a[j]))
        be.free_input(dev)
    # the composed record equals the two set openings of the union under the first and the last tree, word for word
    t = compose_transitions(parts, L, device=True)
    host = compose_transitions(parts, L, device=False)
    union = np.unique(np.concatenate([cells_a[j] for j in picks]))
    dev = be.upload_input(ArrayInput({"initial_tree": trees[0][0], "final_tree": trees[-1][0], "roots": [trees[0][1], trees[-1][1]]}))
    first, r_first = be.open_memory_set(dev, 0, union)
    last, r_last = be.open_memory_set(dev, 1, union)
    be.free_input(dev)
    assert (r_first, r_last) == (trees[0][1], trees[-1][1]) == (t.root_before, t.root_after)
    assert np.array_equal(t.addresses, union) and np.array_equal(t.siblings, first.siblings) and np.array_equal(t.siblings, last.siblings)
    assert np.array_equal(t.old_values, first.values) and np.array_equal(t.new_values, last.values)
    for f in ("addresses", "old_values", "new_values", "siblings"):
        assert getattr(t, f).tobytes() == getattr(host, f).tobytes(), f
    assert verify_transition(t, L, with_roots=True) == (True, (trees[0][1], trees[-1][1]))
    assert all(verify_transition(p, L) for p in parts)

    views, keep = (MemTransitionViewC * k)(), []
    for i, p in enumerate(parts):
        views[i], kept = _transition_view(p)
        keep.append(kept)
    out_view = MemTransitionViewC()
    out_view.struct_size = C.sizeof(MemTransitionViewC)

    def compose(device):
        h = C.c_void_p()
        t0 = time.perf_counter()
        rcs = [L.cm_compose_transitions(views, C.c_uint32(k), C.c_uint32(device), C.byref(h)), L.cm_mem_transition_get(h, C.byref(out_view)),
               L.cm_mem_transition_free(h)]
        dt = (time.perf_counter() - t0) * 1e3
        assert not any(rcs), rcs
        return dt

    ok, both = C.c_uint8(0), (C.c_uint32 * 2)()
    part_args = [_transition_args(p) for p in parts]
    one_args = _transition_args(t)

    def verify(arg_sets):
        t0 = time.perf_counter()
        for args, _ in arg_sets:
            rc = L.cm_verify_memory_transition(*args, C.byref(ok), both, C.c_uint64(0))
            assert rc == 0 and ok.value == 1
        return (time.perf_counter() - t0) * 1e3

    sides = {"compose_device": lambda: compose(1), "compose_host": lambda: compose(0), "verify_parts": lambda: verify(part_args),
             "verify_composed": lambda: verify([one_args])}
    for _ in range(2):                                                            # the pool and the code objects are warm
        for f in sides.values():
            f()
    ms = {key: [] for key in sides}
    for _ in range(a.blocks):
        for key, f in sides.items():
            for _ in range(a.calls):
                ms[key].append(f())
    ms = {key: stats(v) for key, v in ms.items()}
    med = lambda key: ms[key]["median"]
    bytes_parts, bytes_composed = sum(p.nbytes for p in parts), t.nbytes
    return {"regime": name, "parts": k, "cells_per_part": per, "cells_in_all": int(sum(p.addresses.size for p in parts)), "union_cells": int(union.size),
            "words_of_the_parts": int(sum(p.siblings.size for p in parts)), "words_composed": int(t.siblings.size), "blocks": a.blocks,
            "calls_per_block": a.calls, "ms": ms, "bytes": {"parts": bytes_parts, "composed": bytes_composed},
            "parts_over_composed": {"bytes": round(bytes_parts / bytes_composed, 2), "verify": round(med("verify_parts") / med("verify_composed"), 2),
                                    "verify_against_compose_plus_verify": round(med("verify_parts") / (med("compose_device") + med("verify_composed")), 2)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18)
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--parts", type=int, default=8)
    ap.add_argument("--part-cells", type=int, default=1 << 13, help="cells each part rewrites")
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
           "regimes": [regime(a, be, name, cells_a, cells_v, tree0, root0, 2 + i) for i, name in enumerate(("same", "disjoint"))]}
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
