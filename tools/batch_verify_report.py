#!/usr/bin/env python3
"""Measurement of the batched transition verifier (cm_verify_memory_transitions) for a maintainer with a GPU, against what a
follower of a run does without it: one cm_verify_memory_transition per segment.

    python tools/batch_verify_report.py --out profiles/batch_verify_report.json

A chain of images, each the one before with some seeded random cells rewritten; every tree comes from the host builder, tree i - 1
and tree i reach the device as the initial and final tree of one uploaded input, whose transition cm_input_open_transition opens:
the parts.  Shapes: 8 parts of 8 192 cells of a 2^18-cell image, once with every part rewriting the same set (`same`) and once
with no two parts sharing a cell (`disjoint`); 8 and 64 parts of 1 023 cells (disjoint, of a 2^17-cell image: the fold of a part
does not depend on the image's size, and 64 host trees of the larger image would only make the tool slow).  Before anything is
timed the tool asserts that the batch accepts every part with the roots the single calls compute.  One process, one GPU session.
Per shape, wall ms of the C calls alone, the median of --calls calls after --warm:
  loop        k calls of cm_verify_memory_transition: what follow_run does, the yardstick
  batch       one cm_verify_memory_transitions
  compose     cm_compose_transitions(device = 1) + get + free, followed by one cm_verify_memory_transition of the result
and, for the batch, the split host / upload+kernels+download from two more timings: `plan` = cm_mem_batch_plan over the same
addresses (the host checks and the plan the call runs before its upload) and `stream` = batch - plan, the copy up, the launches,
the copy down and the wait.  The plan's launches are recorded beside them.  No threshold on the times."""
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


def image(L, cells, heap, seed):
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.arange(cells - heap), (1 << 28) - heap + np.arange(heap)]).astype(np.uint32)   # ascending: the heap lies on top
    v = rng.integers(0, (1 << 31) - 1, (cells, 4)).astype(np.uint32)
    return a, v, host_tree(L, a, v)


def shape(a, be, name, k, per, regime, img, seed):
    from cairo_m_amd.lib import (ArrayInput, MemTransitionViewC, _transition_args, _transition_view, mem_batch_launches, mem_batch_plan, verify_transition,
                                 verify_transitions)
    L = be.L
    cells_a, cells_v, tree0 = img
    rng = np.random.default_rng(seed)
    if regime == "same":
        picks = [np.sort(rng.choice(cells_a.size, per, replace=False))] * k
    else:
        perm = rng.permutation(cells_a.size)[:k * per]
        picks = [np.sort(perm[i * per:(i + 1) * per]) for i in range(k)]
    trees, values, parts = [tree0], cells_v.copy(), []
    for j in picks:
        values[j] = rng.integers(1, (1 << 31) - 1, (j.size, 4)).astype(np.uint32)
        trees.append(host_tree(L, cells_a, values))
        dev = be.upload_input(ArrayInput({"initial_tree": trees[-2][0], "final_tree": trees[-1][0], "roots": [trees[-2][1], trees[-1][1]]}))
        parts.append(be.open_transition(dev, cells_a[j]))
        be.free_input(dev)
    # the batch gives, part for part, what the single calls give
    single = [verify_transition(p, L, with_roots=True) for p in parts]
    assert single == [(True, (trees[i][1], trees[i + 1][1])) for i in range(k)]
    assert verify_transitions(parts, L, with_roots=True) == single

    views, keep = (MemTransitionViewC * k)(), []
    for i, p in enumerate(parts):
        views[i], kept = _transition_view(p)
        keep.append(kept)
    part_args = [_transition_args(p) for p in parts]
    ok, both = C.c_uint8(0), (C.c_uint32 * 2)()
    oks, roots = (C.c_uint8 * k)(), (C.c_uint32 * (2 * k))()
    out_view = MemTransitionViewC()
    out_view.struct_size = C.sizeof(MemTransitionViewC)
    ptrs = (C.POINTER(C.c_uint32) * k)(*[v.addresses for v in views])
    counts = np.array([p.addresses.size for p in parts], dtype=np.uint32)
    steps, n_steps = (C.c_uint32 * (4 * 29))(), C.c_uint32(0)

    def loop():
        t0 = time.perf_counter()
        for args, _ in part_args:
            rc = L.cm_verify_memory_transition(*args, C.byref(ok), both, C.c_uint64(0))
            assert rc == 0 and ok.value == 1
        return (time.perf_counter() - t0) * 1e3

    def batch():
        t0 = time.perf_counter()
        rc = L.cm_verify_memory_transitions(views, C.c_uint32(k), oks, roots, C.c_uint64(0))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and all(oks)
        return dt

    def compose():
        h = C.c_void_p()
        t0 = time.perf_counter()
        rcs = [L.cm_compose_transitions(views, C.c_uint32(k), C.c_uint32(1), C.byref(h)), L.cm_mem_transition_get(h, C.byref(out_view))]
        rcs.append(L.cm_verify_memory_transition(C.c_uint32(out_view.root_before), C.c_uint32(out_view.root_after), out_view.addresses, C.c_uint64(out_view.n),
                                                 out_view.old_values, out_view.new_values, out_view.siblings, C.c_uint32(out_view.n_siblings), C.byref(ok),
                                                 both, C.c_uint64(0)))
        rcs.append(L.cm_mem_transition_free(h))
        dt = (time.perf_counter() - t0) * 1e3
        assert not any(rcs) and ok.value == 1, rcs
        return dt

    def plan():
        t0 = time.perf_counter()
        rc = L.cm_mem_batch_plan(ptrs, counts.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(k), steps, C.c_uint32(29), C.byref(n_steps))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0
        return dt

    sides = {"loop": loop, "batch": batch, "compose": compose, "plan": plan}
    if a.batch_only is not None:                                                  # for a kernel trace: nothing but the batch's launches repeats
        sides = {"batch": batch, "plan": plan}
    ms = {}
    for key, f in sides.items():
        for _ in range(a.warm):
            f()
        ms[key] = stats([f() for _ in range(a.calls)])
    med = lambda key: ms[key]["median"]
    the_plan = mem_batch_plan([p.addresses for p in parts], L)
    return {"shape": name, "regime": regime, "parts": k, "cells_per_part": per, "image_cells": int(cells_a.size),
            "words_of_the_parts": int(sum(p.siblings.size for p in parts)), "warm": a.warm, "calls": a.calls, "ms": ms,
            "batch_split_ms": {"host_checks_and_plan": med("plan"), "upload_kernels_download_and_wait": round(med("batch") - med("plan"), 4)},
            "launches": {"batch_hashing": mem_batch_launches(the_plan), "batch_in_all": mem_batch_launches(the_plan) + 3,
                         "per_level_steps": sum(1 for s in the_plan if s["kernel"] == "level")},
            **({} if a.batch_only is not None else {"loop_over_batch": round(med("loop") / med("batch"), 2),
                                                    "loop_over_compose": round(med("loop") / med("compose"), 2)})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18, help="cells of the image of the 8 192-cell shapes")
    ap.add_argument("--small-cells", type=int, default=1 << 17, help="cells of the image of the 1 023-cell shapes")
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of either image that lie in the heap")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch-only", type=int, help="time only the batch of shape 0 .. 3: what a kernel trace of the call is taken from")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    be = Backend(0)
    shapes = [("8 x 8192", 8, 1 << 13, "same", a.cells, 3), ("8 x 8192", 8, 1 << 13, "disjoint", a.cells, 4), ("8 x 1023", 8, 1023, "disjoint", a.small_cells, 5),
              ("64 x 1023", 64, 1023, "disjoint", a.small_cells, 6)]
    if a.batch_only is not None:
        shapes = [shapes[a.batch_only]]
    images = {c: image(be.L, c, a.heap, c % 7) for c in {s[4] for s in shapes}}
    rep = {"shapes": [shape(a, be, name, k, per, regime, images[c], seed) for name, k, per, regime, c, seed in shapes]}
    text = json.dumps(rep, indent=1)
    print(text)
    if a.out:
        open(a.out, "w").write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
