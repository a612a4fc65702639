#!/usr/bin/env python3
"""Measurement of the batched image update (cm_mem_images_apply) for a maintainer with a GPU, against what a follower of many
runs does without it: one cm_mem_image_apply per image, which is unchanged code and the yardstick.

    python tools/image_batch_report.py --out profiles/image_batch_report.json

Images of 2^18 cells (locals dense from 0, a heap on top), all of the same seeded contents.  Shapes: 8 parts of 1 023 cells, 64
parts of 1 023 cells, 8 parts of 8 192 cells; every part rewrites its own seeded random pick of held cells with fresh words.
Before anything is timed the tool asserts that the batch gives, part for part, the roots of the single calls and the same node
lists.  One process, one GPU session.  Per shape the two legs run in alternating blocks, loop then batch, --repeats times; a block
is --warm untimed and --calls timed calls, and EVERY call of either leg gets freshly created images (the update changes them),
made and freed outside the timed window.  A timed call is the wall time of the C calls alone, which end in the stream's wait:
  loop        k calls of cm_mem_image_apply
  batch       one cm_mem_images_apply
The file holds every block's median and, per leg, the spread of those medians; `batch_ahead_beyond_spread` is true only when the
slowest batch block is faster than the fastest loop block.  The launches cm_mem_batch_plan lists for the parts are recorded
beside them.  No threshold on the times."""
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


def contents(cells, heap, seed):
    rng = np.random.default_rng(seed)
    a = np.concatenate([np.arange(cells - heap), (1 << 28) - heap + np.arange(heap)]).astype(np.uint32)   # ascending: the heap lies on top
    v = rng.integers(0, (1 << 31) - 1, (cells, 4)).astype(np.uint32)
    return a, v


def shape(a, L, name, k, per, img, seed):
    from cairo_m_amd.lib import MemImage, MemImageResultC, MemImageUpdateC, mem_batch_launches, mem_batch_plan
    cells_a, cells_v = img
    started = time.perf_counter()
    rng = np.random.default_rng(seed)
    perm = rng.permutation(cells_a.size)
    picks = [np.sort(perm[i * per:(i + 1) * per]) for i in range(k)]                 # no two parts share a cell
    addrs = [np.ascontiguousarray(cells_a[j]) for j in picks]
    news = [np.ascontiguousarray(rng.integers(1, (1 << 31) - 1, (per, 4)).astype(np.uint32)) for _ in range(k)]
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))

    def fresh():
        ims = []
        for _ in range(k):
            h = C.c_void_p()
            rc = L.cm_mem_image_create(p(cells_a), p(cells_v), C.c_uint64(cells_a.size), C.c_uint32(1), C.byref(h))
            assert rc == 0, rc
            ims.append(MemImage(L, h, True))
        return ims

    def free(ims):
        for im in ims:
            im.free()

    parts, res, root = (MemImageUpdateC * k)(), (MemImageResultC * k)(), C.c_uint32(0)
    for i in range(k):
        parts[i].struct_size, parts[i].n = C.sizeof(MemImageUpdateC), per
        parts[i].addresses, parts[i].new_values = p(addrs[i]), p(news[i])

    def loop(ims):
        t0 = time.perf_counter()
        for i, im in enumerate(ims):
            rc = L.cm_mem_image_apply(im.h, p(addrs[i]), p(news[i]), C.c_uint64(per), None, None, None, C.byref(root), None)
            assert rc == 0, rc
        return (time.perf_counter() - t0) * 1e3

    def batch(ims):
        for i, im in enumerate(ims):
            parts[i].img = im.h
        t0 = time.perf_counter()
        rc = L.cm_mem_images_apply(parts, C.c_uint32(k), res)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt

    # the batch gives, part for part, what the single calls give
    x, y = fresh(), fresh()
    loop(x)
    batch(y)
    assert [im.root for im in x] == [r.root for r in res] == [im.root for im in y]
    assert all(u.nodes().tobytes() == w.nodes().tobytes() for u, w in zip(x[:2], y[:2]))
    free(x + y)

    def block(leg):
        out = []
        for i in range(a.warm + a.calls):
            ims = fresh()
            dt = leg(ims)
            free(ims)
            if i >= a.warm:
                out.append(dt)
        return stats(out)

    blocks = {"loop": [], "batch": []}
    for _ in range(a.repeats):
        blocks["loop"].append(block(loop))
        blocks["batch"].append(block(batch))
    med = {key: [b["median"] for b in v] for key, v in blocks.items()}
    the_plan = mem_batch_plan(addrs, L)
    return {"shape": name, "parts": k, "cells_per_part": per, "image_cells": int(cells_a.size), "warm": a.warm, "calls": a.calls, "repeats": a.repeats,
            "blocks_ms": blocks,
            "medians_ms": {key: {"of_the_blocks": v, "median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4)} for key, v in med.items()},
            "loop_over_batch": round(statistics.median(med["loop"]) / statistics.median(med["batch"]), 2),
            "batch_ahead_beyond_spread": max(med["batch"]) < min(med["loop"]),
            "launches": {"batch_hashing": mem_batch_launches(the_plan), "per_level_steps": sum(1 for s in the_plan if s["kernel"] == "level")},
            "seconds_in_all": round(time.perf_counter() - started, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18, help="cells of every image")
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", type=int, help="shape 0 .. 2 alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    be = Backend(0)
    shapes = [("8 x 1023", 8, 1023, 5), ("64 x 1023", 64, 1023, 6), ("8 x 8192", 8, 1 << 13, 4)]
    if a.only is not None:
        shapes = [shapes[a.only]]
    img = contents(a.cells, a.heap, 3)
    rep = {"shapes": []}
    for name, k, per, seed in shapes:
        rep["shapes"].append(shape(a, be.L, name, k, per, img, seed))
        text = json.dumps(rep, indent=1)
        if a.out:                                                                 # (written shape by shape: a long run leaves what it has)
            open(a.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
