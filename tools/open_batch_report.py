#!/usr/bin/env python3
"""Measurement of the batched set opening (cm_mem_images_open_memory_sets) for a maintainer with a GPU, against what a follower
that serves clients does without it: one cm_mem_image_open_memory_set per request, which is unchanged code and the yardstick.

    python tools/open_batch_report.py --out profiles/open_batch_report.json

Images of 2^18 cells (locals dense from 0, a heap on top), all of the same seeded contents.  Shapes: 64 parts of 64 random cells
under ONE image; 8 parts of 1 023 cells under 8 images; 8 parts of 8 192 cells under 8 images; 1 part of 64 cells, the batch's own
overhead against the single call.  Before anything is timed the tool asserts that the batch gives, part for part, the bytes of
the single calls, and that verify_sets accepts every record.  One process, one GPU session.  Per shape the two legs run in
alternating blocks, loop then batch, --repeats times; a block is --warm untimed and --calls timed calls.  Openings change
nothing, so the images are made once per shape.  A timed call is the wall time of the C calls alone, which end in the stream's
wait:
  loop        k calls of cm_mem_image_open_memory_set
  batch       one cm_mem_images_open_memory_sets
The file holds every block's median and, per leg, the spread of those medians; `batch_ahead_beyond_spread` is true only when the
slowest batch block is faster than the fastest loop block.  The in-library kernel profile of ONE batched call (cm_kprof_report:
the classes that are registered, k_sets_gather among them) is recorded beside them.  No threshold on the times."""
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


def shape(a, L, name, k, per, n_images, img, seed):
    from cairo_m_amd.lib import MemImage, MemSetOpening, MemSetRequestC, MemSetResultC, mem_set_plan, verify_sets
    cells_a, cells_v = img
    started = time.perf_counter()
    rng = np.random.default_rng(seed)
    addrs = [np.ascontiguousarray(np.sort(rng.choice(cells_a, per, replace=False))) for _ in range(k)]
    need = [mem_set_plan(x, L)[1] for x in addrs]
    p = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    ims = []
    for _ in range(n_images):
        h = C.c_void_p()
        rc = L.cm_mem_image_create(p(cells_a), p(cells_v), C.c_uint64(cells_a.size), C.c_uint32(1), C.byref(h))
        assert rc == 0, rc
        ims.append(MemImage(L, h, True))
    of = lambda i: ims[i % n_images]
    arrays = lambda: ([np.zeros(4 * per, dtype=np.uint32) for _ in range(k)], [np.zeros(m, dtype=np.uint32) for m in need])
    lv, lw = arrays()
    bv, bw = arrays()
    parts, res, n_sib, root = (MemSetRequestC * k)(), (MemSetResultC * k)(), C.c_uint32(0), C.c_uint32(0)
    for i in range(k):
        parts[i].struct_size, parts[i].n, parts[i].img, parts[i].cap_siblings = C.sizeof(MemSetRequestC), per, of(i).h, need[i]
        parts[i].addresses, parts[i].values, parts[i].siblings = p(addrs[i]), p(bv[i]), p(bw[i])

    def loop():
        t0 = time.perf_counter()
        for i in range(k):
            rc = L.cm_mem_image_open_memory_set(of(i).h, p(addrs[i]), C.c_uint64(per), p(lv[i]), p(lw[i]), C.c_uint32(need[i]), C.byref(n_sib), C.byref(root))
            assert rc == 0, rc
        return (time.perf_counter() - t0) * 1e3

    def batch():
        t0 = time.perf_counter()
        rc = L.cm_mem_images_open_memory_sets(parts, C.c_uint32(k), res)
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0, rc
        return dt

    # the batch gives, part for part, what the single calls give, and the records verify
    loop()
    batch()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(lv + lw, bv + bw))
    assert [r.n_siblings for r in res] == need and all(r.root == of(i).root for i, r in enumerate(res))
    assert all(verify_sets([r.root for r in res], [MemSetOpening(addrs[i], bv[i], bw[i]) for i in range(k)], L))

    def block(leg):
        out = [leg() for _ in range(a.warm + a.calls)]
        return stats(out[a.warm:])

    blocks = {"loop": [], "batch": []}
    for _ in range(a.repeats):
        blocks["loop"].append(block(loop))
        blocks["batch"].append(block(batch))
    med = {key: [b["median"] for b in v] for key, v in blocks.items()}
    # the kernel profile of one batched call
    L.cm_kprof_enable(C.c_int32(1))
    batch()
    buf = C.create_string_buffer(1 << 16)
    L.cm_kprof_report(buf, C.c_size_t(1 << 16))
    L.cm_kprof_enable(C.c_int32(0))
    for im in ims:
        im.free()
    return {"shape": name, "parts": k, "cells_per_part": per, "images": n_images, "image_cells": int(cells_a.size), "sibling_words": int(sum(need)),
            "warm": a.warm, "calls": a.calls, "repeats": a.repeats, "blocks_ms": blocks,
            "medians_ms": {key: {"of_the_blocks": v, "median": round(statistics.median(v), 4), "spread": round(max(v) - min(v), 4)} for key, v in med.items()},
            "loop_over_batch": round(statistics.median(med["loop"]) / statistics.median(med["batch"]), 2),
            "batch_ahead_beyond_spread": max(med["batch"]) < min(med["loop"]),
            "kprof_of_one_batched_call": json.loads(buf.value.decode()),
            "seconds_in_all": round(time.perf_counter() - started, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=1 << 18, help="cells of every image")
    ap.add_argument("--heap", type=int, default=1 << 12, help="cells of the image that lie in the heap")
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", type=int, help="shape 0 .. 3 alone")
    ap.add_argument("--out")
    a = ap.parse_args()
    from cairo_m_amd import Backend
    be = Backend(0)
    shapes = [("64 x 64, one image", 64, 64, 1, 5), ("8 x 1023", 8, 1023, 8, 6), ("8 x 8192", 8, 1 << 13, 8, 4), ("1 x 64", 1, 64, 1, 7)]
    if a.only is not None:
        shapes = [shapes[a.only]]
    img = contents(a.cells, a.heap, 3)
    rep = {"shapes": []}
    for name, k, per, n_images, seed in shapes:
        rep["shapes"].append(shape(a, be.L, name, k, per, n_images, img, seed))
        text = json.dumps(rep, indent=1)
        if a.out:                                                                 # (written shape by shape: a long run leaves what it has)
            open(a.out, "w").write(text + "\n")
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
