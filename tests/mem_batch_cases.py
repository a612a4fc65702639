"""The batches the CPU and the GPU tests of the batched verifiers share (tests/test_mem_batch_cpu.py, tests/test_gpu_mem_batch.py),
and the plan of a batch derived in Python from tests/mem_set_ref.levels — never the code under test.

BATCHES name lists of indices into mem_set_ref.SETS; the parts of a batch are the reference transitions (or sets) of those
entries.  SMALL is 300 parts of one or two cells, each under the root of a small memory of its own."""
import functools

import numpy as np

from tests.mem_set_ref import P, SETS, SPACE, TAIL, N_DEPTHS, RefTree, levels, ref_set

BLOCK = 256                                                                      # lanes of a block of the per-level kernel

BATCHES = {
    "all": list(range(len(SETS))),                                               # the widest parts enter the tail at 79 nodes
    "reversed": list(range(len(SETS)))[::-1],
    "widest in the middle": [0, 1, 9, 2, 3, 10, 8, 4, 5, 11, 6, 7],
    "range first": [10, 0, 1, 3, 4, 5],                                          # range(1000, 1257) enters the tail at 65
    "three runs last": [2, 6, 7, 11],                                            # the three-run set enters at 72
}


def well_formed(a):
    a = [int(x) for x in a]
    return bool(a) and all(x < SPACE for x in a) and all(y > x for x, y in zip(a, a[1:]))


def ref_batch_plan(address_lists):
    """[(depth, n_nodes of all parts, widest part, kernel)]: [] when no part has cells and good addresses, else 29 steps — the
    per-level kernel while ANY part's S_k is wider than TAIL"""
    lv = [levels(a) for a in address_lists if well_formed(a)]
    if not lv:
        return []
    steps = [(28, sum(len(l[0]) for l in lv), max(len(l[0]) for l in lv), "cells")]
    for k in range(N_DEPTHS):
        kind = "level" if max(len(l[k]) for l in lv) > TAIL else "tail"
        steps.append((27 - k, sum(len(l[k + 1]) for l in lv), max(len(l[k + 1]) for l in lv), kind))
    return steps


def tail_entry(address_lists):
    """(k_tail, [|S_k_tail| of every part]): the shift at which the batch enters the tail and every part's width there"""
    lv = [levels(a) for a in address_lists]
    k = next(k for k in range(N_DEPTHS + 1) if max(len(l[k]) for l in lv) <= TAIL)
    return k, [len(l[k]) for l in lv]


@functools.lru_cache(maxsize=None)
def small_parts():
    """300 dicts as mem_transition_ref.reference gives them (a, old, new, words, root0, root1), of one or two cells each: [0],
    [0, 2^28 - 1] and the straddle pair first, then seeded random singles and pairs; every part has a memory of its own (its cells,
    some of them absent, and three bystanders) and a second memory that differs in exactly its cells"""
    rng = np.random.default_rng(300)
    sets = [[0], [0, SPACE - 1], [(1 << 27) - 1, 1 << 27]]
    while len(sets) < 300:
        a = sorted({int(x) for x in rng.integers(0, SPACE, 1 + len(sets) % 2)})
        if len(a) == 1 + len(sets) % 2:                                          # (two draws that coincide are drawn again)
            sets.append(a)
    out = []
    for j, a in enumerate(sets):
        word = lambda: tuple(int(x) for x in rng.integers(1, P - 1, 4))
        cells = {int(x): word() for x in rng.integers(0, SPACE, 3)}
        for x in a[j % 3 == 0:]:                                                 # (every third part's first cell is absent before)
            cells[x] = word()
        after = dict(cells)
        for x in a:
            after[x] = word()
        t0, t1 = RefTree([(x,) + v for x, v in cells.items()]), RefTree([(x,) + v for x, v in after.items()])
        words, old, _ = ref_set(t0, a)
        words_after, new, _ = ref_set(t1, a)
        assert words == words_after
        out.append({"a": list(a), "old": old, "new": new, "words": words, "root0": t0.root, "root1": t1.root})
    return out


__all__ = ["BATCHES", "BLOCK", "ref_batch_plan", "small_parts", "tail_entry", "well_formed"]
