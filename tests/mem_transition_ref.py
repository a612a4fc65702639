"""Reference for memory transitions, independent of the code under test and built on tests/mem_set_ref.py: for every entry of
SETS a second memory that differs from the first in exactly that set's cells, both trees from the pinned host builder (RefTree),
and the reference transition = ref_set of the set under both.  Nothing here folds with the library's set code: the roots are the
trees' own and the words are read off their node records.

How the second memory is made, per set: every cell of the set gets four fresh words from a seeded generator (never the old
value); the first cell of the set that the first memory holds with a value other than zero is written to (0, 0, 0, 0) and stays
in the memory as an explicit zero cell; a cell the first memory lacks is thereby created; and the last cell of the set, unless it
is the zeroed one, gets P - 1 as its word 3."""
import functools

import numpy as np

from tests.mem_set_ref import P, SETS, RefTree, range_memories, ref_plan, ref_set

ZERO = (0, 0, 0, 0)


@functools.lru_cache(maxsize=None)
def first_tree(name):
    return RefTree(range_memories()[name])


@functools.lru_cache(maxsize=None)
def second_memory(i):
    """(cells of the second memory, the address written to zero or None, the addresses created, the address holding P - 1 or None)"""
    name, a = SETS[i]
    cells = {c[0]: tuple(c[1:]) for c in range_memories()[name]}
    rng = np.random.default_rng(1000 + i)
    zeroed = next((x for x in a if cells.get(x, ZERO) != ZERO), None)
    created = [x for x in a if x not in cells]
    top = a[-1] if a[-1] != zeroed else None
    for x in a:
        old = cells.get(x, ZERO)
        new = tuple(int(w) for w in rng.integers(1, P - 1, 4))
        if x == zeroed:
            new = ZERO
        elif x == top:
            new = new[:3] + (P - 1,)
        assert new != old
        cells[x] = new
    return [(x,) + v for x, v in sorted(cells.items())], zeroed, created, top


@functools.lru_cache(maxsize=None)
def second_tree(i):
    return RefTree(second_memory(i)[0])


@functools.lru_cache(maxsize=None)
def reference(i):
    """dict: a, old, new ((n, 4) arrays), words, counts, root0, root1, words_after (the words under the second tree)"""
    name, a = SETS[i]
    t0, t1 = first_tree(name), second_tree(i)
    words, old, counts = ref_set(t0, a)
    words_after, new, counts_after = ref_set(t1, a)
    assert counts == counts_after
    return {"a": list(a), "old": old, "new": new, "words": words, "words_after": words_after, "counts": counts, "root0": t0.root, "root1": t1.root}


def tampers(r):
    """name -> (a, old, new, words, root0, root1, what the host verifier's message must contain, which side still folds to its
    root: 'old', 'new', 'both' or None when the record is malformed): each is ONE change to a valid transition"""
    a, old, new, w = list(r["a"]), r["old"], r["new"], list(r["words"])
    n, m, r0, r1 = len(a), len(w), r["root0"], r["root1"]
    out = {}

    def bump(x, cell, i):
        y = x.copy()
        y[cell, i] = (int(y[cell, i]) + 1) % P
        return y

    def put(x, cell, i, v):
        y = x.copy()
        y[cell, i] = v
        return y

    out["an old word + 1"] = (a, bump(old, n // 2, 1), new, w, r0, r1, "the old values hash to root", "new")
    out["a new word + 1"] = (a, old, bump(new, n - 1, 2), w, r0, r1, "the new values hash to root", "old")
    x = list(w)
    x[m // 2] = (x[m // 2] + 1) % P
    out["a sibling + 1"] = (a, old, new, x, r0, r1, "the old values hash to root", None)   # both sides fail, the old one is named
    if r0 != r1:
        out["roots swapped"] = (a, old, new, w, r1, r0, f"the old values hash to root {r0}, not {r1}", "both")
    out["root after + 1"] = (a, old, new, w, r0, (r1 + 1) % P, f"the new values hash to root {r1}, not {(r1 + 1) % P}", "both")
    out["an old word = P"] = (a, put(old, 0, 3, P), new, w, r0, r1, f"old value word 3 of cell {a[0]} is not below P", None)
    out["a new word = P"] = (a, old, put(new, n - 1, 0, P), w, r0, r1, f"new value word 0 of cell {a[-1]} is not below P", None)
    q = m // 3
    depth, seen = None, 0
    for k, (_, _, c, _) in enumerate(ref_plan(a)[0][1:]):
        if q < seen + c:
            depth = 28 - k
            break
        seen += c
    x = list(w)
    x[q] = P
    out["a sibling = P"] = (a, old, new, x, r0, r1, f"sibling {q} (depth {depth}) is not below P", None)
    out["one word appended"] = (a, old, new, w + [1], r0, r1, f"{m + 1} sibling words where the addresses need {m}", None)
    out["one word dropped"] = (a, old, new, w[:-1], r0, r1, f"{m - 1} sibling words where the addresses need {m}", None)
    if n > 1:
        x = list(a)
        x[0], x[1] = x[1], x[0]
        out["two addresses swapped"] = (x, old, new, w, r0, r1, "address 1 is not above address 0", None)
    return out


__all__ = ["P", "SETS", "ZERO", "first_tree", "second_memory", "second_tree", "reference", "tampers"]
