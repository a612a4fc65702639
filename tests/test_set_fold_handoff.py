"""The handoff from the per-level kernel to the one-workgroup tail of the set fold (csrc/set_fold.hpp), which the set verifier,
the transition verifier and the image update share: sets whose widths sit on the threshold, where an off-by-one in the shared
driver or in the tail's bounds would show.

    128 contiguous cells      S_0 = 128 = the tail's width: straight into the tail with every lane live
    128 unpaired odd cells    the tail at full width, every parent of the first step taking a LEFT sibling word
    129 contiguous cells      exactly one per-level launch, 129 -> 65, then the tail
    the last 129 cells        the same at the top of the address space
    a single cell             the tail at width 1

The plan is asserted on the CPU against these very shapes.  On the GPU every consumer runs every set over one of the memories of
tests/mem_open_ref.py and is held to the independent paths: RefTree (the pinned host tree builder's records), the pure-Python
fold of tests/mem_set_ref.py, the *_host verifiers and the host image."""
import functools

import numpy as np
import pytest

from cairo_m_amd.lib import (MemImage, MemSetOpening, MemTransition, mem_set_plan, verify_set, verify_set_host, verify_transition,
                             verify_transition_host)
from tests.mem_image_ref import assert_image_is, assert_refused, snapshot
from tests.mem_open_ref import P, SPACE, RefTree, memories
from tests.mem_set_ref import TAIL, fold, levels, ref_plan, ref_set

# (memory, addresses, per-level launches, the width at which the tail is entered)
SETS = [
    ("c", list(range(128)), 0, 128),
    ("c", list(range(1, 256, 2)), 0, 128),
    ("c", list(range(129)), 1, 65),
    ("b", list(range(SPACE - 129, SPACE)), 1, 65),
    ("c", [7], 0, 1),
]
IDS = ["128-contiguous", "128-odd", "129-contiguous", "129-at-the-top", "single"]
CASES = range(len(SETS))


def test_the_plans_are_the_handoffs_named_above():
    assert TAIL == 128
    for (_, a, n_level, entry), name in zip(SETS, IDS):
        steps, n_words = mem_set_plan(a)
        want, want_words = ref_plan(a)
        assert [(s["depth"], s["n_nodes"], s["n_siblings"], s["kernel"]) for s in steps] == want and n_words == want_words, name
        assert [s["kernel"] for s in steps] == ["cells"] + ["level"] * n_level + ["tail"] * (28 - n_level), name
        assert len(levels(a)[n_level]) == entry and steps[n_level]["n_nodes"] == entry, name
    odd = mem_set_plan(SETS[1][1])[0]
    assert odd[1]["n_nodes"] == 128 and odd[1]["n_siblings"] == 128                # every lane of the tail's first step reads a word
    assert ref_set(RefTree(memories()["c"]), SETS[1][1])[2][0] == 128
    assert all(x & 1 for x in SETS[1][1])                                          # ... and puts it on the left


@functools.lru_cache(maxsize=None)
def reference(i):
    """the transition of SETS[i] from its memory to the same memory with every cell of the set rewritten, from RefTree alone"""
    name, a, _, _ = SETS[i]
    tree0 = RefTree(memories()[name])
    words, old, _ = ref_set(tree0, a)
    new = np.array([[(3 * x + 5 * j + 1) % P for j in range(4)] for x in a], dtype=np.uint32)
    after = {c[0]: c[1:] for c in tree0.cells}
    after.update({x: tuple(int(w) for w in v) for x, v in zip(a, new)})
    tree1 = RefTree([(x,) + v for x, v in after.items()])
    assert fold(a, old, words) == tree0.root and fold(a, new, words) == tree1.root and tree0.root != tree1.root
    return {"a": a, "words": words, "old": old, "new": new, "tree0": tree0, "tree1": tree1}


def _bump(x, *at):
    """a copy of the array with one word raised by one (mod P)"""
    y = np.array(x, dtype=np.uint32)
    y[at] = (int(y[at]) + 1) % P
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_verify_set_at_the_handoff(backend, i):
    r = reference(i)
    root = r["tree0"].root
    good = MemSetOpening(r["a"], r["old"], r["words"])
    assert verify_set(root, good, backend.L, with_root=True) == (True, root)
    assert verify_set_host(root, good, backend.L) == (0, "")
    n, m = len(r["a"]), len(r["words"])
    for bad in (MemSetOpening(r["a"], r["old"], _bump(r["words"], m // 2)), MemSetOpening(r["a"], _bump(r["old"], n // 2, 1), r["words"])):
        ok, got = verify_set(root, bad, backend.L, with_root=True)
        rc, msg = verify_set_host(root, bad, backend.L)
        assert ok is False and got not in (0, root) and rc == 11 and "hashes to root" in msg, (ok, got, rc, msg)


@pytest.mark.gpu
@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_verify_transition_at_the_handoff(backend, i):
    r = reference(i)
    roots = (r["tree0"].root, r["tree1"].root)
    make = lambda old, new, words: MemTransition(r["a"], old, new, words, *roots)
    good = make(r["old"], r["new"], r["words"])
    assert verify_transition(good, backend.L, with_roots=True) == (True, roots)
    assert verify_transition_host(good, backend.L) == (0, "")
    n, m = len(r["a"]), len(r["words"])
    word = make(r["old"], r["new"], _bump(r["words"], m // 2))                     # one word serves both folds: both roots move
    value = make(r["old"], _bump(r["new"], n // 2, 1), r["words"])                 # a new value: the root after alone
    for bad, same in ((word, ()), (value, (0,))):
        ok, got = verify_transition(bad, backend.L, with_roots=True)
        rc, msg = verify_transition_host(bad, backend.L)
        assert ok is False and rc == 11 and "hash to root" in msg, (ok, got, rc, msg)
        assert all((got[j] == roots[j]) == (j in same) and got[j] != 0 for j in (0, 1)), (got, roots)


@pytest.mark.gpu
@pytest.mark.parametrize("i", CASES, ids=IDS)
def test_image_update_at_the_handoff(backend, i):
    r = reference(i)
    tree0, tree1 = r["tree0"], r["tree1"]
    dev, host = (MemImage.from_cells(tree0.cells, backend.L, device=d) for d in (True, False))
    try:
        assert_image_is(dev, tree0)
        off = _bump(r["old"], len(r["a"]) // 2, 1)                                # a tampered old value: refused alike, nothing changes
        for image in (dev, host):
            assert_refused(image, lambda im: im.apply(r["a"], r["new"], old_values=off), 11, f"cell {r['a'][len(r['a']) // 2]} holds")
        apply = lambda im: im.apply(r["a"], r["new"], old_values=r["old"], root_before=tree0.root, root_after=tree1.root)
        assert apply(dev) == tree1.root == apply(host)
        assert_image_is(dev, tree1)
        assert snapshot(dev) == snapshot(host)
    finally:
        dev.free()
        host.free()
