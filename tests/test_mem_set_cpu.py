"""Host side of the set openings against tests/mem_set_ref.py: cm_verify_memory_set_host and cm_memory_set_root_host accept the
reference's records and name what is wrong with a tampered one, cm_mem_set_plan equals the plan derived with Python sets, the
plan shows which kernels and which kinds of parent the shared sets reach, and the bytes / hashes arithmetic holds.  CPU only."""
import functools

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, MemSetOpening, mem_set_plan, set_root, verify_set_host
from tests.mem_set_ref import (CONTIGUOUS, MIXED, N_DEPTHS, P, SET_IDS, SETS, SPACE, TAIL, RefTree, check_set, fold, hashes, levels, parent_kinds,
                               range_memories, ref_plan, ref_set, tampers)
from tests.mem_range_ref import ref_range


@functools.lru_cache(maxsize=None)
def tree(name):
    return RefTree(range_memories()[name])


@functools.lru_cache(maxsize=None)
def reference(i):
    name, a = SETS[i]
    words, values, counts = ref_set(tree(name), a)
    return tree(name).root, a, values, words, counts


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_host_verifier_accepts_the_reference_and_agrees_with_the_python_fold(i):
    root, a, values, words, counts = reference(i)
    assert len(words) == sum(counts)
    assert check_set(root, a, values, words)
    o = MemSetOpening(a, values, words)
    assert verify_set_host(root, o) == (0, "")
    assert set_root(o) == root == fold(a, values, words)


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_every_tamper_is_rejected_with_the_named_message(i):
    root, a, values, words, _ = reference(i)
    cases = tampers(a, values, words, root)
    assert len(cases) == (14 if len(a) > 1 else 12)
    for what, (ta, tv, tw, tr, needle) in cases.items():
        assert not check_set(tr, ta, tv, tw), what
        rc, msg = verify_set_host(tr, MemSetOpening(ta, tv, tw))
        assert rc == 11 and msg.startswith(f"memory set of {len(ta)} cells: ") and needle in msg, (what, rc, msg)


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_plan_equals_the_reference_plan(i):
    _, a, _, _, counts = reference(i)
    steps, m = mem_set_plan(a)
    want, want_m = ref_plan(a)
    assert m == want_m == sum(counts) and len(steps) == 29
    assert [(s["depth"], s["n_nodes"], s["n_siblings"], s["kernel"]) for s in steps] == want
    assert [s["n_siblings"] for s in steps[1:]] == counts


def test_the_sets_reach_every_kernel_and_every_kind_of_parent_in_level_and_tail():
    seen = {"level": set(), "tail": set()}
    kernels, tail_entries = set(), []
    for _, a in SETS:
        steps, _ = mem_set_plan(a)
        lv = levels(a)
        kernels |= {s["kernel"] for s in steps}
        assert steps[0]["kernel"] == "cells" and steps[-1]["kernel"] == "tail" and steps[-1]["n_nodes"] == 1
        kinds = [s["kernel"] for s in steps[1:]]
        first_tail = kinds.index("tail")
        assert kinds == ["level"] * first_tail + ["tail"] * (N_DEPTHS - first_tail)   # one run of levels, then the tail
        assert all(len(lv[k]) > TAIL for k in range(first_tail)) and len(lv[first_tail]) <= TAIL
        tail_entries.append(len(lv[first_tail]))
        for k in range(N_DEPTHS):
            seen[kinds[k]] |= parent_kinds(a, k)
    assert kernels == {"cells", "level", "tail"}
    assert seen["level"] == seen["tail"] == {"both", "left", "right"}
    assert max(tail_entries) > TAIL // 2 and min(tail_entries) == 1              # the tail entered above half its width, and at one node
    assert sum(1 for _, a in SETS if mem_set_plan(a)[0][1]["kernel"] == "level") >= 4
    # every cell of the stride-3 set needs a sibling and no two of them share a parent
    steps, _ = mem_set_plan(SETS[8][1])
    assert steps[1]["n_siblings"] == steps[0]["n_nodes"] == 1667 == steps[1]["n_nodes"]


def test_special_cases_are_the_single_and_the_range_opening():
    # n = 1: siblings[0 .. 27] of the single opening
    t = tree("a")
    words, values, counts = ref_set(t, [5])
    assert counts == [1] * 28 and words == t.opening(5)[6:34] and values.tolist() == [list(t.opening(5)[2:6])]
    # two ends of the address space: two nodes at every depth below the root's children
    words, _, counts = ref_set(tree("b"), [0, SPACE - 1])
    assert counts == [2] * 27 + [0] and len(words) == 54
    # the pair that meets only at the root
    _, _, counts = ref_set(tree("straddle"), [(1 << 27) - 1, 1 << 27])
    assert counts == [2] * 27 + [0]
    # a contiguous set: per depth [left[k] if used] + [right[k] if used] of the range record
    name, a = SETS[CONTIGUOUS]
    words, values, counts = ref_set(tree(name), a)
    rec, range_values = ref_range(tree(name), a[0], len(a))
    want = []
    for k in range(N_DEPTHS):
        want += [rec[2 + k]] * ((a[0] >> k) & 1) + [rec[30 + k]] * (1 - ((a[-1] >> k) & 1))
    assert words == want and np.array_equal(values, range_values)


def test_set_root_with_other_values_is_the_root_after_the_write():
    rng = np.random.default_rng(7)
    for i in (6, 7, MIXED):                                                       # present, absent and many cells
        name, a = SETS[i]
        root, _, values, words, _ = reference(i)
        new = rng.integers(0, P, size=values.shape, dtype=np.uint32)
        new[0] = 0                                                                # a cell written to zero
        cells = {c[0]: c[1:] for c in range_memories()[name]}
        cells.update({x: tuple(int(y) for y in new[j]) for j, x in enumerate(a)})
        after = RefTree([(x,) + v for x, v in cells.items()])
        o = MemSetOpening(a, values, words)
        assert set_root(o) == root and set_root(o, new) == after.root != root
        # and the sibling words under the new tree are the old ones: only cells of the set changed
        assert ref_set(after, a)[0] == words


def test_bytes_and_hashes_match_the_plan():
    for i in (8, 9):                                                              # the two big dense sets
        _, a, values, words, counts = reference(i)
        steps, m = mem_set_plan(a)
        n = len(a)
        o = MemSetOpening(a, values, words, counts)
        assert o.nbytes == 20 * n + 4 * m == 4 * len(a) + values.nbytes + 4 * len(words)
        assert hashes(a) == 3 * n + sum(s["n_nodes"] for s in steps[1:])
        assert o.nbytes < 136 * n and hashes(a) < 31 * n                          # against cell-by-cell openings


def test_plan_and_host_calls_refuse_bad_sets():
    for bad, needle in (([], "no cells"), ([5, 5], "address 1 is not above address 0"), ([6, 5], "address 1 is not above address 0"),
                        ([5, SPACE], "address 1 is beyond the address space"), (list(range((1 << 20) + 1)), "split the set")):
        with pytest.raises(CmError) as e:
            mem_set_plan(bad)
        assert "status 1:" in str(e.value) and needle in str(e.value), str(e.value)
    big = np.arange((1 << 20) + 1, dtype=np.uint32)
    rc, msg = verify_set_host(0, MemSetOpening(big, np.zeros((big.size, 4), dtype=np.uint32), [0] * 28))
    assert rc == 1 and "split the set" in msg
    rc, msg = verify_set_host(0, MemSetOpening([], np.zeros((0, 4), dtype=np.uint32), []))
    assert rc == 11 and "no cells" in msg
