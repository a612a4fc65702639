"""The batched verifiers' host side (cm_mem_batch_plan, the refusals of cm_verify_memory_transitions / cm_verify_memory_sets) without
a GPU: the plan against one derived in Python from tests/mem_set_ref.levels, proof in numbers that the batches of
tests/test_gpu_mem_batch.py reach every path of the kernels, the status-1 refusals with the message naming the part, parts
without cells, and the status without a GPU."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemSetOpening, MemSetViewC, MemTransition, MemTransitionViewC, _set_view, _transition_args, _transition_view,
                             load_library, mem_batch_launches, mem_batch_plan, mem_set_plan, verify_sets, verify_transitions)
from tests.mem_batch_cases import BATCHES, BLOCK, ref_batch_plan, small_parts, tail_entry
from tests.mem_set_ref import SETS, SPACE, TAIL, levels, parent_kinds

L = load_library()


def lists_of(name):
    return [SETS[i][1] for i in BATCHES[name]]


def as_tuples(plan):
    return [(s["depth"], s["n_nodes"], s["widest_part"], s["kernel"]) for s in plan]


def last_error():
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return buf.value.decode(errors="replace")


def has_gpu():
    import torch
    return torch.cuda.is_available()


@pytest.mark.parametrize("name", list(BATCHES))
def test_the_plan_of_a_batch_equals_the_python_plan(name):
    lists = lists_of(name)
    plan = mem_batch_plan(lists, L)
    assert as_tuples(plan) == ref_batch_plan(lists) and len(plan) == 29
    # a part alone: the batch's plan is the single record's
    for a in lists[:3]:
        single, _ = mem_set_plan(a, L)
        assert as_tuples(mem_batch_plan([a], L)) == [(s["depth"], s["n_nodes"], s["n_nodes"], s["kernel"]) for s in single]


def test_the_launches_do_not_depend_on_the_number_of_parts():
    widest = SETS[8][1]                                                           # the stride-3 set: six per-level launches
    one = mem_batch_launches(mem_batch_plan([widest], L))
    assert one == 1 + 6 + 1
    for k in (2, 12, 64):
        assert mem_batch_launches(mem_batch_plan([widest] * k, L)) == one
    assert mem_batch_launches(mem_batch_plan(lists_of("all"), L)) == one          # the part with the most per-level steps decides
    small = [p["a"] for p in small_parts()]
    assert mem_batch_launches(mem_batch_plan(small, L)) == mem_batch_launches(mem_batch_plan(small[:1], L)) == 2   # cells and tail


def test_parts_that_do_not_reach_the_device_are_left_out_of_the_plan():
    good = SETS[6][1]
    swapped = [good[1], good[0]] + good[2:]
    assert mem_batch_plan([[], []], L) == []                                      # a batch of only such parts launches nothing
    assert mem_batch_plan([swapped, [SPACE]], L) == []
    assert mem_batch_plan([[], good, swapped, [], SETS[10][1], [5, 5]], L) == mem_batch_plan([good, SETS[10][1]], L)
    assert as_tuples(mem_batch_plan([[], good, swapped], L)) == ref_batch_plan([[], good, swapped])


def test_the_gpu_batches_reach_every_path():
    every = lists_of("all")
    plan = ref_batch_plan(every)
    lv = [levels(a) for a in every]
    level_steps = [k for k in range(28) if plan[k + 1][3] == "level"]
    tail_steps = [k for k in range(28) if plan[k + 1][3] == "tail"]
    assert level_steps == list(range(6)) and tail_steps == list(range(6, 28))
    # a level launch in which one part is at or below TAIL nodes while another is above: the narrow part rides along
    for k in level_steps:
        widths = [len(l[k]) for l in lv]
        assert min(widths) <= TAIL < max(widths), (k, widths)
    # a level launch whose combined parents span more than one block, with a part boundary strictly inside a block
    for name in ("all", "reversed", "widest in the middle"):
        lvn = [levels(a) for a in lists_of(name)]
        parents = [len(l[1]) for l in lvn]
        bounds = np.cumsum(parents)[:-1]
        assert sum(parents) > 2 * BLOCK and any(b % BLOCK for b in bounds), (name, parents)
        assert any(b > BLOCK and b % BLOCK for b in bounds), (name, bounds)       # a boundary inside a block that is not the first
    # tail-only batches with more parts than a block of the level kernel, and than the tail's workgroup, has lanes
    small = [p["a"] for p in small_parts()]
    assert len(small) == 300 > BLOCK and 130 > TAIL
    for lists in (small, small[:130]):
        assert [s[3] for s in ref_batch_plan(lists)] == ["cells"] + ["tail"] * 28
    assert small[0] == [0] and small[1] == [0, SPACE - 1] and small[2] == [(1 << 27) - 1, 1 << 27]
    assert {len(a) for a in small} == {1, 2}
    # parts enter the tail at width 1, 2, 65, 72 and 79
    entries = {}
    for name in ("all", "range first", "three runs last", ):
        k, widths = tail_entry(lists_of(name))
        entries[name] = (k, widths)
    assert entries["all"][0] == 6 and {1, 2, 79} <= set(entries["all"][1])
    assert entries["range first"][0] == 2 and entries["range first"][1][0] == 65 and {1, 2} <= set(entries["range first"][1])
    assert entries["three runs last"][0] == 1 and entries["three runs last"][1][-1] == 72
    assert tail_entry(small) == (0, [len(a) for a in small])
    # parents with only a left child, only a right child and both children, in a level step and in a tail step
    kinds = lambda steps: set().union(*(parent_kinds(a, k) for a in every for k in steps))
    assert kinds(level_steps) == kinds(tail_steps) == {"left", "right", "both"}
    assert parent_kinds(SETS[8][1], 0) == {"left", "right"} and "both" in parent_kinds(SETS[8][1], 1)
    assert set().union(*(parent_kinds(SETS[11][1], k) for k in range(1, 28))) == {"left", "right", "both"}   # the three-run set, in its batch's tail


# ---- refusals: status 1 before any address is read, the message naming the part ----------------------------------------------
def _transition(n=2, m=54):
    return MemTransition([0, SPACE - 1][:n], np.zeros((n, 4)), np.zeros((n, 4)), np.zeros(m), 1, 2)


def _raw(fn, views, n_parts, planes, ok=True):
    oks, got = (C.c_uint8 * max(n_parts, 1))(), (C.c_uint32 * max(planes * n_parts, 1))()
    rc = fn(views, C.c_uint32(n_parts), oks if ok else None, got, C.c_uint64(0))
    return rc, last_error() if rc else ""


def _views(ts, kind):
    views = ((MemTransitionViewC if kind == 2 else MemSetViewC) * max(len(ts), 1))()
    keep = []
    for i, t in enumerate(ts):
        views[i], k = _transition_view(t) if kind == 2 else _set_view(7, MemSetOpening(t.addresses, t.old_values, t.siblings))
        keep.append(k)
    return views, keep


@pytest.mark.parametrize("kind", [2, 1], ids=["transitions", "sets"])
def test_the_call_refuses_with_status_1_and_names_the_part(kind):
    fn = L.cm_verify_memory_transitions if kind == 2 else L.cm_verify_memory_sets
    who = "cm_verify_memory_transitions" if kind == 2 else "cm_verify_memory_sets"
    good = [_transition(), _transition(1, 28), _transition()]
    views, keep = _views(good, kind)
    assert _raw(fn, None, 3, kind) == (1, f"{who}: null argument")
    assert _raw(fn, views, 3, kind, ok=False) == (1, f"{who}: null argument")
    for n_parts in (0, (1 << 16) + 1):
        rc, why = _raw(fn, views, n_parts, kind)
        assert rc == 1 and why.startswith(f"{who}: no parts, or more than 2^16 parts"), why
    views, keep = _views(good, kind)
    views[1].struct_size -= 1
    rc, why = _raw(fn, views, 3, kind)
    assert rc == 1 and why.startswith(f"{who}: part 1: struct_size does not cover cm_mem_"), why
    fields = ("addresses", "old_values", "new_values", "siblings") if kind == 2 else ("addresses", "values", "siblings")
    for f in fields:
        views, keep = _views(good, kind)
        setattr(views[2], f, None)
        assert _raw(fn, views, 3, kind) == (1, f"{who}: part 2: null array"), f
    views, keep = _views(good, kind)
    views[1].n = (1 << 20) + 1                                                    # decided before any address is read: the arrays are short
    assert _raw(fn, views, 3, kind) == (1, f"{who}: part 1: more than 2^20 cells: split the set")
    views, keep = _views(good, kind)
    views[0].n = views[2].n = 1 << 19
    rc, why = _raw(fn, views, 3, kind)
    assert rc == 1 and why == f"{who}: the parts hold {(1 << 20) + 1} cells, more than 2^20 in one call: verify in groups", why
    with pytest.raises(CmError) as e:
        (verify_transitions if kind == 2 else lambda ts, lib: verify_sets(7, ts, lib))([], L)
    assert e.value.status == 1 and "no parts" in e.value.message


def test_the_plan_query_refuses_like_the_call():
    a = np.array([1, 2, 3], dtype=np.uint32)
    ptr = lambda x: x.ctypes.data_as(C.POINTER(C.c_uint32))
    lists = (C.POINTER(C.c_uint32) * 2)(ptr(a), ptr(a))
    steps, k = (C.c_uint32 * (4 * 29))(), C.c_uint32(0)
    call = lambda ls, n, n_parts, cap=29: L.cm_mem_batch_plan(ls, ptr(np.array(n, dtype=np.uint32)), C.c_uint32(n_parts), steps, C.c_uint32(cap), C.byref(k))
    assert call(lists, [3, 3], 2) == 0 and k.value == 29
    assert call(None, [3, 3], 2) == 1 and last_error() == "cm_mem_batch_plan: null argument"
    assert call(lists, [3, 3], 0) == 1 and "no parts" in last_error()
    assert call(lists, [3, (1 << 20) + 1], 2) == 1 and last_error() == "cm_mem_batch_plan: part 1: more than 2^20 cells: split the set"
    assert call(lists, [1 << 20, 1], 2) == 1 and "verify in groups" in last_error()
    lists[1] = None
    assert call(lists, [3, 3], 2) == 1 and last_error() == "cm_mem_batch_plan: part 1: null array"
    assert call(lists, [3, 0], 2) == 0 and k.value == 29                          # (a NULL list without a count is a part without cells)
    assert call(lists, [3, 0], 2, cap=28) == 1 and k.value == 29 and "29 steps" in last_error()


def test_without_a_gpu_the_call_returns_what_the_single_calls_return():
    """a call that passes the argument checks: cm_init's status (3) on a machine without a GPU, as cm_verify_memory_transition and
    cm_verify_memory_set; on a machine with one, the verdicts of parts without cells, which need no launch"""
    still = [MemTransition([], [], [], [], 5, 5), MemTransition([], [], [], [], 5, 6), MemTransition([], [], [], [1], 5, 5)]
    views, keep = _views(still, 2)
    oks, got = (C.c_uint8 * 3)(), (C.c_uint32 * 6)()
    rc = L.cm_verify_memory_transitions(views, C.c_uint32(3), oks, got, C.c_uint64(0))
    args, keep2 = _transition_args(still[0])
    ok1, got1 = C.c_uint8(0), (C.c_uint32 * 2)()
    single = L.cm_verify_memory_transition(*args, C.byref(ok1), got1, C.c_uint64(0))
    assert rc == single
    if has_gpu():
        assert rc == 0 and list(oks) == [1, 0, 0] and list(got) == [5, 5, 5, 5, 0, 0]
    else:
        assert rc == 3 and last_error()
        sviews, keep3 = _views([_transition()], 1)
        assert L.cm_verify_memory_sets(sviews, C.c_uint32(1), oks, got, C.c_uint64(0)) == 3
