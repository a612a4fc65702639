"""cm_verify_memory_range_host and cm_mem_range_plan against tests/mem_range_ref.py: the records the reference reads off the
pinned host tree builder's nodes are accepted by the host verifier and by the pure-Python refold, every single change of a record,
its values or the root is refused by both with a message that names the field, and the plan — the records the device verifier
launches from — equals the intervals and sibling uses derived by shifting, with kernel ids that switch once from the per-level
kernel to the tail.  CPU only."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, MemOpening, MemRangeOpening, MemRangeStep, load_library, mem_range_plan, verify_opening, verify_range_host
from tests.mem_range_ref import (LEFT, N_SLOTS, P, RIGHT, SHAPES, SPACE, TAIL, RefTree, check_range, range_memories, ref_plan, ref_range,
                                 tampers)

IDS = [f"{m}-{s}-{n}" for m, s, n in SHAPES]


@pytest.fixture(scope="module")
def trees():
    return {name: RefTree(cells) for name, cells in range_memories().items()}


def _host(root, words, values):
    rc, msg = verify_range_host(root, MemRangeOpening.from_words(words), values)
    assert rc in (0, 11), (rc, msg)
    assert (rc == 0) == check_range(root, words, values), (rc, msg)             # the pure-Python refold agrees
    return rc, msg


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_reference_ranges_are_accepted(trees, shape):
    name, start, n = shape
    t = trees[name]
    words, values = ref_range(t, start, n)
    assert _host(t.root, words, values) == (0, "")
    for a in range(start, start + n):                                             # the values are the tree's cells, zeros where absent
        want = [t.node(30, 4 * a + i) if a in t.present else 0 for i in range(4)]
        assert values[a - start].tolist() == want


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] == 1], ids=[i for i, s in zip(IDS, SHAPES) if s[2] == 1])
def test_a_single_cell_uses_one_slot_per_depth_and_it_is_the_single_openings_sibling(trees, shape):
    name, a, _ = shape
    t = trees[name]
    words, values = ref_range(t, a, 1)
    single = t.opening(a)
    assert verify_opening(t.root, MemOpening.from_words(single))[0] == 0
    for k in range(N_SLOTS):
        used_left = bool((a >> k) & 1)
        assert words[(LEFT if used_left else RIGHT) + k] == single[6 + k]
        assert words[(RIGHT if used_left else LEFT) + k] == 0
    assert values[0].tolist() == single[2:6]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_every_single_change_is_refused(trees, shape):
    name, start, n = shape
    t = trees[name]
    words, values = ref_range(t, start, n)
    cases = tampers(words, values, t.root)
    assert {"value of the first cell", "value of a middle cell", "value of the last cell", "root + 1", "value word = P"} <= set(cases)
    assert any(k.startswith("unused") for k in cases) and any("used left" in k or "used right" in k for k in cases)
    assert ("start + 1" in cases) == (start + n < SPACE) and ("start - 1" in cases) == (start > 0) and ("n_cells - 1" in cases) == (n > 1)
    for what, (w, v, root, needle) in cases.items():
        rc, msg = _host(root, w, v)
        assert rc == 11, what
        assert msg.startswith(f"memory range [{w[0]}, {w[0] + w[1]}): "), (what, msg)
        assert needle in msg, (what, msg)


def test_messages_name_the_field_the_depth_and_the_cell(trees):
    t = trees["c"]
    words, values = ref_range(t, 3, 5)                                            # 3 .. 7: left[0] and left[1] used, right[3] the lowest right
    msg = {k: _host(r, w, v)[1] for k, (w, v, r, _) in tampers(words, values, t.root).items()}
    assert msg["value word = P"].endswith("value word 2 of cell 7 is not below P")
    assert msg["left word = P"].endswith("the left sibling at depth 27 is not below P")       # left[1]
    assert msg["right word = P"].endswith("the right sibling at depth 25 is not below P")     # right[3]: 7 >> 3 = 0 is even
    assert any(m.endswith("unused left slot at depth %d is not zero" % (28 - k)) for k in range(2, N_SLOTS) for m in [msg.get(f"unused left[{k}]", "")])
    assert any(m.endswith("unused right slot at depth %d is not zero" % (28 - k)) for k in range(0, 3) for m in [msg.get(f"unused right[{k}]", "")])
    assert msg["root + 1"].endswith(f"the range hashes to root {t.root}, not {(t.root + 1) % P}")
    for k in ("value of the first cell", "value of a middle cell", "value of the last cell", "lowest used left[0]", "highest used left[1]",
              "lowest used right[3]", "highest used right[27]"):
        assert "the range hashes to root" in msg[k], k
    # a bad header is a verdict too
    bad = list(words)
    bad[1] = 0
    assert "n_cells is 0" in verify_range_host(t.root, MemRangeOpening.from_words(bad), values[:0])[1]
    bad = list(words)
    bad[0] = SPACE - 4
    rc, m = verify_range_host(t.root, MemRangeOpening.from_words(bad), values)
    assert rc == 11 and "beyond the address space" in m


# ---- the plan ---------------------------------------------------------------------------------------------------------------
def _plans():
    return {(m, s, n): mem_range_plan(s, n) for m, s, n in SHAPES}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_plan_equals_the_reference_and_switches_kernels_once(shape):
    _, start, n = shape
    plan = mem_range_plan(start, n)
    assert [(s["depth"], s["lo"], s["hi"], s["uses_left"], s["uses_right"]) for s in plan] == ref_plan(start, n)
    kinds = [s["kernel"] for s in plan]
    assert kinds[0] == "cells" and "cells" not in kinds[1:] and kinds[-1] == "tail"
    n_level = kinds.count("level")
    assert kinds == ["cells"] + ["level"] * n_level + ["tail"] * (28 - n_level)
    for i in range(1, 29):                                                        # a level step reads more than TAIL nodes, a tail step at most TAIL
        width_in = plan[i - 1]["hi"] - plan[i - 1]["lo"] + 1
        assert (kinds[i] == "level") == (width_in > TAIL), (i, width_in)
    assert plan[-1]["depth"] == 0 and plan[-1]["lo"] == plan[-1]["hi"] == 0


def test_the_shapes_reach_every_kernel_and_both_sides_of_the_tail_width():
    assert TAIL <= 1024
    plans = _plans()
    level_counts, tail_entry, combos = {}, set(), set()
    for key, plan in plans.items():
        kinds = [s["kernel"] for s in plan]
        level_counts[key] = kinds.count("level")
        first_tail = kinds.index("tail")
        tail_entry.add(plan[first_tail - 1]["hi"] - plan[first_tail - 1]["lo"] + 1)
        combos |= {(s["uses_left"], s["uses_right"]) for s in plan if s["kernel"] == "level"}
    assert {k for p in plans.values() for k in (s["kernel"] for s in p)} == {"cells", "level", "tail"}
    assert level_counts[("dense", 777, 4099)] >= 2 and level_counts[("dense", 1000, 2048)] >= 2
    assert level_counts[("dense", 777, 257)] >= 1 and level_counts[("dense", 778, 256)] >= 1      # 257 and 256 nodes: above the tail's width
    assert 1 in tail_entry and any(TAIL // 2 < w <= TAIL for w in tail_entry), tail_entry
    assert combos == {(False, False), (False, True), (True, False), (True, True)}
    # every combination of sibling use also reaches the tail, and the cell kernel runs more than one block
    assert {(s["uses_left"], s["uses_right"]) for p in plans.values() for s in p if s["kernel"] == "tail"} == combos
    assert any(n > 256 for _, _, n in SHAPES)
    # the straddling range: both siblings at depth after depth up to depth 2, none at depth 1
    straddle = plans[("straddle", (1 << 27) - 3, 6)]
    by_depth = {s["depth"]: s for s in straddle[1:]}                             # the step that produces depth d reads the siblings of depth d + 1
    assert all(by_depth[d - 1]["uses_left"] and by_depth[d - 1]["uses_right"] for d in range(2, 27))
    assert not by_depth[0]["uses_left"] and not by_depth[0]["uses_right"]
    # aligned: no sibling below k = 3
    assert all(not s["uses_left"] and not s["uses_right"] for s in plans[("c", 8, 8)][1:4])


def test_plan_refusals():
    L = load_library()
    steps, k = (MemRangeStep * 29)(), C.c_uint32(77)
    for start, n, cap, st, kk in ((0, 0, 29, steps, k), (SPACE - 1, 2, 29, steps, k), (SPACE, 1, 29, steps, k), (0, 1, 28, steps, k),
                                  (0, 1, 29, None, k), (0, 1, 29, steps, None)):
        rc = L.cm_mem_range_plan(C.c_uint32(start), C.c_uint32(n), st, C.c_uint32(cap), C.byref(kk) if kk is not None else None)
        assert rc == 1, (start, n, cap)
    assert k.value == 77
    with pytest.raises(CmError):
        mem_range_plan(SPACE - 1, 2)
    assert len(mem_range_plan(0, SPACE)) == 29 and len(mem_range_plan(SPACE - 1, 1)) == 29   # the plan itself has no 2^24 limit


def test_host_verifier_limits():
    L = load_library()
    rec = MemRangeOpening.from_words([0, (1 << 24) + 1] + [0] * 56)
    v = np.zeros(4, dtype=np.uint32)
    assert L.cm_verify_memory_range_host(C.c_uint32(0), C.byref(rec), v.ctypes.data_as(C.POINTER(C.c_uint32))) == 1   # read before the values
