"""Reference for composed transitions, independent of the code under test and built on tests/mem_open_ref.py (RefTree) and
tests/mem_set_ref.py (ref_set, ref_plan): a chain is a starting memory M0 and address sets A_1 .. A_k; M_i is M_{i-1} with every
cell of A_i rewritten, T_i = RefTree(M_i); part i is (A_i, ref_set(T_{i-1}, A_i), ref_set(T_i, A_i), T_{i-1}.root, T_i.root) and
the reference composition (U, ref_set(T_0, U), ref_set(T_k, U), T_0.root, T_k.root) — every word read off the trees' node
records, nothing folded with the library's set or transition code.  The helper asserts the premise: the words of U under T_0 and
under T_k are identical."""
import functools

import numpy as np

from cairo_m_amd.lib import MemTransition
from tests.mem_open_ref import P, SPACE, RefTree, memories
from tests.mem_range_ref import dense_memory
from tests.mem_set_ref import ref_plan, ref_set

ZERO = (0, 0, 0, 0)


@functools.lru_cache(maxsize=1)
def spread():
    """257 distinct addresses all over the address space, the two ends among them, no two of the inner ones buddies, and a memory
    that holds every other one (the idea of tests/test_gpu_transition.py::_spread)"""
    rng = np.random.default_rng(20241020)
    a = sorted({0, SPACE - 1} | {int(x) & ~1 for x in rng.integers(2, SPACE - 2, 300)})[:256] + [SPACE - 1]
    a = sorted(set(a))
    assert len(a) == 257 and a[0] == 0 and a[-1] == SPACE - 1 and all(x ^ 1 not in a for x in a[1:-1])
    cells = {x: tuple(int(w) for w in rng.integers(0, P, 4)) for x in a[::2]}
    return a, cells


@functools.lru_cache(maxsize=1)
def dense():
    return {c[0]: tuple(c[1:]) for c in dense_memory()}


@functools.lru_cache(maxsize=1)
def both():
    """the dense memory and the spread cells in one memory"""
    return {**dense(), **spread()[1]}


def _tree(mem):
    return RefTree([(x,) + tuple(v) for x, v in mem.items()])


def build(m0, sets, overrides=None, seed=1):
    """{parts: [dict], ref: dict, trees: [RefTree]} of the chain; overrides: {(part index, address): value} instead of a random one"""
    rng = np.random.default_rng(20241100 + seed)
    overrides = overrides or {}
    mem = dict(m0)
    trees, parts = [_tree(mem)], []
    for i, s in enumerate(sets):
        s = sorted({int(x) for x in s})
        for x in s:
            mem[x] = overrides.get((i, x), tuple(int(w) for w in rng.integers(0, P, 4)))
        trees.append(_tree(mem) if s else trees[-1])
        words, old, _ = ref_set(trees[i], s)
        words_after, new, _ = ref_set(trees[i + 1], s)
        assert words == words_after
        parts.append({"a": s, "old": old, "new": new, "words": words, "root0": trees[i].root, "root1": trees[i + 1].root})
    u = sorted(set().union(*[p["a"] for p in parts]))
    words, old, counts = ref_set(trees[0], u)
    words_after, new, _ = ref_set(trees[-1], u)
    assert words == words_after                                                  # the premise: the same words under the first and the last tree
    ref = {"a": u, "old": old, "new": new, "words": words, "counts": counts, "root0": trees[0].root, "root1": trees[-1].root}
    return {"parts": parts, "ref": ref, "trees": trees}


def _one():
    a, cells = spread()
    return build(cells, [[a[4], a[5], a[6]]])


def _far():
    a, cells = spread()
    return build(cells, [[a[4]], [a[200]]])


def _buddies():
    a, cells = spread()
    x = a[6]
    assert x % 2 == 0 and x in cells and x ^ 1 not in cells
    c = build(cells, [[x], [x ^ 1]])
    assert c["ref"]["counts"][0] == 0 and len(c["ref"]["words"]) == 27          # no word at depth 28
    # part 2 holds node(28, x) as hashed AFTER part 1's write: stale against the first tree, and never needed
    assert c["parts"][1]["words"][0] == c["trees"][1].node(28, x) != c["trees"][0].node(28, x)
    return c


def _cousins_top():
    a, cells = spread()
    return build(cells, [[(1 << 27) - 1], [1 << 27]])


def _cousins_low():
    m0 = {c[0]: tuple(c[1:]) for c in memories()["c"]}
    return build(m0, [[4, 5], [6, 7]])


def _same_set():
    a, _ = spread()
    s = list(range(1000, 1030)) + a[10:20]
    c = build(both(), [s, s, s])
    assert c["ref"]["words"] == c["parts"][0]["words"]
    assert np.array_equal(c["ref"]["old"], c["parts"][0]["old"]) and np.array_equal(c["ref"]["new"], c["parts"][2]["new"])
    return c


def _gap_and_restore():
    a, cells = spread()
    m0 = both()
    cc, d = 2000, a[8]
    c = build(m0, [[cc, d, 2001, a[9]], [2002, 2003, a[30]], [cc, d, 2004]], {(2, d): m0[d]})
    i = c["ref"]["a"].index(d)
    assert tuple(c["ref"]["old"][i]) == tuple(c["ref"]["new"][i]) == m0[d]      # listed, with old == new
    assert cc not in c["parts"][1]["a"]
    return c


def _create_and_zero():
    a, cells = spread()
    z, top = a[5], a[4]
    assert z not in cells and top in cells
    c = build(cells, [[z, a[40]], [z, top]], {(1, z): ZERO, (1, top): (1, 2, 3, P - 1)})
    i = c["ref"]["a"].index(z)
    assert tuple(c["ref"]["old"][i]) == tuple(c["ref"]["new"][i]) == ZERO and tuple(c["parts"][0]["new"][0 if z < a[40] else 1]) != ZERO
    return c


def _ab():
    a, _ = spread()
    return [a[4], 1000, 1001], [1001, 1002, a[100]]


def _empties():
    x, y = _ab()
    return build(both(), [[], x, [], y, []])


def _no_empties():
    x, y = _ab()
    return build(both(), [x, y])


def _all_empty():
    return build(spread()[1], [[], []])


def _wide():
    a, cells = spread()
    rng = np.random.default_rng(20241101)
    m0 = both()
    sizes, sets = [129, 300, 200, 257, 180], []
    for i, size in enumerate(sizes):
        keep = [int(x) for x in rng.choice(sets[-1], len(sets[-1]) // 2, replace=False)] if sets else [0, SPACE - 1]
        keep = keep[:size // 2]
        run = list(range(900 + 350 * i, 900 + 350 * i + size // 4))              # a run of the dense memory (and a little below it)
        pool = [x for x in a + list(range(777, 5777, 7)) if x not in set(keep) | set(run)]
        fresh = [int(x) for x in rng.choice(pool, size - len(set(keep) | set(run)), replace=False)]
        s = sorted(set(keep) | set(run) | set(fresh))
        assert len(s) == size
        sets.append(s)
    c = build(m0, sets)
    u = c["ref"]["a"]
    assert 0 in u and SPACE - 1 in u and len(u) > 512
    steps, _ = ref_plan(u)
    assert sum(1 for s in steps if s[3] == "level") >= 3 and steps[-1][3] == "tail"
    for p, q in zip(sets, sets[1:]):
        assert len(set(p) & set(q)) >= min(len(p), len(q)) // 3
    return c


def _edge_512():
    return build(dense(), [range(1000, 1256), range(1128, 1384)])                # N = 512, each part exactly 256 cells


def _edge_513():
    return build(dense(), [range(1000, 1256), range(1128, 1385)])                # N = 513: parts of 256 and 257 cells


BUILDERS = {
    "one": _one, "far": _far, "buddies": _buddies, "cousins_top": _cousins_top, "cousins_low": _cousins_low, "same_set": _same_set,
    "gap_and_restore": _gap_and_restore, "create_and_zero": _create_and_zero, "empties": _empties, "all_empty": _all_empty,
    "wide": _wide, "edge_512": _edge_512, "edge_513": _edge_513,
}
CHAINS = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def chain(name):
    if name == "no_empties":
        return _no_empties()
    return BUILDERS[name]()


def as_transition(p):
    return MemTransition(p["a"], p["old"], p["new"], p["words"], p["root0"], p["root1"])


def parts_of(name):
    return [as_transition(p) for p in chain(name)["parts"]]


def assert_equals(t, r):
    assert t.addresses.tolist() == r["a"] and t.siblings.tolist() == r["words"]
    assert np.array_equal(t.old_values, r["old"]) and np.array_equal(t.new_values, r["new"])
    assert (t.root_before, t.root_after) == (r["root0"], r["root1"])
    assert t.nbytes == 36 * len(r["a"]) + 4 * len(r["words"])


def same_bytes(x, y):
    return all(getattr(x, f).tobytes() == getattr(y, f).tobytes() for f in ("addresses", "old_values", "new_values", "siblings")) and \
        (x.root_before, x.root_after, x.n_zero_only) == (y.root_before, y.root_after, y.n_zero_only)


# ---- the refusals the CPU and the GPU tests share: each is ONE change to a valid chain ------------------------------------------
def _with(t, **kw):
    f = dict(addresses=t.addresses, old_values=t.old_values, new_values=t.new_values, siblings=t.siblings, root_before=t.root_before,
             root_after=t.root_after)
    f.update(kw)
    return MemTransition(f["addresses"], f["old_values"], f["new_values"], f["siblings"], f["root_before"], f["root_after"])


REFUSALS = ["roots that do not chain", "a seam's old word bumped", "two addresses swapped", "an address at 2^28", "a sibling word appended",
            "a sibling word dropped"]


@functools.lru_cache(maxsize=1)
def refusals():
    """{what: (parts, status, needle)}"""
    gap, wide = parts_of("gap_and_restore"), parts_of("wide")
    out = []
    p = list(gap)
    p[1] = _with(p[1], root_before=p[1].root_before ^ 1)
    out.append(("roots that do not chain", p, 11, f"part 1 starts at root {p[1].root_before}, part 0 ended at root {gap[0].root_after}"))
    # the seam cells of part 2 are 2000 and a spread address, both last written by part 0: both bumped, the lowest is named
    seams = sorted(set(gap[2].addresses.tolist()) & set(gap[0].addresses.tolist()))
    assert len(seams) == 2
    old = gap[2].old_values.copy()
    for x in seams:
        old[gap[2].addresses.tolist().index(x), 2] ^= 1
    p = list(gap)
    p[2] = _with(p[2], old_values=old)
    out.append(("a seam's old word bumped", p, 11, f"cell {seams[0]}: part 2 reads a value part 0 did not leave"))
    a = wide[1].addresses.copy()
    a[[7, 8]] = a[[8, 7]]
    p = list(wide)
    p[1] = _with(p[1], addresses=a)
    out.append(("two addresses swapped", p, 11, "part 1: address 8 is not above address 7"))
    a = wide[2].addresses.copy()
    a[-1] = SPACE
    p = list(wide)
    p[2] = _with(p[2], addresses=a)
    out.append(("an address at 2^28", p, 11, f"part 2: address {a.size - 1} is beyond the address space of 2^28 cells"))
    m = wide[3].siblings.size
    p = list(wide)
    p[3] = _with(p[3], siblings=np.append(wide[3].siblings, np.uint32(5)))
    out.append(("a sibling word appended", p, 11, f"part 3: {m + 1} sibling words where the addresses need {m}"))
    p = list(wide)
    p[3] = _with(p[3], siblings=wide[3].siblings[:-1])
    out.append(("a sibling word dropped", p, 11, f"part 3: {m - 1} sibling words where the addresses need {m}"))
    assert [o[0] for o in out] == REFUSALS
    return {o[0]: o[1:] for o in out}
