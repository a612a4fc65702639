"""Reference for range openings, independent of the code under test and built on tests/mem_open_ref.py: the expected record
and values of a range are read off RefTree.node (the pinned host tree builder's node records, a missing node = the default hash
of its depth), check_range refolds a record in pure Python with poseidon2_hash, and ref_plan derives every depth's interval and
sibling use by shifting.

Record words: [start, n_cells, left[0..27], right[0..27]].  With last = start + n - 1 the range covers [start >> k, last >> k] at
depth 28 - k; left[k] = node (start >> k) - 1 when start >> k is odd, right[k] = node (last >> k) + 1 when last >> k is even,
else 0."""
import numpy as np

from tests.mem_open_ref import HEIGHT, P, SPACE, RefTree, memories, poseidon2_hash

N_SLOTS = 28
WORDS = 2 + 2 * N_SLOTS
LEFT, RIGHT = 2, 2 + N_SLOTS
TAIL = 128                                                                      # the widest interval the one-workgroup tail takes


def ref_range(tree, start, n):
    """(the 58 words of cm_mem_range_opening, values (n, 4)) of [start, start + n) under `tree`"""
    last = start + n - 1
    left = [tree.node(28 - k, (start >> k) - 1) if (start >> k) & 1 else 0 for k in range(N_SLOTS)]
    right = [tree.node(28 - k, (last >> k) + 1) if not (last >> k) & 1 else 0 for k in range(N_SLOTS)]
    held = {c[0]: c[1:] for c in tree.cells}
    values = np.array([held.get(a, (0, 0, 0, 0)) for a in range(start, start + n)], dtype=np.uint32).reshape(n, 4)
    return [start, n] + left + right, values


def check_range(root, words, values):
    """pure Python: are the record and the values well formed and do they hash to `root`?"""
    w = [int(x) for x in words]
    v = [int(x) for x in np.asarray(values).reshape(-1)]
    start, n = w[0], w[1]
    if n == 0 or start + n > SPACE or len(v) != 4 * n or any(x >= P for x in v):
        return False
    last = start + n - 1
    level = [poseidon2_hash(poseidon2_hash(v[4 * i], v[4 * i + 1]), poseidon2_hash(v[4 * i + 2], v[4 * i + 3])) for i in range(n)]
    for k in range(N_SLOTS):
        lo, hi = start >> k, last >> k
        assert len(level) == hi - lo + 1
        for used, word in ((lo & 1, w[LEFT + k]), (not hi & 1, w[RIGHT + k])):
            if (word >= P) if used else (word != 0):
                return False
        if lo & 1:
            level.insert(0, w[LEFT + k])
        if not hi & 1:
            level.append(w[RIGHT + k])
        level = [poseidon2_hash(level[i], level[i + 1]) for i in range(0, len(level), 2)]
    return level == [int(root)]


def ref_plan(start, n):
    """one (depth, lo, hi, uses_left, uses_right) per hashing step: the cells (depth 28), then depth 27 .. 0"""
    last = start + n - 1
    return [(28, start, last, False, False)] + \
        [(27 - k, start >> (k + 1), last >> (k + 1), bool((start >> k) & 1), not (last >> k) & 1) for k in range(N_SLOTS)]


# ---- the memories and the shapes the CPU and the GPU tests share -------------------------------------------------------------
def dense_memory():
    rng = np.random.default_rng(20241019)
    return [(777 + i,) + tuple(int(x) for x in rng.integers(0, P, 4)) for i in range(5000)]


def range_memories():
    return dict(memories(), dense=dense_memory(),
                straddle=[((1 << 27) - 1, 21, 22, 23, 24), (1 << 27, 25, 26, 27, 28)])


SHAPES = [
    ("a", 5, 1), ("a", 4, 2), ("a", 4, 3),
    ("b", 0, 1), ("b", 0, 2), ("b", SPACE - 1, 1), ("b", SPACE - 2, 2),
    ("c", 0, 9), ("c", 3, 5), ("c", 8, 8), ("c", 1000, 1), ("c", 123_456_789 - 2, 5),
    ("straddle", (1 << 27) - 3, 6),
    ("dense", 777, 257), ("dense", 778, 256), ("dense", 777, 4099), ("dense", 1000, 2048),
]


def tampers(words, values, root):
    """name -> (words, values, root, what the host verifier's message must contain): each is ONE change to a valid range"""
    w, v = [int(x) for x in words], np.asarray(values, dtype=np.uint32).reshape(-1, 4)
    start, n = w[0], w[1]
    last = start + n - 1
    out = {}

    def value(name, cell, i):
        x = v.copy()
        x[cell, i] = (int(x[cell, i]) + 1) % P
        out[name] = (list(w), x, root, "hashes to root")

    def word(name, pos, new, needle):
        x = list(w)
        x[pos] = new
        out[name] = (x, v.copy(), root, needle)

    value("value of the first cell", 0, 0)
    value("value of a middle cell", n // 2, 1)
    value("value of the last cell", n - 1, 3)
    used_l = [k for k in range(N_SLOTS) if (start >> k) & 1]
    used_r = [k for k in range(N_SLOTS) if not (last >> k) & 1]
    for side, base, used in (("left", LEFT, used_l), ("right", RIGHT, used_r)):
        for which, k in (("lowest", used[0]), ("highest", used[-1])) if used else ():
            word(f"{which} used {side}[{k}]", base + k, (w[base + k] + 1) % P, "hashes to root")
        unused = [k for k in range(N_SLOTS) if k not in used]
        if unused:
            k = unused[len(unused) // 2]
            word(f"unused {side}[{k}]", base + k, 1, f"unused {side} slot at depth {28 - k} is not zero")
    # a neighbouring range with the same values and siblings: some slot changes between used and unused, or the fold differs
    if start + n < SPACE:
        word("start + 1", 0, start + 1, "")
    if start > 0:
        word("start - 1", 0, start - 1, "")
    if n > 1:
        x = list(w)
        x[1] = n - 1
        out["n_cells - 1"] = (x, v[:n - 1].copy(), root, "")
    out["root + 1"] = (list(w), v.copy(), (root + 1) % P, f"hashes to root {root}, not {(root + 1) % P}")
    x = v.copy()
    x[n - 1, 2] = P
    out["value word = P"] = (list(w), x, root, f"value word 2 of cell {last} is not below P")
    if used_l:
        word("left word = P", LEFT + used_l[-1], P, f"the left sibling at depth {28 - used_l[-1]} is not below P")
    if used_r:
        word("right word = P", RIGHT + used_r[0], P, f"the right sibling at depth {28 - used_r[0]} is not below P")
    return out


__all__ = ["HEIGHT", "P", "SPACE", "RefTree", "N_SLOTS", "WORDS", "LEFT", "RIGHT", "TAIL", "SHAPES", "ref_range", "check_range", "ref_plan",
           "range_memories", "dense_memory", "tampers"]
