"""Reference for set openings, independent of the code under test and built on tests/mem_open_ref.py and tests/mem_range_ref.py:
the expected sibling words and values of a set are read off RefTree.node (the pinned host tree builder's node records, a missing
node = the default hash of its depth), check_set refolds a record in pure Python with poseidon2_hash, and ref_plan derives every
depth's node list with Python sets.

The statement: the addresses are strictly ascending and below 2^28; S_k = the sorted distinct a >> k; a node x of S_k needs a
sibling exactly when x ^ 1 is not in S_k; the words come depth by depth, k = 0 first, by ascending node, each node(28 - k, x ^ 1)."""
import numpy as np

from tests.mem_open_ref import P, SPACE, RefTree, poseidon2_hash
from tests.mem_range_ref import dense_memory, range_memories

N_DEPTHS = 28
TAIL = 128                                                                      # the widest level the one-workgroup tail takes
MAX_CELLS = 1 << 20


def levels(addresses):
    """[S_0, ..., S_28] as sorted lists"""
    out = [sorted({int(a) for a in addresses})]
    for _ in range(N_DEPTHS):
        out.append(sorted({x >> 1 for x in out[-1]}))
    return out


def ref_set(tree, addresses):
    """(sibling words, values (n, 4), counts[28]) of the strictly ascending `addresses` under `tree`"""
    a = [int(x) for x in addresses]
    assert a == sorted(set(a))
    words, counts = [], []
    for k, s in enumerate(levels(a)[:N_DEPTHS]):
        have = set(s)
        need = [x for x in s if x ^ 1 not in have]
        words += [tree.node(28 - k, x ^ 1) for x in need]
        counts.append(len(need))
    held = {c[0]: c[1:] for c in tree.cells}
    values = np.array([held.get(x, (0, 0, 0, 0)) for x in a], dtype=np.uint32).reshape(len(a), 4)
    return words, values, counts


def fold(addresses, values, words):
    """pure Python, the fold of the statement: the root, or None when the statement is malformed"""
    a = [int(x) for x in addresses]
    v = [int(x) for x in np.asarray(values).reshape(-1)]
    w = [int(x) for x in words]
    if not a or len(a) > MAX_CELLS or len(v) != 4 * len(a) or any(x >= SPACE for x in a) or any(y <= x for x, y in zip(a, a[1:])):
        return None
    if any(x >= P for x in v) or any(x >= P for x in w):
        return None
    nodes = [(x, poseidon2_hash(poseidon2_hash(v[4 * i], v[4 * i + 1]), poseidon2_hash(v[4 * i + 2], v[4 * i + 3]))) for i, x in enumerate(a)]
    q = 0
    for _ in range(N_DEPTHS):
        up, j = [], 0
        while j < len(nodes):
            x, h = nodes[j]
            if not x & 1 and j + 1 < len(nodes) and nodes[j + 1][0] == x + 1:
                up.append((x >> 1, poseidon2_hash(h, nodes[j + 1][1])))
                j += 2
                continue
            if q >= len(w):
                return None
            up.append((x >> 1, poseidon2_hash(w[q], h) if x & 1 else poseidon2_hash(h, w[q])))
            q += 1
            j += 1
        nodes = up
    return nodes[0][1] if q == len(w) and len(nodes) == 1 else None


def check_set(root, addresses, values, words):
    got = fold(addresses, values, words)
    return got is not None and got == int(root)


def parent_kinds(addresses, k):
    """the kinds of parent the step S_k -> S_{k+1} holds: 'both' children in the set, only the 'left', only the 'right'"""
    s = set(levels(addresses)[k])
    return {"both" if (2 * p in s and 2 * p + 1 in s) else "left" if 2 * p in s else "right" for p in {x >> 1 for x in s}}


def ref_plan(addresses):
    """([(depth, n_nodes, n_siblings, kernel)] * 29, n_siblings in all): the cells, then the step S_k -> S_{k+1} per k"""
    lv = levels(addresses)
    steps, total = [(28, len(lv[0]), 0, "cells")], 0
    for k in range(N_DEPTHS):
        have = set(lv[k])
        need = sum(1 for x in lv[k] if x ^ 1 not in have)
        steps.append((27 - k, len(lv[k + 1]), need, "level" if len(lv[k]) > TAIL else "tail"))
        total += need
    return steps, total


def hashes(addresses):
    """Poseidon2 calls of the fold: three per cell and one per parent"""
    lv = levels(addresses)
    return 3 * len(lv[0]) + sum(len(s) for s in lv[1:])


# ---- the sets the CPU and the GPU tests share --------------------------------------------------------------------------------
def _random_dense():
    rng = np.random.default_rng(20241019)
    cells = [c[0] for c in dense_memory()]
    return sorted(int(x) for x in rng.choice(cells, 1500, replace=False))


SETS = [
    ("a", [5]), ("a", [4, 5]), ("a", [4, 6]),
    ("b", [0]), ("b", [0, SPACE - 1]),                                          # two nodes at every depth: 54 words
    ("straddle", [(1 << 27) - 1, 1 << 27]),                                     # the pair meets only at the root
    ("c", [0, 1, 2, 3, 7, 8, 1000]), ("c", [2, 6, 123_456_789]),                # a held zero cell, an absent near and an absent far cell
    ("dense", list(range(777, 5777, 3))),                                       # every cell needs a sibling, no two share a parent
    ("dense", _random_dense()),                                                 # paired and lone nodes mixed
    ("dense", list(range(1000, 1257))),
    ("dense", list(range(777, 817)) + list(range(3000, 3100)) + [5776]),
]
SET_IDS = [f"{m}-{len(a)}-{a[0]}" + (f"-{a[1] - a[0]}" if len(a) > 1 else "") for m, a in SETS]
CONTIGUOUS = 10                                                                 # SETS[10] is a range
MIXED = 11


def tampers(addresses, values, words, root):
    """name -> (addresses, values, words, root, what the host verifier's message must contain): each is ONE change to a valid set"""
    a, v, w = [int(x) for x in addresses], np.asarray(values, dtype=np.uint32).reshape(-1, 4), [int(x) for x in words]
    n, m = len(a), len(w)
    out = {}

    def value(name, cell, i):
        x = v.copy()
        x[cell, i] = (int(x[cell, i]) + 1) % P
        out[name] = (list(a), x, list(w), root, "hashes to root")

    def word(name, pos):
        x = list(w)
        x[pos] = (x[pos] + 1) % P
        out[name] = (list(a), v.copy(), x, root, "hashes to root")

    value("value of the first cell", 0, 0)
    value("value of a middle cell", n // 2, 1)
    value("value of the last cell", n - 1, 3)
    word("the first sibling", 0)
    word("a middle sibling", m // 2)
    word("the last sibling", m - 1)
    out["one word appended"] = (list(a), v.copy(), w + [1], root, f"{m + 1} sibling words where the addresses need {m}")
    out["one word dropped"] = (list(a), v.copy(), w[:-1], root, f"{m - 1} sibling words where the addresses need {m}")
    q = m // 3
    counts = ref_plan(a)[0][1:]
    depth, seen = None, 0
    for k, (_, _, c, _) in enumerate(counts):
        if q < seen + c:
            depth = 28 - k
            break
        seen += c
    x = list(w)
    x[q] = P
    out["a sibling = P"] = (list(a), v.copy(), x, root, f"sibling {q} (depth {depth}) is not below P")
    x = v.copy()
    x[n - 1, 2] = P
    out["a value = P"] = (list(a), x, list(w), root, f"value word 2 of cell {a[-1]} is not below P")
    if n > 1:
        x = list(a)
        x[0], x[1] = x[1], x[0]
        out["two addresses swapped"] = (x, v.copy(), list(w), root, "address 1 is not above address 0")
        x = list(a)
        x[n - 1] = x[n - 2]
        out["an address repeated"] = (x, v.copy(), list(w), root, f"address {n - 1} is not above address {n - 2}")
    # a neighbouring set with the same values and words: the counts change, or the fold differs, or the order breaks.  (Moving an
    # absent cell next to another absent one can give a TRUE statement — two zero cells hash alike on either side — so the
    # address moved is the first, from the middle on, whose move the Python fold refuses.)
    for j in list(range(n // 2, n)) + list(range(n // 2)):
        x = list(a)
        x[j] += 1
        if fold(x, v, w) != root:
            out["an address + 1"] = (x, v.copy(), list(w), root, "")
            break
    assert "an address + 1" in out
    out["root + 1"] = (list(a), v.copy(), list(w), (root + 1) % P, f"hashes to root {root}, not {(root + 1) % P}")
    return out


__all__ = ["P", "SPACE", "RefTree", "N_DEPTHS", "TAIL", "SETS", "SET_IDS", "CONTIGUOUS", "MIXED", "levels", "ref_set", "fold", "check_set",
           "parent_kinds", "ref_plan", "hashes", "tampers", "range_memories"]
