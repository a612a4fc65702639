"""Reference for memory openings, independent of the code under test: the node records of the pinned host tree builder
(cm_adapter_partial_tree, tests/test_adapter.py) give {(depth, index): value}; a node the map lacks is the default hash of its
depth, computed with cm_poseidon2_permute (KAT-pinned to the reference); the expected cm_mem_opening of an address is read off
the map, and check() recomputes a record's root in pure Python."""
import ctypes as C
import functools

import numpy as np

from cairo_m_amd.lib import load_library, partial_merkle_tree

P = (1 << 31) - 1
HEIGHT = 30
N_SIBLINGS = 28
SPACE = 1 << 28
WORDS = 34


@functools.lru_cache(maxsize=1 << 16)
def poseidon2_hash(l, r):
    s = np.zeros(16, dtype=np.uint32)
    s[0], s[1] = l, r
    load_library().cm_poseidon2_permute(s.ctypes.data_as(C.POINTER(C.c_uint32)))
    return int(s[0])


@functools.lru_cache(maxsize=1)
def default_hashes():
    d = [0] * (HEIGHT + 1)
    for depth in range(HEIGHT - 1, -1, -1):
        d[depth] = poseidon2_hash(d[depth + 1], d[depth + 1])
    return d


class RefTree:
    """cells: [(address, v0, v1, v2, v3)] in any order, addresses distinct."""

    def __init__(self, cells):
        cells = sorted((int(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[4])) for c in cells)
        self.cells = cells
        self.nodes, self.root = partial_merkle_tree(cells) if cells else (np.zeros((0, 8), dtype=np.uint32), default_hashes()[0])
        self.map = {}
        for index, depth, left, right in self.nodes[:, :4].tolist():
            self.map[(depth, index)] = left
            self.map[(depth, index + 1)] = right
        self.present = {c[0] for c in cells}

    def node(self, depth, index):
        return self.map.get((depth, index), default_hashes()[depth])

    def opening(self, address, present=None):
        """the 34 words of cm_mem_opening for `address` (present: override the flag, for a cell the tree holds with zeros)"""
        a = int(address)
        held = a in self.present
        value = [self.node(HEIGHT, 4 * a + i) for i in range(4)] if held else [0, 0, 0, 0]
        sib = [self.node(28 - k, (a >> k) ^ 1) for k in range(N_SIBLINGS)]
        return [a, int(held) if present is None else int(present)] + value + sib

    def openings(self, addresses):
        return np.array([self.opening(a) for a in addresses], dtype=np.uint32).reshape(-1, WORDS)


def image_cells(lo, hi):
    """Run.memory() -> the cells of the image: locals dense from 0, heap index i = the cell at 2^28 - 1 - i"""
    cells = [(a,) + tuple(int(x) for x in lo[a]) for a in range(lo.shape[0])]
    cells += [(SPACE - 1 - i,) + tuple(int(x) for x in hi[i]) for i in range(hi.shape[0])]
    return cells


def check(root, w):
    """pure Python: is the record well formed and does it hash to `root`?"""
    w = [int(x) for x in w]
    a, present, v, sib = w[0], w[1], w[2:6], w[6:34]
    if a >= SPACE or present > 1 or any(x >= P for x in v + sib) or (present == 0 and any(v)):
        return False
    h = poseidon2_hash(poseidon2_hash(v[0], v[1]), poseidon2_hash(v[2], v[3]))
    for k in range(N_SIBLINGS):
        h = poseidon2_hash(sib[k], h) if (a >> k) & 1 else poseidon2_hash(h, sib[k])
    return h == int(root)


# ---- the memories and the single-record tampers the CPU and the GPU tests share ------------------------------------------------
def memories():
    return {
        "a": [(5, 11, 12, 13, 14)],
        "b": [(0, 1, 2, 3, 4), (SPACE - 1, 5, 6, 7, 8)],                       # full height, an all-default middle
        "c": [(0, 10, 0, 0, 0), (1, 11, 1, 0, 0), (2, 0, 0, 0, 0), (3, 13, 0, 3, 0), (7, 17, 0, 0, 7), (8, 18, 8, 8, 8),
              (1000, P - 1, 0, P - 1, 1)],                                     # cell 2 holds (0, 0, 0, 0) explicitly
    }


ZERO_CELL_OF_C = 2
ABSENT_NEAR = {"a": 4, "b": 1, "c": 6}                                          # an absent cell whose sibling is present
ABSENT_FAR = {"a": 1 << 20, "b": 1 << 27, "c": 123_456_789}                     # far from every present cell


def tampers(w, root, absent_w):
    """name -> (words, root): each is ONE change to a valid record — w, of a present cell, or absent_w, of an absent one"""
    out = {}

    def edit(name, pos, value):
        x = list(w)
        x[pos] = value
        out[name] = (x, root)

    for i in range(4):
        edit(f"value[{i}]", 2 + i, (w[2 + i] + 1) % P)
    edit("siblings[0]", 6, (w[6] + 1) % P)
    edit("siblings[27]", 33, (w[33] + 1) % P)
    edit("address neighbour", 0, w[0] ^ 1)
    edit("address bit 27", 0, w[0] ^ (1 << 27))
    out["root"] = (list(w), (root + 1) % P)
    edit("present = 2", 1, 2)
    edit("word = P", 6 + 13, P)
    x = list(absent_w)
    assert x[1] == 0 and x[2:6] == [0, 0, 0, 0]
    x[2] = 1
    out["absent with value[0] = 1"] = (x, root)
    return out
