"""What the CPU and the GPU tests of the program id share: the shapes, and two roots that owe nothing to the code under test — the
host restatement of build_partial_merkle_tree (lib.partial_merkle_tree, pinned by tests/test_adapter.py) and a plain-Python sparse
tree over mem_open_ref's KAT-pinned hash."""
import numpy as np

from cairo_m_amd.lib import partial_merkle_tree
from tests.mem_open_ref import HEIGHT, P, SPACE, default_hashes, poseidon2_hash


def field_values(n, seed):
    """n x 4 field words, full-width and small ones mixed, none of them an all-zero cell"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, P, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    v[::3, 1:] = 0                                       # instruction-like cells: one opcode word, small operands
    v[:, 0] |= 1
    v[v >= P] = P - 1
    return v


def shapes():
    """[(name, start, values n x 4, small)]: `small` ones are also held to the plain-Python tree"""
    out = [
        ("one cell at 0", 0, field_values(1, 1), True),
        ("one cell at 5", 5, np.array([[1, 2, 3, 4]], dtype=np.uint32), True),                  # test_single_element_tree
        ("cells 0 and 1", 0, np.array([[10, 11, 12, 13], [20, 21, 22, 23]], dtype=np.uint32), True),  # test_multiple_elements_tree
        ("start 3, n 4", 3, field_values(4, 2), True),                                               # both ends need a default at depth 28
        ("n 3", 0, field_values(3, 3), True),
        ("across the middle", (1 << 27) - 1, field_values(2, 4), True),                              # two nodes wide up to depth 1
        ("the last cells", SPACE - 2, field_values(2, 5), True),
        ("n 1024", 1, field_values(1024, 6), False),                                                 # either side of the LDS level's width
        ("n 1025", 1, field_values(1025, 7), False),
        ("n 2049", 1, field_values(2049, 8), False),
    ]
    return out


def cells_of(start, values):
    return [(int(start) + i,) + tuple(int(x) for x in row) for i, row in enumerate(np.asarray(values).reshape(-1, 4))]


def tree_root(start, values):
    """the yardstick: build_partial_merkle_tree over exactly these cells, no public ranges"""
    return partial_merkle_tree(cells_of(start, values), initial=True, ranges=(0,) * 6)[1]


def python_root(cells):
    """plain Python: the sparse tree of height 30 over the leaves 4 a + i, a missing node being the default of its depth"""
    level = {4 * a + i: int(v[i]) for a, *v in cells for i in range(4)}
    dflt = default_hashes()
    for depth in range(HEIGHT, 0, -1):
        up = {}
        for index in sorted({i >> 1 for i in level}):
            up[index] = poseidon2_hash(level.get(2 * index, dflt[depth]), level.get(2 * index + 1, dflt[depth]))
        level = up
    return level[0]


def image_values(program):
    """the memory image of a program (a list of instruction word lists): every instruction takes whole cells, four words each, the
    last one padded with zeros (crates/runner/src/vm/mod.rs:75-101) -> n x 4"""
    rows = []
    for ins in program:
        for i in range(0, len(ins), 4):
            chunk = [int(x) for x in ins[i:i + 4]]
            rows.append(chunk + [0] * (4 - len(chunk)))
    return np.array(rows, dtype=np.uint32).reshape(-1, 4)


def casm_programs():
    """[(name, values n x 4)]: the 122 compiler-emitted programs, instructions and data behind them, as the image from address 0"""
    from tests.casm_fixtures import load
    out = []
    for fx in load():
        out.append((fx["name"], image_values(fx["instructions"] + fx.get("data", []))))
    return out
