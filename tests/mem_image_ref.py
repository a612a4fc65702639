"""Reference for followed memory (MemImage), independent of the code under test and built on tests/mem_open_ref.py (RefTree: the
pinned host tree builder plus cm_poseidon2_permute) and tests/mem_transition_ref.py: the node list an image must hold is RefTree
over every cell it then holds — a cell written to zero stays, with zeros — and only the words 0 .. 4 of a record (index, depth,
left, right, parent) are compared: the multiplicity words enter no hash and are unspecified."""
import numpy as np

from cairo_m_amd.lib import CmError, MemTransition
from tests.mem_open_ref import P, SPACE, RefTree, default_hashes
from tests.mem_set_ref import SETS, SET_IDS
from tests.mem_transition_ref import first_tree, reference, second_memory, second_tree

FORMS = ("full", "bare", "pair")


def words(nodes):
    """the contract words of a node list"""
    return np.asarray(nodes, dtype=np.uint32).reshape(-1, 8)[:, :5]


def tree_cells(tree):
    """(addresses, values (n, 4)) of a RefTree, ascending"""
    a = np.array([c[0] for c in tree.cells], dtype=np.uint32)
    v = np.array([c[1:] for c in tree.cells], dtype=np.uint32).reshape(-1, 4)
    return a, v


def assert_image_is(image, tree):
    """root, nodes and cells of `image` are those of the reference tree"""
    assert image.root == tree.root
    assert np.array_equal(words(image.nodes()), words(tree.nodes))
    a, v = image.cells()
    ra, rv = tree_cells(tree)
    assert np.array_equal(a, ra) and np.array_equal(v, rv)
    s = image.stats()
    assert s["n_cells"] == ra.size == image.n_cells and s["n_nodes"] == tree.nodes.shape[0]


def snapshot(image):
    a, v = image.cells()
    return image.root, image.nodes().tobytes(), a.tobytes(), v.tobytes()


def transition(i):
    r = reference(i)
    return MemTransition(r["a"], r["old"], r["new"], r["words"], r["root0"], r["root1"])


def apply_form(image, i, form, record=False):
    """the update of SETS[i] in one of its three forms"""
    t = transition(i)
    if form == "full":
        return image.apply_transition(t, record=record)
    if form == "bare":
        assert t.bare().siblings.size == 0 and t.bare().nbytes_bare == 20 * t.addresses.size
        return image.apply_transition(t.bare(), record=record)
    return image.apply(t.addresses, t.new_values, record=record)


def same_record(t, r):
    return (t.addresses.tolist() == r["a"] and t.siblings.tolist() == r["words"] and np.array_equal(t.old_values, r["old"])
            and np.array_equal(t.new_values, r["new"]) and (t.root_before, t.root_after) == (r["root0"], r["root1"]))


def refusals(i):
    """name -> (call on an image of first_tree, status, what the message must contain): each is ONE change to the valid update of
    SETS[i], which has at least two cells"""
    t = transition(i)
    a, old, new = t.addresses, t.old_values, t.new_values
    n = a.size
    assert n >= 2
    out = {}
    out["a wrong root before"] = (lambda im: im.apply(a, new, root_before=t.root_before ^ 1), 11,
                                  f"the image is at root {t.root_before}, the update starts from {t.root_before ^ 1}")
    off = old.copy()
    for cell in (n // 2, n - 1):                                                  # two cells off: the lowest is named
        off[cell, 1] = (int(off[cell, 1]) + 1) % P
    out["an old value word off"] = (lambda im: im.apply(a, new, old_values=off), 11,
                                    f"cell {int(a[n // 2])} holds ({', '.join(str(int(x)) for x in old[n // 2])}), the update's old value is")
    out["a wrong root after"] = (lambda im: im.apply(a, new, old_values=old, root_before=t.root_before, root_after=(t.root_after + 1) % P), 11,
                                 f"the image would hash to root {t.root_after}, not {(t.root_after + 1) % P}")
    big = new.copy()
    big[n - 1, 2] = P
    out["a new value word = P"] = (lambda im: im.apply(a, big), 11, f"new value word 2 of cell {int(a[-1])} is not below P")
    out["descending addresses"] = (lambda im: im.apply(a[::-1].copy(), new), 1, "address 1 is not above address 0")
    rep = a.copy()
    rep[n - 1] = rep[n - 2]
    out["a repeated address"] = (lambda im: im.apply(rep, new), 1, f"address {n - 1} is not above address {n - 2}")
    far = a.copy()
    far[n - 1] = SPACE
    out["an address at 2^28"] = (lambda im: im.apply(far, new), 1, f"address {n - 1} is beyond the address space of 2^28 cells")
    out["no cells, unequal roots"] = (lambda im: im.apply_transition(MemTransition([], [], [], [], t.root_before, t.root_after)), 11,
                                      f"no cell changes, and root {t.root_before} is not root {t.root_after}")
    out["no cells, another root"] = (lambda im: im.apply_transition(MemTransition([], [], [], [], t.root_after, t.root_after)), 11,
                                     f"the image is at root {t.root_before}, the update starts from {t.root_after}")
    return out


def assert_refused(image, call, status, needle):
    before = snapshot(image)
    try:
        call(image)
    except CmError as e:
        assert e.status == status and needle in e.message, (e.status, e.message)
    else:
        raise AssertionError("accepted")
    assert snapshot(image) == before


__all__ = ["P", "SPACE", "SETS", "SET_IDS", "FORMS", "RefTree", "default_hashes", "first_tree", "second_tree", "second_memory", "reference", "words",
           "tree_cells", "assert_image_is", "snapshot", "transition", "apply_form", "same_record", "refusals", "assert_refused"]
