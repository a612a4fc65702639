"""cm_verify_memory_opening, the host verifier of a light client, against the pinned host tree builder: the openings
tests/mem_open_ref.py reads off cm_adapter_partial_tree's node records are accepted under the builder's root, and every
single-field change of a record is refused with status 11 and a message that names the address.  CPU only."""
import pytest

from cairo_m_amd.lib import MemOpening, verify_opening
from tests.mem_open_ref import (ABSENT_FAR, ABSENT_NEAR, P, ZERO_CELL_OF_C, RefTree, check, default_hashes, memories, poseidon2_hash,
                                tampers)

NAMES = ["a", "b", "c"]


@pytest.fixture(scope="module")
def trees():
    return {name: RefTree(cells) for name, cells in memories().items()}


def _accepts(root, words):
    rc, msg = verify_opening(root, MemOpening.from_words(words))
    assert (rc == 0) == check(root, words), (rc, msg)                            # the pure-Python recomputation agrees
    return rc, msg


def test_reference_is_self_consistent(trees):
    """the map's top pair hashes to the builder's root; an empty memory's root is the default of depth 0"""
    for name, t in trees.items():
        assert poseidon2_hash(t.node(1, 0), t.node(1, 1)) == t.root, name
    assert RefTree([]).root == default_hashes()[0]
    assert poseidon2_hash(0, 0) == default_hashes()[29]                          # why an absent cell and a zero cell hash alike


@pytest.mark.parametrize("name", NAMES)
def test_openings_of_the_reference_are_accepted(trees, name):
    t = trees[name]
    for cell in t.cells:
        w = t.opening(cell[0])
        assert w[1] == 1 and w[2:6] == list(cell[1:])
        assert _accepts(t.root, w) == (0, ""), cell
    for a in (ABSENT_NEAR[name], ABSENT_FAR[name]):
        w = t.opening(a)
        assert w[1] == 0 and w[2:6] == [0, 0, 0, 0] and a not in t.present
        assert _accepts(t.root, w) == (0, ""), a
    near = t.opening(ABSENT_NEAR[name])
    assert near[6] != default_hashes()[28] and (ABSENT_NEAR[name] ^ 1) in t.present   # its sibling is a present cell
    far = t.opening(ABSENT_FAR[name])
    assert far[6:6 + 8] == default_hashes()[28:20:-1]                            # nothing but empty subtrees near it


def test_a_present_zero_cell_opens_as_present_and_as_absent(trees):
    t = trees["c"]
    assert ZERO_CELL_OF_C in t.present
    for present in (1, 0):
        w = t.opening(ZERO_CELL_OF_C, present=present)
        assert w[1] == present and w[2:6] == [0, 0, 0, 0]
        assert _accepts(t.root, w) == (0, "")


@pytest.mark.parametrize("name", NAMES)
def test_every_single_change_is_refused(trees, name):
    t = trees[name]
    cell = t.cells[-1]
    w, absent_w = t.opening(cell[0]), t.opening(ABSENT_NEAR[name])
    cases = tampers(w, t.root, absent_w)
    assert len(cases) == 12
    for what, (x, root) in cases.items():
        rc, msg = _accepts(root, x)
        assert rc == 11, what
        assert msg.startswith(f"memory opening of address {x[0]}: "), (what, msg)
    # what the message says beyond the address
    msg = {k: verify_opening(r, MemOpening.from_words(x))[1] for k, (x, r) in cases.items()}
    assert msg["root"].endswith(f"the path hashes to root {t.root}, not {(t.root + 1) % P}")
    assert "present is 2" in msg["present = 2"]
    assert "the sibling at depth 15 is not below P" in msg["word = P"]          # siblings[13] = depth 28 - 13
    assert "absent cell with a non-zero value" in msg["absent with value[0] = 1"]
    for k in ("value[0]", "value[3]", "siblings[0]", "siblings[27]", "address neighbour", "address bit 27"):
        assert "the path hashes to root" in msg[k], k
