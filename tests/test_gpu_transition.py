"""Memory transitions on the GPU (cm_input_write_set, cm_input_open_transition, cm_verify_memory_transition,
cm_prove_run_transitions) against tests/mem_transition_ref.py: two trees of the pinned host builder that differ in exactly one
set's cells, the words and values read off their node records from Python — never the code under test.

The pairs of trees reach the device as the initial and final tree of an uploaded input (cm_input_upload), as the set test's do;
such inputs carry no boundary memory, so they are opened with the set's addresses given.  The write set (addresses = NULL,
cm_input_write_set) is checked on an adapted scatter-store segment under both tree builders against the numpy diff of its own
downloaded rows (tests/link_diff_ref.py), and on the two-segment heap run, whose followed updates rebuild the final image."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, MemTransition, Run, follow_run, prover_input_arrays, verify_transition,
                             verify_transition_host, vm_segment)
from tests.link_diff_ref import link_diff_ref
from tests.mem_open_ref import image_cells
from tests.mem_set_ref import SET_IDS, SETS, SPACE, RefTree, ref_set
from tests.mem_transition_ref import P, first_tree, reference, second_tree, tampers
from tests.test_gpu_adapter import scatter_store_program
from tests.test_gpu_mem_open import _heap_run

pytestmark = pytest.mark.gpu


def _upload(backend, before, after):
    ai = ArrayInput({"initial_tree": before.nodes, "final_tree": after.nodes, "roots": [before.root, after.root]})
    return backend.upload_input(ai), ai


@pytest.fixture(scope="module")
def uploaded(backend):
    """i -> the device input whose initial tree is SETS[i]'s memory and whose final tree is that memory after the set was written"""
    out = [_upload(backend, first_tree(name), second_tree(i)) for i, (name, _) in enumerate(SETS)]
    yield [dev for dev, _ in out]
    for dev, _ in out:
        backend.free_input(dev)


def _equals(t, r):
    assert t.addresses.tolist() == r["a"] and t.siblings.tolist() == r["words"]
    assert np.array_equal(t.old_values, r["old"]) and np.array_equal(t.new_values, r["new"])
    assert (t.root_before, t.root_after) == (r["root0"], r["root1"])
    assert t.nbytes == 36 * len(r["a"]) + 4 * len(r["words"])


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_transitions_of_uploaded_trees_equal_the_reference(backend, uploaded, i):
    r = reference(i)
    t = backend.open_transition(uploaded[i], r["a"])
    _equals(t, r)
    assert t.n_zero_only == 0                                                     # (no boundary memory: nothing to diff)
    again = backend.open_transition(uploaded[i], r["a"][::-1] + r["a"][:1])       # any order, any repeats: the same bytes
    for f in ("addresses", "old_values", "new_values", "siblings"):
        assert getattr(again, f).tobytes() == getattr(t, f).tobytes(), f
    assert verify_transition(t, backend.L, with_roots=True) == (True, (r["root0"], r["root1"]))
    assert verify_transition_host(t, backend.L) == (0, "")


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_each_tamper_is_a_verdict_of_the_gpu_and_of_the_host(backend, i):
    r = reference(i)
    for what, (a, old, new, w, r0, r1, needle, still) in tampers(r).items():
        t = MemTransition(a, old, new, w, r0, r1)
        gpu, got = verify_transition(t, backend.L, with_roots=True)               # status 0: a verdict, never a failure
        rc, msg = verify_transition_host(t, backend.L)
        assert gpu is False and rc == 11 and needle in msg, (what, gpu, rc, msg)
        if still is None and what != "a sibling + 1":
            assert got == (0, 0), what                                            # malformed: no roots
        if still == "both":
            assert got == (r["root0"], r["root1"]), what                          # well formed: it folds to the true roots
        if still == "new":
            assert got[1] == r["root1"] and got[0] != r["root0"], what            # the old side alone is off
        if still == "old":
            assert got[0] == r["root0"] and got[1] != r["root1"], what
        if what == "a sibling + 1":
            assert got[0] != r["root0"] and got[1] != r["root1"] and 0 not in got, what


def test_no_cells_and_status_1(backend):
    L = backend.L
    none = np.zeros((0, 4), dtype=np.uint32)
    assert verify_transition(MemTransition([], none, none, [], 7, 7), L, with_roots=True) == (True, (7, 7))
    assert verify_transition(MemTransition([], none, none, [], 7, 8), L, with_roots=True) == (False, (7, 7))
    assert verify_transition(MemTransition([], none, none, [1], 7, 7), L, with_roots=True) == (False, (0, 0))
    one, words, ok = (C.c_uint32 * 4)(5), (C.c_uint32 * 28)(), C.c_uint8(7)

    def call(a=one, n=1, old=one, new=one, sib=words, okp=C.byref(ok)):
        return L.cm_verify_memory_transition(C.c_uint32(0), C.c_uint32(0), a, C.c_uint64(n), old, new, sib, C.c_uint32(28), okp, None, C.c_uint64(0))

    for kw in (dict(a=None), dict(old=None), dict(new=None), dict(sib=None), dict(okp=None), dict(n=(1 << 20) + 1)):
        assert call(**kw) == 1 and ok.value == 7, kw
    assert call() == 0 and ok.value == 0                                          # zeros under root 0: a verdict


def _spread():
    """257 distinct addresses all over the address space, the two ends among them, and a memory that holds every other one"""
    rng = np.random.default_rng(20241020)
    a = sorted({0, SPACE - 1} | {int(x) & ~1 for x in rng.integers(2, SPACE - 2, 300)})[:256] + [SPACE - 1]
    a = sorted(set(a))
    assert len(a) == 257 and a[0] == 0 and a[-1] == SPACE - 1 and all(x ^ 1 not in a for x in a[1:-1])
    cells = [(x,) + tuple(int(w) for w in rng.integers(0, P, 4)) for x in a[::2]]
    return a, cells


def test_the_smallest_shapes(backend):
    a, cells = _spread()
    before = RefTree(cells)
    shapes = [[a[4]], [a[5]], [a[6], a[6] ^ 1], [0, SPACE - 1], a[:129], a]       # a held cell, an absent one, a pair without a word at depth 28
    live = None
    for j, s in enumerate(shapes):
        held = {c[0]: c[1:] for c in cells}
        held.update({x: (j + 1, x % P, P - 1, 1 + k) for k, x in enumerate(s)})
        after = RefTree([(x,) + tuple(v) for x, v in held.items()])
        words, old, counts = ref_set(before, s)
        words_after, new, _ = ref_set(after, s)
        assert words == words_after and before.root != after.root
        if len(s) == 2 and s[1] == s[0] ^ 1:
            assert counts[0] == 0 and len(words) == 27
        dev, _ = _upload(backend, before, after)
        t = backend.open_transition(dev, s)
        _equals(t, {"a": s, "old": old, "new": new, "words": words, "root0": before.root, "root1": after.root})
        assert verify_transition(t, backend.L, with_roots=True) == (True, (before.root, after.root))
        assert verify_transition_host(t, backend.L) == (0, "")
        moved = MemTransition(t.addresses, t.new_values, t.old_values, t.siblings, t.root_before, t.root_after)
        assert verify_transition(moved, backend.L, with_roots=True) == (False, (after.root, before.root))
        backend.free_input(dev)
        if live is None:
            live = backend.mem_stats().live_bytes
        assert backend.mem_stats().live_bytes == live                             # every buffer of the calls went back to the pool


def test_refusals_of_the_opener(backend, uploaded):
    dev = uploaded[2]                                                             # ("a", [4, 6])
    for addresses, needle in (([], "no cells"), ([5, SPACE], "address 1 is beyond the address space")):
        with pytest.raises(CmError) as e:
            backend.open_transition(dev, addresses)
        assert "status 1:" in str(e.value) and needle in str(e.value), str(e.value)
    L, h = backend.L, C.c_void_p()
    two = (C.c_uint32 * 2)(6, 4)
    assert L.cm_input_open_transition(dev, two, C.c_uint64(2), C.byref(h)) == 1 and not h.value          # not ascending
    assert L.cm_input_open_transition(dev, two, C.c_uint64((1 << 20) + 1), C.byref(h)) == 1 and not h.value
    assert L.cm_input_open_transition(None, two, C.c_uint64(1), C.byref(h)) == 1
    assert L.cm_input_open_transition(dev, two, C.c_uint64(1), None) == 1
    # trees alone: the write set is empty, and so is the transition over it
    a, total, zero_only = backend.write_set(dev, with_counts=True)
    assert (a.size, total, zero_only) == (0, 0, 0)
    t = backend.open_transition(dev)
    assert t.addresses.size == 0 and t.siblings.size == 0 and (t.root_before, t.root_after) == (reference(2)["root0"], reference(2)["root1"])
    assert verify_transition(t, L) is False                                       # no cell changes, and the roots differ


@pytest.mark.parametrize("device_trees", [False, True])
def test_write_set_and_transition_of_an_adapted_segment_under_both_tree_builders(backend, monkeypatch, device_trees):
    """300 cells: below the 2048-row cut-over the adapter hashes its trees on the host; CM_ADAPTER_DEVICE_TREE_MIN=1 sends them
    through the device builder.  The write set is the numpy diff of the input's own downloaded rows."""
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    hs = vm_segment(scatter_store_program(300))
    dev = backend.adapt_segment(hs)
    hi = backend.download_input(dev)
    rows = prover_input_arrays(hi.view)
    cells, totals = link_diff_ref(rows["initial_memory"], rows["final_memory"])
    want = cells[:, 1].tolist()
    assert len(want) >= 4                                                         # (the loop's own variables: a store to a fresh cell changes nothing)
    got, total, zero_only = backend.write_set(dev, with_counts=True)
    assert got.tolist() == want and total == len(want) and zero_only == totals["n_zero_only"]
    few, total, _ = backend.write_set(dev, cap=7, with_counts=True)               # truncated, not an error
    assert few.tolist() == want[:7] and total == len(want)
    refs = [RefTree([tuple(int(x) for x in r[:5]) for r in rows[key]]) for key in ("initial_memory", "final_memory")]
    assert [t.root for t in refs] == [int(x) for x in rows["roots"]]              # the reference trees ARE the input's trees
    words, old, _ = ref_set(refs[0], want)
    _, new, _ = ref_set(refs[1], want)
    t = backend.open_transition(dev)
    _equals(t, {"a": want, "old": old, "new": new, "words": words, "root0": refs[0].root, "root1": refs[1].root})
    assert t.n_zero_only == totals["n_zero_only"]
    assert verify_transition(t, backend.L, with_roots=True) == (True, (refs[0].root, refs[1].root))
    assert backend.open_transition(dev).siblings.tobytes() == t.siblings.tobytes()
    # a supplied set must hold every changed cell; the lowest one missing is named
    drop = [want[1], want[3]]
    with pytest.raises(CmError) as e:
        backend.open_transition(dev, [x for x in want if x not in drop])
    assert "status 1:" in str(e.value) and f"cell {drop[0]} changes in this segment and is not in the set" in str(e.value), str(e.value)
    untouched = [want[-1] + 2, 1 << 27, SPACE - 1]
    assert not set(untouched) & set(want)
    big = backend.open_transition(dev, want + untouched)                          # a superset rides along
    assert big.addresses.tolist() == sorted(want + untouched) and big.n_zero_only == totals["n_zero_only"]
    ride = [big.addresses.tolist().index(x) for x in untouched]
    assert np.array_equal(big.old_values[ride], big.new_values[ride])
    assert verify_transition(big, backend.L) and verify_transition_host(big, backend.L) == (0, "")
    backend.free_input(dev)
    hi.free(); hs.free()


def test_a_followed_run_rebuilds_the_final_image(backend):
    """The starting image is the memory under proof 0's initial_root: segment 0's initial boundary rows, downloaded from a run of
    their own.  That is Run.memory() before the first segment plus the cells the segment first writes, which the adapter (as the
    reference's) commits to in the INITIAL tree with the value of their first access — they are no change between the two roots
    and so are in no transition; a follower that starts from the proved initial_root holds them already."""
    hss = _heap_run()
    plain = Run.from_segment(backend, hss[0])
    want = [p.words().copy() for p in plain.prove(hss)]
    plain.free()
    first = Run.from_segment(backend, hss[0])
    lo, hp = first.memory()
    dev0 = first.adapt_next(hss[0])
    hi0 = backend.download_input(dev0)
    rows = prover_input_arrays(hi0.view)
    image = {int(r[0]): tuple(int(x) for x in r[1:5]) for r in rows["initial_memory"]}
    assert RefTree([(a,) + v for a, v in image.items()]).root == int(rows["roots"][0])
    assert all(image[c[0]] == tuple(c[1:]) for c in image_cells(lo, hp))          # Run.memory() at the start is part of it
    backend.free_input(dev0)
    hi0.free()
    first.free()
    run = Run.from_segment(backend, hss[0])
    proofs, moves = run.prove(hss, transitions=True)
    assert proofs[0].public_data()["initial_root"] == int(rows["roots"][0])
    assert len(proofs) == len(moves) == 2 and all(m is not None for m in moves)
    for p, w in zip(proofs, want):
        assert np.array_equal(p.words(), w)                                       # the proofs are cm_prove_run's
    for device in (True, False):
        updates = follow_run(proofs, moves, backend.L, device=device)
    assert len(updates) == sum(m.addresses.size for m in moves) > 0
    for a, v in updates:
        image[a] = v
    lo, hp = run.memory()
    final = {c[0]: tuple(c[1:]) for c in image_cells(lo, hp)}
    zero = (0, 0, 0, 0)
    assert all(image.get(a, zero) == final.get(a, zero) for a in set(image) | set(final))
    assert moves[1].root_before == moves[0].root_after
    with pytest.raises(CmError) as e:
        follow_run(proofs, moves[::-1], backend.L)
    assert "segment 0" in str(e.value), str(e.value)
    bent = MemTransition(moves[1].addresses, moves[1].old_values, moves[1].new_values + np.uint32(1), moves[1].siblings,
                         moves[1].root_before, moves[1].root_after)
    with pytest.raises(CmError) as e:
        follow_run(proofs, [moves[0], bent], backend.L)
    assert "segment 1" in str(e.value), str(e.value)
    for p in proofs:
        p.free()
    run.free()
    for hs in hss:
        hs.free()
