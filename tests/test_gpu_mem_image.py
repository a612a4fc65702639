"""Followed memory on the GPU (cm_mem_image_*, device = 1): the update kernels of mem_image.hip against the reference trees of
tests/mem_image_ref.py for every entry of SETS, byte-equal to the host image; the refusals with the host path's statuses and
messages; the three openers over a merged node list; the re-emitted record; a real two-segment run followed from its bare
transitions; the pool's accounting."""
import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemImage, MemTransition, Run, follow_run_image, mem_set_plan, mem_stats, prover_input_arrays, verify_openings,
                             verify_range, verify_set, verify_transition)
from tests.mem_image_ref import (FORMS, SET_IDS, SETS, SPACE, RefTree, apply_form, assert_image_is, assert_refused, default_hashes, first_tree, reference,
                                 refusals, same_record, second_tree, snapshot, tree_cells)
from tests.mem_open_ref import memories
from tests.mem_range_ref import ref_range
from tests.mem_set_ref import ref_set

pytestmark = pytest.mark.gpu
MULTI = 6                                                                         # SETS[6]: seven cells of memory "c", a held zero cell among them


def images(backend, cells):
    """the same cells on the device and in host memory"""
    return MemImage.from_cells(cells, backend.L, device=True), MemImage.from_cells(cells, backend.L, device=False)


def test_the_updates_cross_both_hashing_kernels():
    kernels = [{s["kernel"] for s in mem_set_plan(a)[0][1:]} for _, a in SETS]
    assert any("level" in k for k in kernels) and any(k == {"tail"} for k in kernels)
    assert max(sum(1 for s in mem_set_plan(a)[0] if s["kernel"] == "level") for _, a in SETS) == 6
    # held cells only (every record replaces one) and created cells (records are inserted): both shapes of the merge
    created = [bool(set(a) - {c[0] for c in first_tree(name).cells}) for name, a in SETS]
    assert any(created) and not all(created)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_apply_gives_the_reference_tree_and_the_host_image(backend, i, form):
    name, a = SETS[i]
    r = reference(i)
    dev, host = images(backend, first_tree(name).cells)
    try:
        assert_image_is(dev, first_tree(name))
        assert snapshot(dev) == snapshot(host)
        assert apply_form(dev, i, form) == r["root1"] == apply_form(host, i, form)
        assert_image_is(dev, second_tree(i))
        assert snapshot(dev) == snapshot(host)
        assert np.array_equal(dev.read(a[::-1]), r["new"][::-1])
    finally:
        dev.free()
        host.free()


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_record_is_the_reference_transition(backend, i):
    dev = MemImage.from_cells(first_tree(SETS[i][0]).cells, backend.L)
    try:
        root, t = apply_form(dev, i, "pair", record=True)
        assert root == reference(i)["root1"] and same_record(t, reference(i))
        assert verify_transition(t, backend.L)
        assert_image_is(dev, second_tree(i))
    finally:
        dev.free()


@pytest.mark.parametrize("what", list(refusals(MULTI)))
def test_refusals_are_the_host_paths_and_leave_the_image_as_it_was(backend, what):
    call, status, needle = refusals(MULTI)[what]
    dev, host = images(backend, first_tree(SETS[MULTI][0]).cells)
    try:
        assert_refused(dev, call, status, needle)
        said = []
        for im in (dev, host):
            with pytest.raises(CmError) as e:
                call(im)
            said.append((e.value.status, e.value.message))
        assert said[0] == said[1]
        apply_form(dev, MULTI, "full")
        assert_image_is(dev, second_tree(MULTI))
    finally:
        dev.free()
        host.free()


def test_the_empty_image(backend):
    dev = MemImage.from_cells([], backend.L)
    try:
        assert dev.root == default_hashes()[0] and dev.n_cells == 0 and dev.nodes().shape == (0, 8)
        assert not dev.read([3, 3, 0]).any()
        for call in (lambda: dev.open([5]), lambda: dev.open_range(0, 2), lambda: dev.open_set([5])):
            with pytest.raises(CmError) as e:
                call()
            assert "status 1:" in str(e.value) and "the image is empty" in str(e.value)
        tree = first_tree("dense")
        a, v = tree_cells(tree)
        assert dev.apply(a, v, old_values=np.zeros_like(v), root_before=default_hashes()[0], root_after=tree.root) == tree.root
        assert_image_is(dev, tree)
    finally:
        dev.free()


def test_openings_over_a_merged_list(backend):
    """memory "b" — the two ends of the address space — written into the image of memory "a": records inserted at both ends of
    every depth's slice.  What the three openers then bisect is the merged list."""
    m = memories()
    tree = RefTree(m["a"] + m["b"])
    dev = MemImage.from_cells(m["a"], backend.L)
    try:
        assert dev.apply([c[0] for c in m["b"]], [c[1:] for c in m["b"]]) == tree.root
        assert_image_is(dev, tree)
        addrs = [SPACE - 1, 0, 5, 4, 1 << 27, 5]
        got, root = dev.open(addrs)
        assert root == tree.root and np.array_equal(np.array([o.words() for o in got], dtype=np.uint32), tree.openings(addrs))
        assert all(verify_openings(root, got, backend.L))
        for start, n in ((0, 8), (SPACE - 3, 3)):
            rec, values, root = dev.open_range(start, n)
            want, want_values = ref_range(tree, start, n)
            assert root == tree.root and rec.words() == want and np.array_equal(values, want_values)
            assert verify_range(root, rec, values, backend.L)
        s = [0, 4, 5, 6, 1 << 20, SPACE - 2, SPACE - 1]
        opening, root = dev.open_set(s)
        w, v, counts = ref_set(tree, s)
        assert root == tree.root and opening.siblings.tolist() == w and np.array_equal(opening.values, v) and opening.counts == counts
        assert verify_set(root, opening, backend.L)
    finally:
        dev.free()


def test_a_followed_run(backend):
    """The two-segment heap run, followed from its bare transitions.  The starting image is the memory under proof 0's
    initial_root — segment 0's initial boundary rows — as in tests/test_gpu_transition.py's follow test, which says why."""
    from tests.test_gpu_mem_open import _heap_run
    hss = _heap_run()
    first = Run.from_segment(backend, hss[0])
    dev0 = first.adapt_next(hss[0])
    hi0 = backend.download_input(dev0)
    rows = prover_input_arrays(hi0.view)
    cells = [(int(r[0]),) + tuple(int(x) for x in r[1:5]) for r in rows["initial_memory"]]
    root0 = int(rows["roots"][0])
    backend.free_input(dev0)
    hi0.free()
    first.free()
    run = Run.from_segment(backend, hss[0])
    proofs, moves = run.prove(hss, transitions=True)
    image = MemImage.from_cells(cells, backend.L)
    try:
        assert image.root == root0 == proofs[0].public_data()["initial_root"]
        bare = [m.bare() for m in moves]
        assert all(b.siblings.size == 0 for b in bare) and moves[1].addresses.size > 0
        bent = MemTransition(bare[1].addresses, bare[1].old_values, bare[1].new_values.copy(), [], bare[1].root_before, bare[1].root_after)
        bent.new_values[0, 0] ^= 1
        with pytest.raises(CmError) as e:
            follow_run_image(proofs, [bare[0], bent], image)
        assert "segment 1" in str(e.value) and "would hash to root" in str(e.value)
        assert image.root == proofs[0].public_data()["final_root"]               # the image stays at the last good segment
        with pytest.raises(CmError) as e:
            follow_run_image(proofs, bare, image)                                 # and segment 0 does not apply twice
        assert "segment 0" in str(e.value)
        assert follow_run_image(proofs[1:], [(bare[1].addresses, bare[1].new_values)], image) == proofs[-1].public_data()["final_root"]
        last = moves[1].addresses
        got, root = image.open_set(last)
        want, want_root = run.open_set(last)
        assert root == want_root == proofs[-1].public_data()["final_root"]
        assert got.siblings.tobytes() == want.siblings.tobytes() and got.values.tobytes() == want.values.tobytes()
        assert np.array_equal(got.values, moves[1].new_values)
    finally:
        image.free()
        for p in proofs:
            p.free()
        run.free()
        for hs in hss:
            hs.free()


def test_the_pool_counts_the_image_while_it_lives(backend):
    tree = first_tree("dense")
    before = mem_stats(backend.L).live_bytes
    dev = MemImage.from_cells(tree.cells, backend.L)
    # (the pool hands out a cached block that wastes at most a quarter: the handle's own figure is the rounded request)
    held = dev.stats()["bytes"]
    assert held >= 32 * tree.nodes.shape[0] and before + held <= mem_stats(backend.L).live_bytes <= before + held + held // 4
    apply_form(dev, 9, "bare")                                                    # the 1 500 random cells: the handle swaps buffers
    held = dev.stats()["bytes"]
    assert before + held <= mem_stats(backend.L).live_bytes <= before + held + held // 4
    dev.free()
    assert mem_stats(backend.L).live_bytes == before
