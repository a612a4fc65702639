"""Batched image updates on the GPU (cm_mem_images_apply, mem_image_batch.inc): all twelve SETS in one call against the reference
trees of tests/mem_image_ref.py and byte-equal to the loop of single calls; every refusal the single call can express in the
middle of applied neighbours, in the single call's words; the empty image, a host image and one image twice as parts; two runs
followed round by round; the pool's accounting; and the launch count, which does not depend on the number of parts."""
import ctypes as C
import json

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemImage, MemTransition, Run, apply_images, follow_run_image, follow_runs_images, mem_batch_launches,
                             mem_batch_plan, mem_stats, prover_input_arrays)
from tests.mem_image_ref import (SETS, assert_image_is, default_hashes, first_tree, reference, refusals, second_tree, snapshot, transition, tree_cells)

MIXED = 6                                                                         # SETS[6]: seven cells of memory "c", held and absent ones mixed
LEFT, RIGHT = 1, 8                                                                # the neighbours: two cells of "a"; the 1 667-cell dense set
NEW_KERNELS = ("k_imgs_check", "k_imgs_cells", "k_imgs_level", "k_imgs_tail", "k_imgs_rank", "k_imgs_merge", "k_imgs_offsets")


def image_of(backend, i):
    return MemImage.from_cells(first_tree(SETS[i][0]).cells, backend.L)


def full(i):
    """update i with everything the call can check"""
    t = transition(i)
    return t.addresses, t.new_values, t.old_values, t.root_before, t.root_after


def last_error(L):
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    return buf.value.decode()


class Recorder:
    """stands in for an image in the calls of refusals(): keeps the arguments of MemImage.apply, or None for a call the batch
    cannot express (apply_transition without cells)"""

    def __init__(self):
        self.args = None

    def apply(self, addresses, new_values, old_values=None, root_before=None, root_after=None):
        self.args = (addresses, new_values, old_values, root_before, root_after)

    def apply_transition(self, t):
        assert t.addresses.size == 0


def expressible():
    out = {}
    for what, (call, status, needle) in refusals(MIXED).items():
        rec = Recorder()
        call(rec)
        if rec.args is not None:
            out[what] = (rec.args, status, needle)
    return out


# ---- the reference side, checked without a GPU --------------------------------------------------------------------------------
def test_the_fixtures_stand_on_their_own():
    """RefTree, reference(i) and the refusals as the GPU tests use them: a failure there is then the feature's"""
    for i, (name, a) in enumerate(SETS):
        r, t = reference(i), transition(i)
        assert t.addresses.tolist() == list(a) == r["a"] and t.new_values.shape == (len(a), 4)
        assert first_tree(name).root == r["root0"] and second_tree(i).root == r["root1"]
        ra, rv = tree_cells(second_tree(i))
        assert set(a) <= set(ra.tolist())
    ex = expressible()
    assert len(ex) == len(refusals(MIXED)) - 2 == 7 and {s for _, s, _ in ex.values()} == {1, 11}
    widths = [len(a) for _, a in SETS]
    assert max(widths) == len(SETS[RIGHT][1]) == 1667 and min(widths) == 1
    # dense parts reach the per-level launches, narrow ones only ride along; some parts insert cells, some only replace
    plan = mem_batch_plan([a for _, a in SETS])
    assert mem_batch_launches(plan) == 1 + 6 + 1
    created = [bool(set(a) - {c[0] for c in first_tree(name).cells}) for name, a in SETS]
    assert any(created) and not all(created)


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_twelve_sets_in_one_call_and_against_the_loop(backend):
    """(the looped twin of an image lives only while it is compared: the suite's memory tests hold the driver's free bytes against the
    pool's, and device memory in small blocks that a test held all at once stays with the driver's allocator after a trim)"""
    n = len(SETS)
    batch = [image_of(backend, i) for i in range(n)]
    try:
        rc, got = apply_images([(batch[i],) + full(i) for i in range(n)], with_rc=True)
        assert rc == 0 and got == [(0, reference(i)["root1"], "") for i in range(n)]
        after = []
        for i in range(n):
            assert_image_is(batch[i], second_tree(i))
            after.append((batch[i].nodes().tobytes(), batch[i].cells(), batch[i].stats()))
        # the bare form (addresses and new values alone) on a second round: back to the first memory, a second batch on the same images
        back = [(batch[i], reference(i)["a"], reference(i)["old"]) for i in range(n)]
        assert [s for s, _, _ in apply_images(back)] == [0] * n
        for i in range(n):
            twin = image_of(backend, i)
            try:
                assert twin.apply(*full(i)) == reference(i)["root1"]
                nodes, cells, stats = after[i]
                assert nodes == twin.nodes().tobytes()                            # every word, not only the contract's
                assert all(x.tobytes() == y.tobytes() for x, y in zip(cells, twin.cells())) and stats == twin.stats()
                twin.apply(reference(i)["a"], reference(i)["old"])
                assert batch[i].root == reference(i)["root0"] and snapshot(batch[i]) == snapshot(twin)
            finally:
                twin.free()
    finally:
        for im in batch:
            im.free()


@pytest.mark.gpu
@pytest.mark.parametrize("what", list(expressible()))
def test_one_refusal_among_applied_neighbours(backend, what):
    args, status, needle = expressible()[what]
    ims = [image_of(backend, LEFT), image_of(backend, MIXED), image_of(backend, RIGHT)]
    alone = image_of(backend, MIXED)
    try:
        before = snapshot(ims[1])
        rc, got = apply_images([(ims[0],) + full(LEFT), (ims[1],) + args, (ims[2],) + full(RIGHT)], with_rc=True)
        said = last_error(backend.L)
        assert [g[0] for g in got] == [0, status, 0] and needle in got[1][2], got
        assert rc == status and said == "part 1: " + got[1][2]
        assert snapshot(ims[1]) == before and got[1][1] == before[0]
        with pytest.raises(CmError) as e:                                         # the single call's own status and message
            alone.apply(*args)
        assert (e.value.status, e.value.message) == (got[1][0], got[1][2])
        assert_image_is(ims[0], second_tree(LEFT))
        assert_image_is(ims[2], second_tree(RIGHT))
        assert (got[0][1], got[2][1]) == (reference(LEFT)["root1"], reference(RIGHT)["root1"])
        assert apply_images([(ims[1],) + full(MIXED)]) == [(0, reference(MIXED)["root1"], "")]   # and the image still takes the valid update
        assert_image_is(ims[1], second_tree(MIXED))
    finally:
        for im in ims + [alone]:
            im.free()


@pytest.mark.gpu
def test_two_refusals_name_the_lowest(backend):
    ex = expressible()
    ims = [image_of(backend, MIXED), image_of(backend, LEFT), image_of(backend, MIXED)]
    try:
        rc, got = apply_images([(ims[0],) + ex["a wrong root after"][0], (ims[1],) + full(LEFT), (ims[2],) + ex["a repeated address"][0]], with_rc=True)
        assert [g[0] for g in got] == [11, 0, 1] and rc == 11 and last_error(backend.L).startswith("part 0: memory image: the image would hash to root")
        rc, got = apply_images([(ims[2],) + ex["a repeated address"][0], (ims[0],) + ex["an old value word off"][0]], with_rc=True)
        assert [g[0] for g in got] == [1, 11] and rc == 1 and last_error(backend.L).startswith("part 0: cm_mem_image_apply: ")
        assert_image_is(ims[0], first_tree(SETS[MIXED][0]))
    finally:
        for im in ims:
            im.free()


@pytest.mark.gpu
def test_an_empty_image_a_host_image_and_one_image_twice(backend):
    tree = first_tree("c")
    a, v = tree_cells(tree)
    empty, other = MemImage.from_cells([], backend.L), image_of(backend, LEFT)
    host = MemImage.from_cells(first_tree(SETS[MIXED][0]).cells, backend.L, device=False)
    try:
        before = snapshot(empty), snapshot(other), snapshot(host)
        with pytest.raises(CmError) as e:
            apply_images([(empty, a, v), (other,) + full(LEFT), (empty, a, v)])
        assert e.value.status == 1 and "parts 0 and 2 name one image" in e.value.message and e.value.results is None
        assert (snapshot(empty), snapshot(other), snapshot(host)) == before
        rc, got = apply_images([(empty, a, v, np.zeros_like(v), default_hashes()[0], tree.root), (host,) + full(MIXED), (other,) + full(LEFT)], with_rc=True)
        assert rc == 1 and [g[0] for g in got] == [0, 1, 0] and "device images only" in got[1][2]
        assert last_error(backend.L) == "part 1: " + got[1][2]
        assert_image_is(empty, tree)                                              # its first cells are inserted
        assert_image_is(other, second_tree(LEFT))
        assert snapshot(host) == before[2] and got[1][1] == before[2][0]
    finally:
        for im in (empty, other, host):
            im.free()


@pytest.mark.gpu
def test_two_followed_runs(backend):
    """One three-segment heap run, followed twice: by a run of its first two segments, and by a run of all three whose middle
    update is bent.  The starting image is the memory under proof 0's initial_root, as in test_a_followed_run."""
    from tests.casm_fixtures import heap_program
    from tests.test_gpu_run import _cut
    from cairo_m_amd.lib import vm_segment
    hp, entry, nret, _ = heap_program()
    kw = dict(entry_pc=entry, n_returns=nret)
    ms = _cut(hp, 3, **kw)
    hss = [vm_segment(hp, max_steps=ms, segment=s, **kw) for s in range(3)]
    assert hss[0].n_segments == 3
    first = Run.from_segment(backend, hss[0])
    dev0 = first.adapt_next(hss[0])
    hi0 = backend.download_input(dev0)
    rows = prover_input_arrays(hi0.view)
    cells = [(int(r[0]),) + tuple(int(x) for x in r[1:5]) for r in rows["initial_memory"]]
    backend.free_input(dev0)
    hi0.free()
    first.free()
    run = Run.from_segment(backend, hss[0])
    proofs, moves = run.prove(hss, transitions=True)
    images = [MemImage.from_cells(cells, backend.L) for _ in range(4)]
    try:
        bare = [m.bare() for m in moves]
        assert moves[1].addresses.size > 0
        bent = MemTransition(bare[1].addresses, bare[1].old_values, bare[1].new_values.copy(), [], bare[1].root_before, bare[1].root_after)
        bent.new_values[0, 0] ^= 1
        finals = [p.public_data()["final_root"] for p in proofs]
        good, bad = (proofs[:2], bare[:2], images[0]), (proofs, [bare[0], bent, bare[2]], images[1])
        (root_good, said_good), (root_bad, said_bad) = follow_runs_images([good, bad])
        assert (root_good, said_good) == (finals[1], None) and images[0].root == finals[1]
        assert root_bad == finals[0] == images[1].root                            # the image stays at the last good segment
        assert said_bad.startswith("segment 1: ") and "would hash to root" in said_bad
        # the same two runs through the single-image follower, on copies
        assert follow_run_image(proofs[:2], bare[:2], images[2]) == root_good
        with pytest.raises(CmError) as e:
            follow_run_image(proofs, [bare[0], bent, bare[2]], images[3])
        assert "follow_run_image: " + said_bad == str(e.value) and images[3].root == root_bad
        assert snapshot(images[0]) == snapshot(images[2]) and snapshot(images[1]) == snapshot(images[3])
    finally:
        for im in images:
            im.free()
        for p in proofs:
            p.free()
        run.free()
        for hs in hss:
            hs.free()


@pytest.mark.gpu
def test_the_pool_is_back_at_its_level(backend):
    which = (LEFT, RIGHT, 9)                                                      # 9: the 1 500 random cells
    level = mem_stats(backend.L).live_bytes
    ims, twins = [image_of(backend, i) for i in which], [image_of(backend, i) for i in which]
    assert [s for s, _, _ in apply_images([(im,) + full(i) for im, i in zip(ims, which)])] == [0, 0, 0]
    for im, i in zip(twins, which):
        im.apply(*full(i))
    assert [im.stats()["bytes"] for im in ims] == [im.stats()["bytes"] for im in twins]
    # nothing of the call lives on but the images' own lists (the pool hands out a cached block that wastes at most a quarter, as
    # test_the_pool_counts_the_image_while_it_lives says)
    held = sum(im.stats()["bytes"] for im in ims + twins)
    assert level + held <= mem_stats(backend.L).live_bytes <= level + held + held // 4
    back = [(im, reference(i)["a"], reference(i)["old"]) for im, i in zip(ims, which)]
    assert [s for s, _, _ in apply_images(back)] == [0, 0, 0]                     # a second batch on the same images right after the first
    held = sum(im.stats()["bytes"] for im in ims + twins)
    assert level + held <= mem_stats(backend.L).live_bytes <= level + held + held // 4
    for im in ims + twins:
        im.free()
    assert mem_stats(backend.L).live_bytes == level


@pytest.mark.gpu
def test_the_launch_count_does_not_depend_on_the_number_of_parts(backend):
    """the in-library launch counters: the twelve SETS as 12 parts, and as 36 parts with the eight narrow sets three times more (each
    on a one-cell image of its own, bare), make the same launches in every new kernel class, those of cm_mem_batch_plan for the
    parts' addresses"""
    narrow = [i for i, (_, a) in enumerate(SETS) if len(a) <= 128]
    assert len(narrow) == 8
    counts = []
    for extra in (0, 3):
        ims = [image_of(backend, i) for i in range(len(SETS))]
        small = [(MemImage.from_cells(first_tree("a").cells, backend.L), i) for _ in range(extra) for i in narrow]
        try:
            backend.L.cm_kprof_enable(C.c_int32(1))
            got = apply_images([(im,) + full(i) for i, im in enumerate(ims)] + [(im, reference(i)["a"], reference(i)["new"]) for im, i in small])
            buf = C.create_string_buffer(1 << 16)
            backend.L.cm_kprof_report(buf, C.c_size_t(1 << 16))
            assert [g[0] for g in got] == [0] * (12 + 8 * extra)
            rep = json.loads(buf.value.decode())
            counts.append({k: rep[k]["calls"] for k in NEW_KERNELS})
        finally:
            backend.L.cm_kprof_enable(C.c_int32(0))
            for im in ims + [im for im, _ in small]:
                im.free()
    plan = mem_batch_plan([a for _, a in SETS])
    assert counts[0] == counts[1]
    assert counts[0] == {k: 1 for k in NEW_KERNELS} | {"k_imgs_level": sum(1 for s in plan if s["kernel"] == "level")}
    assert counts[0]["k_imgs_level"] == 6
