"""Batched set openings on the GPU (cm_mem_images_open_memory_sets, mem_image_open_batch.inc): all twelve SETS as twelve parts of
one call against ref_set and the reference trees, byte-equal to the single calls and accepted by verify_sets; the same parts in
other orders; forty parts under ONE image with three short rooms among them; every kind of bad part the call can express among
opened neighbours; an output block that crosses the landing buffer's trip boundary; the launch count, which does not depend on
the number of parts; the pool's accounting; and openings from two threads while a third updates the image.  Every part of every
call is compared."""
import ctypes as C
import functools
import json
import threading

import numpy as np
import pytest

from cairo_m_amd.lib import MemImage, mem_set_plan, mem_stats, open_sets, verify_sets
from tests.mem_image_ref import first_tree, reference
from tests.mem_set_ref import SETS, SPACE, ref_set
from tests.test_mem_open_batch_cpu import SENTINEL, Arrays, call, last_error, ptr

DENSE = (8, 9, 10, 11)                                                            # the four sets of memory "dense"
WHO = "cm_mem_image_open_memory_set: "


def image_of(backend, i):
    return MemImage.from_cells(first_tree(SETS[i][0]).cells, backend.L)


@functools.lru_cache(maxsize=None)
def want(i):
    """(sibling words, values (n, 4), counts, root) of SETS[i] under its memory's reference tree"""
    tree = first_tree(SETS[i][0])
    return ref_set(tree, SETS[i][1]) + (tree.root,)


def same(rec, other):
    return (rec.addresses.tobytes(), rec.values.tobytes(), rec.siblings.tobytes(), rec.counts) == \
           (other.addresses.tobytes(), other.values.tobytes(), other.siblings.tobytes(), other.counts)


@pytest.fixture(scope="module")
def twelve(backend):
    """one device image per set, each of its own memory, and what the single call gives for it: made once, never changed"""
    ims = [image_of(backend, i) for i in range(len(SETS))]
    single = [im.open_set(SETS[i][1]) for i, im in enumerate(ims)]
    yield ims, single
    for im in ims:
        im.free()


def check_parts(backend, twelve, order):
    """the sets `order` as the parts of one call: every part against the reference, against the single call, and verify_sets"""
    ims, single = twelve
    rc, got = open_sets([(ims[i], SETS[i][1]) for i in order], backend.L, with_rc=True)
    assert rc == 0 and len(got) == len(order)
    for i, (status, message, rec, root) in zip(order, got):
        words, values, counts, tree_root = want(i)
        assert (status, message) == (0, ""), (i, message)
        assert root == tree_root == single[i][1]
        assert rec.addresses.tolist() == SETS[i][1] and rec.siblings.tolist() == words and np.array_equal(rec.values, values) and rec.counts == counts
        assert same(rec, single[i][0]), i
    assert verify_sets([g[3] for g in got], [g[2] for g in got], backend.L) == [True] * len(order)


# ---- the reference side, checked without a GPU --------------------------------------------------------------------------------
def test_the_fixtures_stand_on_their_own():
    """the twelve sets hold the shapes the gather can go wrong on, and the boundary test's block crosses a trip where it says"""
    widths = [len(a) for _, a in SETS]
    assert len(SETS) == 12 and min(widths) == 1 and max(widths) == 1667
    assert mem_set_plan(SETS[4][1])[1] == 54 and mem_set_plan(SETS[5][1])[1] == 2 * 27      # two cells: 54 words; a pair that meets at the root
    assert mem_set_plan(SETS[8][1])[0][1]["n_nodes"] == 1667                               # no two cells share a parent
    held = {c[0] for c in first_tree("c").cells}
    assert any(x not in held for x in SETS[7][1]) and [0, 0, 0, 0] in want(6)[1].tolist()   # absent cells; a held zero cell
    assert [SETS[i][0] for i in DENSE] == ["dense"] * 4
    assert sum(1 for w in widths if w <= 128) == 8
    # 16 bytes of counts, then 2^19 * 16 bytes of values: the 8 MiB trip ends 16 bytes before the second part's values do
    assert 16 + (1 << 19) * 16 > (8 << 20) > 16 + (1 << 18) * 16 and mem_set_plan(range(1 << 18, 1 << 19))[1] == 10


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_twelve_sets_as_twelve_parts_of_one_call(backend, twelve):
    check_parts(backend, twelve, list(range(12)))


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["reversed", "shuffled"])
def test_results_follow_the_parts(backend, twelve, order):
    """one-cell parts between wide ones, wide ones first"""
    ids = list(range(12))[::-1] if order == "reversed" else [int(x) for x in np.random.default_rng(7).permutation(12)]
    assert ids != list(range(12))
    check_parts(backend, twelve, ids)


@pytest.mark.gpu
def test_forty_parts_under_one_image_three_with_short_room(backend, twelve):
    ims, single = twelve
    im = ims[DENSE[0]]                                                            # an image of memory "dense"
    short = (3, 20, 39)
    which = [DENSE[j % 4] for j in range(40)]
    parts = []
    for j, i in enumerate(which):
        need = mem_set_plan(SETS[i][1])[1]
        parts.append(Arrays(im.h, SETS[i][1], cap=need - 1 if j in short else None))
    rc, msg, res = call(backend.L, [p.part for p in parts])
    root = first_tree("dense").root
    for j, (i, p, r) in enumerate(zip(which, parts, res)):
        rec = single[i][0]
        assert r.root == root and r.n_siblings == rec.siblings.size == p.need
        if j in short:
            said = WHO + f"room for {p.need - 1} sibling words where the set needs {p.need}"
            assert (r.status, r.message.decode()) == (1, said) and p.clean()
            # the single call's own status and message, and its arrays stay untouched too
            alone = Arrays(im.h, SETS[i][1], cap=p.need - 1)
            n_sib, got_root = C.c_uint32(0), C.c_uint32(0)
            rc1 = backend.L.cm_mem_image_open_memory_set(im.h, ptr(alone.a), C.c_uint64(alone.a.size), ptr(alone.v), ptr(alone.w), C.c_uint32(alone.cap),
                                                         C.byref(n_sib), C.byref(got_root))
            assert (rc1, last_error(backend.L)) == (1, said) and n_sib.value == p.need and alone.clean()
        else:
            assert (r.status, r.message) == (0, b"")
            assert p.v.tobytes() == rec.values.tobytes() and p.w.tobytes() == rec.siblings.tobytes()
    assert rc == 1 and msg == "part 3: " + res[3].message.decode()


@pytest.mark.gpu
def test_one_bad_part_of_each_kind_among_good_neighbours(backend, twelve):
    ims, single = twelve
    host = MemImage.from_cells(first_tree("a").cells, backend.L, device=False)
    empty = MemImage.from_cells([], backend.L)
    try:
        good = lambda i: Arrays(ims[i].h, SETS[i][1])
        c = ims[6]                                                                # memory "c"
        bad = [
            (Arrays(host.h, [4, 5]), "a host image serves no openings: create the image with device = 1"),
            (Arrays(empty.h, [4, 5]), "the image is empty: there is no tree to open"),
            (Arrays(c.h, []), "a set of no cells"),
            (Arrays(c.h, [8, 7]), "address 1 is not above address 0 (7): the addresses must be strictly ascending and below 2^28"),
            (Arrays(c.h, [7, SPACE]), f"address 1 is beyond the address space of 2^28 cells ({SPACE}): the addresses must be strictly ascending and below 2^28"),
            (Arrays(c.h, [7, 8], values=False), "null argument"),
        ]
        neighbours = [8, 0, 9, 4, 6, 11, 1]                                       # wide and narrow, one more than the bad parts
        parts = [good(neighbours[0])]
        for (b, _), i in zip(bad, neighbours[1:]):
            parts += [b, good(i)]
        rc, msg, res = call(backend.L, [p.part for p in parts])
        for j, (p, r) in enumerate(zip(parts, res)):
            if j % 2:
                b, said = bad[j // 2]
                assert (r.status, r.message.decode()) == (1, WHO + said), j
                assert b.clean() and r.root == (first_tree("a").root if j == 1 else empty.root if j == 3 else first_tree("c").root)
                # the single call's own status and message
                n_sib, got_root = C.c_uint32(0), C.c_uint32(0)
                # (a c_void_p field reads back as a plain int, which ctypes would pass as a 32-bit C int: wrap it again)
                rc1 = backend.L.cm_mem_image_open_memory_set(C.c_void_p(b.part.img), b.part.addresses, C.c_uint64(b.part.n), b.part.values, b.part.siblings,
                                                             C.c_uint32(b.cap), C.byref(n_sib), C.byref(got_root))
                assert (rc1, last_error(backend.L)) == (1, WHO + said) and b.clean()
            else:
                i = neighbours[j // 2]
                rec, root = single[i]
                assert (r.status, r.message, r.root, r.n_siblings) == (0, b"", root, rec.siblings.size), j
                assert p.v.tobytes() == rec.values.tobytes() and p.w.tobytes() == rec.siblings.tobytes(), j
        assert rc == 1 and msg == "part 1: " + WHO + bad[0][1]
    finally:
        host.free()
        empty.free()


@pytest.mark.gpu
def test_the_output_block_crosses_a_trip_of_the_landing_buffer(backend):
    """an image of 2^19 consecutive cells opened as two parts of 2^18: 16 bytes of counts and 8 MiB of values, so the first trip
    ends inside the second part's values.  No Python tree at this size: the values are the cells', the records the single calls'."""
    n = 1 << 19
    a = np.arange(n, dtype=np.uint32)
    v = np.random.default_rng(20250611).integers(0, (1 << 31) - 1, (n, 4)).astype(np.uint32)
    h = C.c_void_p()
    assert backend.L.cm_mem_image_create(ptr(a), ptr(v), C.c_uint64(n), C.c_uint32(1), C.byref(h)) == 0
    im = MemImage(backend.L, h, True)
    try:
        halves = [a[:n // 2], a[n // 2:]]
        rc, got = open_sets([(im, x) for x in halves], backend.L, with_rc=True)
        assert rc == 0 and [(g[0], g[1]) for g in got] == [(0, ""), (0, "")]
        for j, (x, (_, _, rec, root)) in enumerate(zip(halves, got)):
            assert root == im.root and rec.siblings.size == 10
            assert rec.values.tobytes() == v[j * (n // 2):(j + 1) * (n // 2)].tobytes()
            alone, alone_root = im.open_set(x)
            assert alone_root == root and same(rec, alone)
        assert verify_sets(im.root, [g[2] for g in got], backend.L) == [True, True]
    finally:
        im.free()


@pytest.mark.gpu
def test_the_launch_count_does_not_depend_on_the_number_of_parts(backend, twelve):
    """the in-library launch counters: the twelve SETS as 12 parts, and as 36 parts with the eight narrow sets three times more,
    make the same calls in the new kernel class: exactly one"""
    ims, single = twelve
    narrow = [i for i, (_, a) in enumerate(SETS) if len(a) <= 128]
    assert len(narrow) == 8
    counts = []
    for extra in (0, 3):
        order = list(range(12)) + narrow * extra
        try:
            backend.L.cm_kprof_enable(C.c_int32(1))
            got = open_sets([(ims[i], SETS[i][1]) for i in order], backend.L)
            buf = C.create_string_buffer(1 << 16)
            backend.L.cm_kprof_report(buf, C.c_size_t(1 << 16))
        finally:
            backend.L.cm_kprof_enable(C.c_int32(0))
        assert len(got) == 12 + 8 * extra and all(g[0] == 0 and same(g[2], single[i][0]) for i, g in zip(order, got))
        counts.append(json.loads(buf.value.decode())["k_sets_gather"]["calls"])
    assert counts == [1, 1]


@pytest.mark.gpu
def test_the_pool_is_back_at_its_level(backend):
    which = (1, 8, 9)
    level = mem_stats(backend.L).live_bytes
    ims = [image_of(backend, i) for i in which]
    held = sum(im.stats()["bytes"] for im in ims)
    with_images = mem_stats(backend.L).live_bytes
    # (the pool hands out a cached block that wastes at most a quarter, as test_the_pool_counts_the_image_while_it_lives says)
    assert level + held <= with_images <= level + held + held // 4
    got = open_sets([(im, SETS[i][1]) for im, i in zip(ims, which)] + [(ims[1], SETS[10][1])], backend.L)
    assert [g[0] for g in got] == [0, 0, 0, 0]
    assert mem_stats(backend.L).live_bytes == with_images                         # nothing of the call lives on: only the images are counted
    for im in ims:
        im.free()
    assert mem_stats(backend.L).live_bytes == level


@pytest.mark.gpu
def test_two_threads_open_while_a_third_updates(backend):
    """Two threads each open the two sets of memory "c" under ONE image through the batch ten times while a third applies the
    update of SETS[6] through cm_mem_image_apply.  Every record verifies under the root it came with, which is the root before the
    update or the root after it.  (Small sets on purpose: every thread has a pool of its own, and device memory in small blocks
    that several pools held at once stays with the driver's allocator after a trim, which the suite's memory tests would see.)"""
    both = (6, 7)
    assert [SETS[i][0] for i in both] == ["c", "c"]
    r = reference(both[0])
    im = image_of(backend, both[0])
    out, failed = [[], []], []

    def opener(k):
        try:
            for _ in range(10):
                out[k].append(open_sets([(im, SETS[i][1]) for i in both], backend.L))
        except Exception as e:                                                    # (a thread's exception is the test's)
            failed.append(e)

    def updater():
        try:
            assert im.apply(r["a"], r["new"], r["old"], r["root0"], r["root1"]) == r["root1"]
        except Exception as e:
            failed.append(e)

    try:
        ts = [threading.Thread(target=opener, args=(0,)), threading.Thread(target=opener, args=(1,)), threading.Thread(target=updater)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not failed, failed
        got = [g for k in range(2) for call_ in out[k] for g in call_]
        assert len(got) == 2 * 10 * 2 and all(g[0] == 0 for g in got)
        for call_ in out[0] + out[1]:
            assert len({g[3] for g in call_}) == 1                                # one call, one root: the lock is held over all its parts
        assert {g[3] for g in got} <= {r["root0"], r["root1"]} and im.root == r["root1"]
        assert verify_sets([g[3] for g in got], [g[2] for g in got], backend.L) == [True] * len(got)
        assert [x.tolist() for x in (got[0][2].addresses, got[-1][2].addresses)] == [SETS[both[0]][1], SETS[both[1]][1]]
    finally:
        im.free()
