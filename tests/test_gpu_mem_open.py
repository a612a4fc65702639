"""Memory openings on the GPU (cm_input_open_memory, cm_run_open_memory, cm_verify_memory_openings) against tests/mem_open_ref.py:
the pinned host tree builder's node records and cm_poseidon2_permute, read from Python — never the code under test.

Memories (a), (b), (c) of the CPU test and a seeded random 300-cell memory are sparse, which no runner segment's dense memory
can be: they reach the device as the two trees of an uploaded input (cm_input_upload), built by the host builder.  Adapted
segments — scatter_store_program(300) with host-built and with device-built trees, a segment of the "high" run with cells only
ever read as zero, and the run path — are checked against the reference tree over their own downloaded rows."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, MemOpening, Run, prover_input_arrays, verify_opening, verify_openings, vm_run,
                             vm_segment)
from tests.mem_open_ref import ABSENT_NEAR, P, SPACE, WORDS, ZERO_CELL_OF_C, RefTree, image_cells, memories, tampers
from tests.test_gpu_adapter import scatter_store_program

pytestmark = pytest.mark.gpu

N_QUERIES = 257                                                                 # crosses a 256-thread block of the batched verifier


def _random_memory():
    rng = np.random.default_rng(20240611)
    addrs = sorted({int(a) for a in rng.integers(0, SPACE, 310)})[:300]
    cells = [(a,) + tuple(int(x) for x in rng.integers(0, P, 4)) for a in addrs]
    cells[17] = (cells[17][0], 0, 0, 0, 0)                                      # one cell holds zeros explicitly
    return cells


def _addresses(ref, extra=()):
    """257 addresses: present and absent cells, absent neighbours of present ones, duplicates, a descending stretch"""
    rng = np.random.default_rng(7)
    present = sorted(ref.present)
    out = [int(a) for a in extra]
    out += [present[int(i)] for i in rng.integers(0, len(present), 100)]
    out += [present[0], present[-1]]
    out += [a for a in (int(x) for x in rng.integers(0, SPACE, 60)) if a not in ref.present]
    out += [p ^ 1 for p in present[:20] if (p ^ 1) not in ref.present]
    out += [0, SPACE - 1]
    out += out[:10]
    out = (out * (N_QUERIES // len(out) + 1))[:N_QUERIES]
    out[100:200] = sorted(out[100:200], reverse=True)
    assert len(out) == N_QUERIES and len(set(out)) < len(out)
    assert any(a in ref.present for a in out) and any(a not in ref.present for a in out)
    return out


def _words(openings):
    return np.array([o.words() for o in openings], dtype=np.uint32).reshape(-1, WORDS)


def _same_as_reference(backend, dev, which, ref, addrs):
    got, root = backend.open_memory(dev, which, addrs)
    want = ref.openings(addrs)
    assert root == ref.root
    bad = np.nonzero((_words(got) != want).any(axis=1))[0]
    assert bad.size == 0, (which, bad[:5], _words(got)[bad[:1]], want[bad[:1]])
    assert all(verify_openings(root, got, backend.L))
    return got, root


@pytest.fixture(scope="module")
def uploaded(backend):
    """name -> (device input whose initial / final trees are those of two memories, their reference trees)"""
    mem = dict(memories(), random300=_random_memory())
    pairs = {"a": ("a", "b"), "b": ("b", "c"), "c": ("c", "random300"), "random300": ("random300", "a")}
    trees = {k: RefTree(v) for k, v in mem.items()}
    out = {}
    for name, (i, f) in pairs.items():
        ai = ArrayInput({"initial_tree": trees[i].nodes, "final_tree": trees[f].nodes, "roots": [trees[i].root, trees[f].root]})
        out[name] = (backend.upload_input(ai), trees[i], trees[f], ai)
    yield out
    for dev, _, _, _ in out.values():
        backend.free_input(dev)


@pytest.mark.parametrize("name", ["a", "b", "c", "random300"])
def test_openings_of_uploaded_trees_equal_the_reference(backend, uploaded, name):
    dev, ti, tf, _ = uploaded[name]
    for which, ref in ((0, ti), (1, tf)):
        extra = [c[0] for c in ref.cells if not any(c[1:])]                       # cells held with an all-zero value
        _same_as_reference(backend, dev, which, ref, _addresses(ref, extra))
    got, root = backend.open_memory(dev, 0, [])                                   # n = 0: the root alone
    assert got == [] and root == ti.root


def _rows_tree(rows):
    return RefTree([tuple(int(x) for x in r[:5]) for r in rows])


def _adapted_case(backend, hi, hs):
    dev = backend.adapt_segment(hs)
    a = prover_input_arrays(hi.view)
    zero_cells = 0
    for which, key in ((0, "initial_memory"), (1, "final_memory")):
        ref = _rows_tree(a[key])
        assert ref.root == a["roots"][which]                                      # the reference tree IS the input's tree
        zeros = [int(r[0]) for r in a[key] if not r[1:5].any()][:5]             # cells the segment only ever read as zero
        zero_cells += len(zeros)
        _same_as_reference(backend, dev, which, ref, _addresses(ref, zeros))
    backend.free_input(dev)
    hi.free(); hs.free()
    return zero_cells


@pytest.mark.parametrize("device_trees", [False, True])
def test_openings_of_an_adapted_segment_under_both_tree_builders(backend, monkeypatch, device_trees):
    """300 cells: below the 2048-row cut-over the adapter hashes its trees on the host; CM_ADAPTER_DEVICE_TREE_MIN=1 sends them
    through the device builder.  The openings read either node list."""
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    prog = scatter_store_program(300)
    _adapted_case(backend, vm_run(prog), vm_segment(prog))


def test_a_cell_touched_only_by_a_zero_read_opens_as_present_zero(backend):
    from tests.test_gpu_run import _runs
    mk_input, mk_segment, max_steps, _ = _runs()["high"]
    assert _adapted_case(backend, mk_input(1, max_steps), mk_segment(1, max_steps)) > 0


# ---- the run path ----------------------------------------------------------------------------------------------------------
def _heap_run():
    from tests.casm_fixtures import heap_program
    from tests.test_gpu_run import _cut
    hp, entry, nret, _ = heap_program()
    kw = dict(entry_pc=entry, n_returns=nret)
    ms = _cut(hp, 2, **kw)
    hss = [vm_segment(hp, max_steps=ms, segment=s, **kw) for s in range(2)]
    assert hss[0].n_segments == 2
    return hss


def _image_reference(run):
    lo, hp = run.memory()
    return RefTree(image_cells(lo, hp)), lo.shape[0], hp.shape[0]


def test_run_openings_follow_the_image(backend):
    hss = _heap_run()
    run = Run.from_segment(backend, hss[0])
    dev0 = run.adapt_next(hss[0])
    ref, n_lo, n_hi = _image_reference(run)
    assert n_lo > 0 and n_hi > 0
    addrs = _addresses(ref, [n_lo, SPACE - 1 - n_hi])                           # (both lie in the gap between the regions)
    got, root = run.open(addrs)
    assert root == ref.root and np.array_equal(_words(got), ref.openings(addrs))
    again, root_again = run.open(addrs)                                           # the cached tree: identical bytes
    assert root_again == root and _words(again).tobytes() == _words(got).tobytes()
    p0 = backend.prove_device(dev0)
    assert p0.public_data()["final_root"] == root
    dev1 = run.adapt_next(hss[1])
    p1 = backend.prove_device(dev1)
    pd1 = p1.public_data()
    assert pd1["initial_root"] == root
    ref1, _, _ = _image_reference(run)
    out_entries = pd1["output"]
    out_addrs = [int(e[1]) for e in out_entries if e[0]]
    assert len(out_addrs) > 0
    got1, root1 = run.open(out_addrs + addrs)
    assert root1 == ref1.root == pd1["final_root"] and root1 != root           # the tree was dropped with the old image
    assert np.array_equal(_words(got1), ref1.openings(out_addrs + addrs))
    for o, e in zip(got1, [e for e in out_entries if e[0]]):
        assert o.present == 1 and list(o.value) == [int(x) for x in e[2:6]]     # cm_proof_public_entries(which = 2)
    assert all(verify_openings(root1, got1, backend.L))
    for p in (p0, p1):
        p.free()
    for d in (dev0, dev1):
        backend.free_input(d)
    run.free()
    for hs in hss:
        hs.free()


def test_run_openings_of_a_large_image_with_a_gap(backend):
    """3000 cells (above the adapter's 2048-row cut-over), both regions non-empty, queries in the gap and at both region edges"""
    rng = np.random.default_rng(3000)
    lo = rng.integers(0, P, (2900, 4)).astype(np.uint32)
    hp = rng.integers(0, P, (100, 4)).astype(np.uint32)
    lo[1234] = 0
    run = backend.run_begin(lo, hp, [0, 1, 1, 1, 1, 1])
    ref = RefTree(image_cells(lo, hp))
    addrs = _addresses(ref, [2900, 1 << 27, SPACE - 101, SPACE - 100, 2899, 1234])
    got, root = run.open(addrs)
    assert root == ref.root and np.array_equal(_words(got), ref.openings(addrs))
    assert [o.present for o in got[:6]] == [0, 0, 0, 1, 1, 1]
    assert all(verify_openings(root, got, backend.L))
    run.free()


# ---- the batched verifier ---------------------------------------------------------------------------------------------------
def test_each_tamper_flips_its_own_verdict_and_no_other(backend, uploaded):
    dev, ref, _, _ = uploaded["c"]
    addrs = _addresses(ref, [ZERO_CELL_OF_C])
    got, root = backend.open_memory(dev, 0, addrs)
    words = _words(got)
    present_at = [i for i, a in enumerate(addrs) if a in ref.present and a != ZERO_CELL_OF_C]
    absent_at = [i for i, a in enumerate(addrs) if a not in ref.present]
    # positions on both sides of the wave and block edges of the verifier, the last record included
    want_pos = [0, 1, 62, 63, 64, 65, 127, 128, 191, 255]
    pos = []
    for w in want_pos:
        pos.append(min((i for i in present_at if i not in pos), key=lambda i: abs(i - w)))
    batch = words.copy()
    changed = {}
    names = ["value[0]", "value[1]", "value[2]", "value[3]", "siblings[0]", "siblings[27]", "address neighbour", "address bit 27",
             "present = 2", "word = P"]
    for i, name in zip(pos, names):
        batch[i] = tampers([int(x) for x in words[i]], root, ref.opening(ABSENT_NEAR["c"]))[name][0]
        changed[i] = name
    last_absent = absent_at[-1]
    batch[last_absent] = tampers([int(x) for x in words[pos[0]]], root, [int(x) for x in words[last_absent]])["absent with value[0] = 1"][0]
    changed[last_absent] = "absent with value[0] = 1"
    if N_QUERIES - 1 not in changed:                                              # the record behind the 256-thread edge
        batch[N_QUERIES - 1, 6 + 5] = (int(batch[N_QUERIES - 1, 6 + 5]) + 1) % P
        changed[N_QUERIES - 1] = "siblings[5]"
    ok = verify_openings(root, batch, backend.L)
    assert [i for i, v in enumerate(ok) if not v] == sorted(changed), changed
    host = [verify_opening(root, MemOpening.from_words(r), backend.L)[0] == 0 for r in batch]
    assert ok == host
    zero_as_absent = ref.opening(ZERO_CELL_OF_C, present=0)
    assert verify_openings(root, [MemOpening.from_words(zero_as_absent)], backend.L) == [True]
    assert not any(verify_openings((root + 1) % P, words, backend.L))           # the root itself
    assert verify_openings(root, [], backend.L) == []


# ---- refusals and accounting ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_run_usable(backend, uploaded):
    dev, ref, _, _ = uploaded["a"]
    for which, addrs, needle in ((0, [5, SPACE], "beyond the address space"), (2, [5], "`which`")):
        with pytest.raises(CmError) as e:
            backend.open_memory(dev, which, addrs)
        assert "status 1:" in str(e.value) and needle in str(e.value), str(e.value)
    empty = backend.run_begin(np.zeros((0, 4), dtype=np.uint32), np.zeros((0, 4), dtype=np.uint32), [0, 0, 0, 0, 0, 0])
    with pytest.raises(CmError) as e:
        empty.open([0])
    assert "status 1:" in str(e.value) and "empty" in str(e.value), str(e.value)
    empty.free()
    lo = np.arange(40, dtype=np.uint32).reshape(10, 4)
    run = backend.run_begin(lo, np.zeros((0, 4), dtype=np.uint32), [0, 1, 1, 1, 1, 1])
    _, root = run.open([3])
    sentinel = (MemOpening * 2)()
    C.memset(sentinel, 0xAB, C.sizeof(sentinel))
    r = C.c_uint32(0)
    a = (C.c_uint32 * 2)(3, SPACE)
    assert backend.L.cm_run_open_memory(run.h, a, C.c_uint64(2), sentinel, C.byref(r)) == 1
    assert bytes(sentinel) == b"\xab" * C.sizeof(sentinel)                        # nothing was written to out
    got, root_after = run.open([3])
    assert root_after == root == RefTree(image_cells(lo, np.zeros((0, 4), dtype=np.uint32))).root
    assert list(got[0].value) == [12, 13, 14, 15]
    run.free()


def test_the_image_tree_is_counted_while_it_lives(backend):
    """live bytes rise on the first Run.open and are back after adapt_next: the tree is dropped, not rebuilt.  The same calls
    without the opening are the control (the advance may grow the image itself)."""
    def walk(opening):
        hss = _heap_run()
        run = Run.from_segment(backend, hss[0])
        backend.free_input(run.adapt_next(hss[0]))
        before = backend.mem_stats().live_bytes
        risen = before
        if opening:
            run.open([0])
            risen = backend.mem_stats().live_bytes
            run.open([1])                                                         # the cached tree: no second one
            assert backend.mem_stats().live_bytes == risen
        backend.free_input(run.adapt_next(hss[1]))
        after = backend.mem_stats().live_bytes
        run.free()
        for hs in hss:
            hs.free()
        return before, risen, after

    b0, _, a0 = walk(False)
    b1, r1, a1 = walk(True)
    print("live bytes: control", b0, a0, "with an opening", b1, r1, a1)
    assert r1 > b1
    assert a1 - b1 == a0 - b0
    assert a1 < r1
