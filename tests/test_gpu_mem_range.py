"""Range openings on the GPU (cm_input_open_memory_range, cm_run_open_memory_range, cm_verify_memory_range) against
tests/mem_range_ref.py: the pinned host tree builder's node records and cm_poseidon2_permute, read from Python — never the code
under test.

The memories reach the device as the two trees of an uploaded input (cm_input_upload), as tests/test_gpu_mem_open.py does; the
shapes are those of the CPU test, whose plan tests show which kernels each of them runs.  An adapted scatter-store segment under
both tree builders and the two-segment heap run are checked against the reference tree over their own downloaded rows."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, MemRangeOpening, Run, prover_input_arrays, verify_range, verify_range_host, vm_run,
                             vm_segment)
from tests.mem_open_ref import image_cells
from tests.mem_range_ref import N_SLOTS, P, SHAPES, SPACE, RefTree, range_memories, ref_range, tampers
from tests.test_gpu_adapter import scatter_store_program
from tests.test_gpu_mem_open import _heap_run

pytestmark = pytest.mark.gpu

IDS = [f"{m}-{s}-{n}" for m, s, n in SHAPES]
NEXT = {"a": "b", "b": "c", "c": "straddle", "straddle": "dense", "dense": "a"}


@pytest.fixture(scope="module")
def uploaded(backend):
    """name -> (device input whose initial tree is that memory's and whose final tree is the next one's, the reference trees)"""
    trees = {k: RefTree(v) for k, v in range_memories().items()}
    out = {}
    for name, other in NEXT.items():
        ai = ArrayInput({"initial_tree": trees[name].nodes, "final_tree": trees[other].nodes, "roots": [trees[name].root, trees[other].root]})
        out[name] = (backend.upload_input(ai), ai)
    yield out, trees
    for dev, _ in out.values():
        backend.free_input(dev)


def _where(uploaded, name):
    """the two places memory `name` was uploaded to: (device input, which)"""
    devs, _ = uploaded
    prev = next(k for k, v in NEXT.items() if v == name)
    return [(devs[name][0], 0), (devs[prev][0], 1)]


def _same_as_reference(backend, dev, which, ref, start, n):
    rec, values, root = backend.open_memory_range(dev, which, start, n)
    want_words, want_values = ref_range(ref, start, n)
    assert root == ref.root
    assert rec.words() == want_words, (which, start, n)
    assert values.shape == (n, 4) and np.array_equal(values, want_values)
    assert verify_range(root, rec, values, backend.L)
    assert verify_range_host(root, rec, values, backend.L) == (0, "")
    return rec, values, root


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_ranges_of_uploaded_trees_equal_the_reference(backend, uploaded, shape):
    name, start, n = shape
    ref = uploaded[1][name]
    for dev, which in _where(uploaded, name):                                     # as an initial and as a final tree
        rec, values, root = _same_as_reference(backend, dev, which, ref, start, n)
        again, values_again, root_again = backend.open_memory_range(dev, which, start, n)
        assert root_again == root and bytes(again) == bytes(rec) and values_again.tobytes() == values.tobytes()
        if n == 1:
            single, single_root = backend.open_memory(dev, which, [start])
            assert single_root == root and list(single[0].value) == values[0].tolist()
            for k in range(N_SLOTS):
                used_left = bool((start >> k) & 1)
                assert (rec.left[k] if used_left else rec.right[k]) == single[0].siblings[k]
                assert (rec.right[k] if used_left else rec.left[k]) == 0


@pytest.mark.parametrize("device_trees", [False, True])
def test_ranges_of_an_adapted_segment_under_both_tree_builders(backend, monkeypatch, device_trees):
    """300 cells: below the 2048-row cut-over the adapter hashes its trees on the host; CM_ADAPTER_DEVICE_TREE_MIN=1 sends them
    through the device builder.  The range reads either node list."""
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    prog = scatter_store_program(300)
    hi, hs = vm_run(prog), vm_segment(prog)
    dev = backend.adapt_segment(hs)
    a = prover_input_arrays(hi.view)
    for which, key in ((0, "initial_memory"), (1, "final_memory")):
        ref = RefTree([tuple(int(x) for x in r[:5]) for r in a[key]])
        assert ref.root == a["roots"][which]                                      # the reference tree IS the input's tree
        touched = sorted(ref.present)
        lo, hi_a = touched[0], touched[-1]
        assert 300 <= hi_a - lo + 1 <= 1 << 16
        _same_as_reference(backend, dev, which, ref, lo, hi_a - lo + 1 + 3)      # every touched cell and three behind the last
        _same_as_reference(backend, dev, which, ref, max(lo, 1) - 1, 3)
    backend.free_input(dev)
    hi.free(); hs.free()


# ---- the run path ----------------------------------------------------------------------------------------------------------
def _image_is_what_the_root_commits_to(backend, run):
    lo, hp = run.memory()
    ref = RefTree(image_cells(lo, hp))
    ranges, root = run.open_image()
    assert root == ref.root
    spans = [(0, lo), (SPACE - hp.shape[0], hp[::-1])]                            # heap index i = the cell at 2^28 - 1 - i
    spans = [(s, v) for s, v in spans if v.shape[0]]
    assert [(r.start, r.n_cells) for r, _ in ranges] == [(s, v.shape[0]) for s, v in spans]
    for (rec, values), (s, want) in zip(ranges, spans):
        assert np.array_equal(values, want)
        assert rec.words() == ref_range(ref, s, want.shape[0])[0]
        assert verify_range(root, rec, values, backend.L) and verify_range_host(root, rec, values, backend.L)[0] == 0
    return ranges, root, lo.shape[0], hp.shape[0], ref


def test_run_ranges_follow_the_image(backend):
    hss = _heap_run()
    run = Run.from_segment(backend, hss[0])
    dev0 = run.adapt_next(hss[0])
    ranges0, root0, n_lo, n_hi, ref0 = _image_is_what_the_root_commits_to(backend, run)
    assert n_lo > 0 and n_hi > 0 and len(ranges0) == 2
    p0 = backend.prove_device(dev0)
    assert p0.public_data()["final_root"] == root0
    # into the gap behind the locals: zeros, under the same root as the single openings
    rec, values, root = run.open_range(n_lo - 2, 5)
    assert root == root0 and rec.words() == ref_range(ref0, n_lo - 2, 5)[0]
    assert not values[2:].any() and np.array_equal(values[:2], run.memory()[0][-2:])
    assert verify_range(root, rec, values, backend.L)
    single, single_root = run.open([n_lo])                                        # the one cached tree serves both calls
    assert single_root == root0 and single[0].present == 0
    dev1 = run.adapt_next(hss[1])
    p1 = backend.prove_device(dev1)
    ranges1, root1, n_lo1, n_hi1, _ = _image_is_what_the_root_commits_to(backend, run)
    assert root1 == p1.public_data()["final_root"] and root1 != root0
    # a range opened before the advance: still good under its own root, not under the new one where a cell of it changed
    lo1, hp1 = run.memory()
    for (rec, values), now in zip(ranges0, (lo1[:n_lo], hp1[:n_hi][::-1])):
        assert verify_range(root0, rec, values, backend.L)
        changed = not np.array_equal(values, now)
        if changed:
            assert not verify_range(root1, rec, values, backend.L)
            assert verify_range_host(root1, rec, values, backend.L)[0] == 11
    assert any(not np.array_equal(v, now) for (_, v), now in zip(ranges0, (lo1[:n_lo], hp1[:n_hi][::-1])))
    for p in (p0, p1):
        p.free()
    for d in (dev0, dev1):
        backend.free_input(d)
    run.free()
    for hs in hss:
        hs.free()


# ---- the verifier -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_each_tamper_flips_the_verdict_and_the_gpu_agrees_with_the_host(backend, uploaded, shape):
    name, start, n = shape
    ref = uploaded[1][name]
    dev, which = _where(uploaded, name)[0]
    rec, values, root = backend.open_memory_range(dev, which, start, n)
    assert verify_range(root, rec, values, backend.L) and verify_range_host(root, rec, values, backend.L)[0] == 0
    cases = tampers(rec.words(), values, root)
    assert len(cases) >= 8
    for what, (w, v, r, _) in cases.items():
        o = MemRangeOpening.from_words(w)
        gpu, host = verify_range(r, o, v, backend.L), verify_range_host(r, o, v, backend.L)[0]
        assert gpu is False and host == 11, (what, gpu, host)
    # malformed headers are verdicts of the device call too, not failures
    for w in ([start, 0] + rec.words()[2:], [SPACE - n + 1, n] + rec.words()[2:]):
        o = MemRangeOpening.from_words(w)
        v = values if w[1] else np.zeros((1, 4), dtype=np.uint32)
        ok = C.c_uint8(7)
        assert backend.L.cm_verify_memory_range(C.c_uint32(root), C.byref(o), v.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(ok), C.c_uint64(0)) == 0
        assert ok.value == 0
        assert backend.L.cm_verify_memory_range_host(C.c_uint32(root), C.byref(o), v.ctypes.data_as(C.POINTER(C.c_uint32))) == 11


# ---- refusals and accounting ------------------------------------------------------------------------------------------------
def test_refusals_leave_the_run_and_the_input_usable(backend, uploaded):
    dev, which = _where(uploaded, "a")[0]
    ref = uploaded[1]["a"]
    live = backend.mem_stats().live_bytes
    for w, start, n, needle in ((which, 5, 0, "no cells"), (which, SPACE - 1, 2, "beyond the address space"), (which, SPACE, 1, "beyond the address space"),
                                (which, 0, (1 << 24) + 1, "more than 2^24 cells"), (2, 5, 1, "`which`")):
        with pytest.raises(CmError) as e:
            backend.open_memory_range(dev, w, start, n)
        assert "status 1:" in str(e.value) and needle in str(e.value), str(e.value)
    # nothing is written by a refused call: a tiny buffer under a range of 2^24 + 1 cells
    sentinel_v, sentinel_o, r = (C.c_uint32 * 4)(*[0xABABABAB] * 4), MemRangeOpening.from_words([0xABABABAB] * 58), C.c_uint32(0xABABABAB)
    L = backend.L
    for args in ((C.c_uint32(0), C.c_uint32((1 << 24) + 1), sentinel_v, C.byref(sentinel_o), C.byref(r)),
                 (C.c_uint32(5), C.c_uint32(1), None, C.byref(sentinel_o), C.byref(r)),
                 (C.c_uint32(5), C.c_uint32(1), sentinel_v, None, C.byref(r)),
                 (C.c_uint32(5), C.c_uint32(1), sentinel_v, C.byref(sentinel_o), None)):
        assert L.cm_input_open_memory_range(dev, C.c_uint32(which), *args) == 1
    assert list(sentinel_v) == [0xABABABAB] * 4 and sentinel_o.words() == [0xABABABAB] * 58 and r.value == 0xABABABAB
    ok = C.c_uint8(7)
    big = MemRangeOpening.from_words([0, (1 << 24) + 1] + [0] * 56)
    assert L.cm_verify_memory_range(C.c_uint32(0), C.byref(big), sentinel_v, C.byref(ok), C.c_uint64(0)) == 1 and ok.value == 7
    assert L.cm_verify_memory_range(C.c_uint32(0), None, sentinel_v, C.byref(ok), C.c_uint64(0)) == 1
    _same_as_reference(backend, dev, which, ref, 4, 3)                            # the input is as usable as before
    assert backend.mem_stats().live_bytes == live                                 # every buffer of the calls went back to the pool

    empty = backend.run_begin(np.zeros((0, 4), dtype=np.uint32), np.zeros((0, 4), dtype=np.uint32), [0, 0, 0, 0, 0, 0])
    with pytest.raises(CmError) as e:
        empty.open_range(0, 1)
    assert "status 1:" in str(e.value) and "empty" in str(e.value), str(e.value)
    with pytest.raises(CmError):
        empty.open_image()
    empty.free()

    lo = np.arange(40, dtype=np.uint32).reshape(10, 4)
    none = np.zeros((0, 4), dtype=np.uint32)
    idle = backend.mem_stats().live_bytes
    run = backend.run_begin(lo, none, [0, 1, 1, 1, 1, 1])
    before = backend.mem_stats().live_bytes
    _, _, root = run.open_range(3, 2)
    with_tree = backend.mem_stats().live_bytes
    assert with_tree > before                                                     # the cached image tree, and nothing else:
    for start, n in ((3, 0), (SPACE - 1, 2), (0, (1 << 24) + 1)):
        with pytest.raises(CmError):
            run.open_range(start, n)
    rec, values, root_after = run.open_range(3, 2)
    assert verify_range(root_after, rec, values, backend.L)
    assert not verify_range((root_after + 1) % P, rec, values, backend.L)
    assert backend.mem_stats().live_bytes == with_tree
    ranges, image_root = run.open_image()                                         # the heap is empty: one range
    assert image_root == root_after == root == RefTree(image_cells(lo, none)).root
    assert len(ranges) == 1 and np.array_equal(ranges[0][1], lo) and values.tolist() == [[12, 13, 14, 15], [16, 17, 18, 19]]
    assert backend.mem_stats().live_bytes == with_tree
    run.free()
    assert backend.mem_stats().live_bytes == idle                                 # the tree went with the run
