"""Set openings on the GPU (cm_input_open_memory_set, cm_run_open_memory_set, cm_verify_memory_set) against
tests/mem_set_ref.py: the pinned host tree builder's node records and cm_poseidon2_permute, read from Python — never the code
under test — and against the single and the range openings, whose special cases they are.

The memories reach the device as the two trees of an uploaded input (cm_input_upload), as tests/test_gpu_mem_range.py does; the
sets are those of the CPU test, whose plan test shows which kernels and which kinds of parent each of them runs.  An adapted
scatter-store segment under both tree builders and the two-segment heap run are checked against the reference tree over their own
downloaded rows; the segment's write set shows the root after the write from the sibling words opened before it."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, MemSetOpening, Run, prover_input_arrays, set_root, verify_set, verify_set_host, vm_run,
                             vm_segment)
from tests.mem_open_ref import image_cells
from tests.mem_set_ref import CONTIGUOUS, MIXED, N_DEPTHS, SET_IDS, SETS, SPACE, RefTree, range_memories, ref_set, tampers
from tests.test_gpu_adapter import scatter_store_program
from tests.test_gpu_mem_open import _heap_run

pytestmark = pytest.mark.gpu

NEXT = {"a": "b", "b": "c", "c": "straddle", "straddle": "dense", "dense": "a"}


@pytest.fixture(scope="module")
def uploaded(backend):
    """name -> (device input whose initial tree is that memory's and whose final tree is the next one's), the reference trees"""
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


def _same_as_reference(backend, open_fn, ref, addresses):
    o, root = open_fn(addresses)
    a = sorted(set(int(x) for x in addresses))
    words, values, counts = ref_set(ref, a)
    assert root == ref.root
    assert o.addresses.tolist() == a and o.counts == counts
    assert o.siblings.tolist() == words
    assert o.values.shape == (len(a), 4) and np.array_equal(o.values, values)
    assert verify_set(root, o, backend.L, with_root=True) == (True, root)
    assert verify_set_host(root, o, backend.L) == (0, "")
    return o, root


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_sets_of_uploaded_trees_equal_the_reference(backend, uploaded, i):
    name, a = SETS[i]
    ref = uploaded[1][name]
    for dev, which in _where(uploaded, name):                                     # as an initial and as a final tree
        o, root = _same_as_reference(backend, lambda x: backend.open_memory_set(dev, which, x), ref, a)
        again, root_again = backend.open_memory_set(dev, which, a[::-1] + a[:1])   # any order, any repeats: the same bytes
        assert root_again == root and again.siblings.tobytes() == o.siblings.tobytes() and again.values.tobytes() == o.values.tobytes()
        assert again.addresses.tobytes() == o.addresses.tobytes()


def test_sets_agree_with_the_single_and_the_range_openings(backend, uploaded):
    # n = 1: siblings[0 .. 27] of the single opening
    for name, a in SETS:
        if len(a) != 1:
            continue
        dev, which = _where(uploaded, name)[0]
        o, root = backend.open_memory_set(dev, which, a)
        single, single_root = backend.open_memory(dev, which, a)
        assert single_root == root and o.siblings.tolist() == list(single[0].siblings) and o.values[0].tolist() == list(single[0].value)
    # a contiguous set: per depth the used left / right slots of the range record, and the same values
    name, a = SETS[CONTIGUOUS]
    dev, which = _where(uploaded, name)[1]
    o, root = backend.open_memory_set(dev, which, a)
    rec, values, range_root = backend.open_memory_range(dev, which, a[0], len(a))
    want = []
    for k in range(N_DEPTHS):
        want += [rec.left[k]] * ((a[0] >> k) & 1) + [rec.right[k]] * (1 - ((a[-1] >> k) & 1))
    assert range_root == root and o.siblings.tolist() == want and np.array_equal(o.values, values)
    # a mixed set: every word is siblings[k] of the single opening of an address under that node
    for name, a in (SETS[MIXED], SETS[7]):
        dev, which = _where(uploaded, name)[0]
        o, root = backend.open_memory_set(dev, which, a)
        single, _ = backend.open_memory(dev, which, a)
        q = 0
        for k in range(N_DEPTHS):
            nodes = sorted({x >> k for x in a})
            for x in nodes:
                if x ^ 1 not in nodes:
                    j = next(j for j, y in enumerate(a) if y >> k == x)
                    assert o.siblings[q] == single[j].siblings[k], (k, x)
                    q += 1
            assert q == sum(o.counts[:k + 1])
        assert q == o.siblings.size


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_each_tamper_is_a_verdict_of_the_gpu_and_of_the_host(backend, uploaded, i):
    name, a = SETS[i]
    dev, which = _where(uploaded, name)[0]
    o, root = backend.open_memory_set(dev, which, a)
    assert verify_set(root, o, backend.L) and verify_set_host(root, o, backend.L)[0] == 0
    cases = tampers(o.addresses, o.values, o.siblings, root)
    assert len(cases) == (14 if len(a) > 1 else 12)
    for what, (ta, tv, tw, tr, needle) in cases.items():
        t = MemSetOpening(ta, tv, tw)
        gpu, got = verify_set(tr, t, backend.L, with_root=True)                   # status 0: a verdict, never a failure
        rc, msg = verify_set_host(tr, t, backend.L)
        assert gpu is False and rc == 11 and needle in msg, (what, gpu, rc, msg)
        if what == "root + 1":
            assert got == root                                                    # well formed: it folds to the true root
    # an empty set is a verdict too
    ok, got = C.c_uint8(7), C.c_uint32(7)
    one = (C.c_uint32 * 4)()
    assert backend.L.cm_verify_memory_set(C.c_uint32(root), one, C.c_uint64(0), one, one, C.c_uint32(0), C.byref(ok), C.byref(got), C.c_uint64(0)) == 0
    assert (ok.value, got.value) == (0, 0)


def test_refusals_write_nothing_and_leave_the_input_usable(backend, uploaded):
    dev, which = _where(uploaded, "a")[0]
    ref = uploaded[1]["a"]
    L = backend.L
    live = backend.mem_stats().live_bytes
    S = 0xABABABAB

    def call(addresses, n=None, w=which, cap=64, values=True, siblings=True, need=True, root=True, d=dev):
        a = np.array([0] if addresses is None else addresses, dtype=np.uint32)
        v, s, m, r = (C.c_uint32 * 16)(*[S] * 16), (C.c_uint32 * 64)(*[S] * 64), C.c_uint32(S), C.c_uint32(S)
        rc = L.cm_input_open_memory_set(d, C.c_uint32(w), a.ctypes.data_as(C.POINTER(C.c_uint32)) if addresses is not None else None,
                                        C.c_uint64(len(a) if n is None else n), v if values else None, s if siblings else None, C.c_uint32(cap),
                                        C.byref(m) if need else None, C.byref(r) if root else None)
        buf = C.create_string_buffer(512)
        L.cm_last_error(buf, C.c_size_t(512))
        assert list(v) == [S] * 16 and list(s) == [S] * 64 and r.value == S   # nothing written to values, siblings or root
        return rc, buf.value.decode(), m.value

    for kw, needle in ((dict(addresses=None, n=1), "null"), (dict(addresses=[5], values=False), "null"), (dict(addresses=[5], siblings=False), "null"),
                       (dict(addresses=[5], need=False), "null"), (dict(addresses=[5], root=False), "null"), (dict(addresses=[5], d=None), "null"),
                       (dict(addresses=[5], n=0), "no cells"), (dict(addresses=[5], n=(1 << 20) + 1), "split the set"),
                       (dict(addresses=[5, SPACE]), "address 1 is beyond the address space"),
                       (dict(addresses=[4, 5, 5, 6]), "address 2 is not above address 1"), (dict(addresses=[4, 6, 5]), "address 2 is not above address 1"),
                       (dict(addresses=[5], w=2), "`which`")):
        rc, msg, m = call(**kw)
        assert rc == 1 and needle in msg and m == S, (kw, rc, msg, m)
    rc, msg, m = call([4, 6], cap=27)                                             # the need is reported with the refusal
    assert rc == 1 and m == 28 and "room for 27 sibling words where the set needs 28" in msg, (rc, msg, m)
    big = MemSetOpening([5], np.zeros((1, 4), dtype=np.uint32), np.zeros(28, dtype=np.uint32))
    ok = C.c_uint8(7)
    a1 = (C.c_uint32 * 4)(5)
    assert L.cm_verify_memory_set(C.c_uint32(0), a1, C.c_uint64((1 << 20) + 1), a1, a1, C.c_uint32(28), C.byref(ok), None, C.c_uint64(0)) == 1
    assert L.cm_verify_memory_set(C.c_uint32(0), None, C.c_uint64(1), a1, a1, C.c_uint32(28), C.byref(ok), None, C.c_uint64(0)) == 1
    assert L.cm_verify_memory_set(C.c_uint32(0), a1, C.c_uint64(1), a1, a1, C.c_uint32(28), None, None, C.c_uint64(0)) == 1 and ok.value == 7
    assert verify_set(0, big, L) is False
    _same_as_reference(backend, lambda x: backend.open_memory_set(dev, which, x), ref, [4, 6])   # the input is as usable as before
    assert backend.mem_stats().live_bytes == live                                 # every buffer of the calls went back to the pool

    empty = backend.run_begin(np.zeros((0, 4), dtype=np.uint32), np.zeros((0, 4), dtype=np.uint32), [0, 0, 0, 0, 0, 0])
    with pytest.raises(CmError) as e:
        empty.open_set([0])
    assert "status 1:" in str(e.value) and "empty" in str(e.value), str(e.value)
    empty.free()


@pytest.mark.parametrize("device_trees", [False, True])
def test_write_set_of_an_adapted_segment_under_both_tree_builders(backend, monkeypatch, device_trees):
    """300 cells: below the 2048-row cut-over the adapter hashes its trees on the host; CM_ADAPTER_DEVICE_TREE_MIN=1 sends them
    through the device builder.  The set reads either node list.  Opened under the initial and under the final tree, the write
    set has the same sibling words, and folding them with the final values gives the final root."""
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    prog = scatter_store_program(300)
    hi, hs = vm_run(prog), vm_segment(prog)
    dev = backend.adapt_segment(hs)
    a = prover_input_arrays(hi.view)
    refs, cells = [], []
    for which, key in ((0, "initial_memory"), (1, "final_memory")):
        rows = [tuple(int(x) for x in r[:5]) for r in a[key]]
        refs.append(RefTree(rows))
        cells.append({r[0]: r[1:] for r in rows})
        assert refs[which].root == a["roots"][which]                              # the reference tree IS the input's tree
    touched = sorted(refs[1].present)
    mixed = touched[::7] + [touched[-1] + 1, touched[-1] + 3, 1 << 27, SPACE - 1]   # touched and untouched cells
    for which in (0, 1):
        _same_as_reference(backend, lambda x: backend.open_memory_set(dev, which, x), refs[which], mixed)
    zero = (0, 0, 0, 0)
    written = sorted(x for x in set(cells[0]) | set(cells[1]) if cells[0].get(x, zero) != cells[1].get(x, zero))
    assert written and set(written) <= set(touched)                               # (the loop's own variables: the stores go to fresh cells)
    before, root0 = _same_as_reference(backend, lambda x: backend.open_memory_set(dev, 0, x), refs[0], written)
    after, root1 = _same_as_reference(backend, lambda x: backend.open_memory_set(dev, 1, x), refs[1], written)
    assert root0 != root1 and before.siblings.tobytes() == after.siblings.tobytes()
    assert not np.array_equal(before.values, after.values)
    assert set_root(before, lib=backend.L) == root0 and set_root(before, after.values, backend.L) == root1
    moved = MemSetOpening(before.addresses, after.values, before.siblings)
    assert verify_set(root1, moved, backend.L, with_root=True) == (True, root1)
    assert verify_set(root0, moved, backend.L, with_root=True) == (False, root1)
    backend.free_input(dev)
    hi.free(); hs.free()


def test_run_sets_follow_the_image_and_share_its_tree(backend):
    hss = _heap_run()
    run = Run.from_segment(backend, hss[0])
    dev0 = run.adapt_next(hss[0])
    lo, hp = run.memory()
    n_lo, n_hi = lo.shape[0], hp.shape[0]
    assert n_lo > 0 and n_hi > 0
    ref0 = RefTree(image_cells(lo, hp))
    # locals, the gap behind them, the middle of the address space, the gap in front of the heap, the heap
    span = list(range(n_lo)) + [n_lo, n_lo + 5, 1 << 27, SPACE - n_hi - 1] + list(range(SPACE - n_hi, SPACE))
    idle = backend.mem_stats().live_bytes
    old, root0 = _same_as_reference(backend, run.open_set, ref0, span)
    with_tree = backend.mem_stats().live_bytes
    assert with_tree > idle                                                       # the cached image tree, and nothing else:
    single, single_root = run.open([n_lo])
    _, _, range_root = run.open_range(0, n_lo)
    assert single_root == range_root == root0 and backend.mem_stats().live_bytes == with_tree   # one tree serves the three calls
    p0 = backend.prove_device(dev0)
    assert p0.public_data()["final_root"] == root0
    dev1 = run.adapt_next(hss[1])
    p1 = backend.prove_device(dev1)
    lo1, hp1 = run.memory()
    ref1 = RefTree(image_cells(lo1, hp1))
    fresh, root1 = _same_as_reference(backend, run.open_set, ref1, span)
    assert root1 == p1.public_data()["final_root"] and root1 != root0
    assert not np.array_equal(fresh.values, old.values)                           # a cell of the set changed with the advance
    assert verify_set(root0, old, backend.L) and not verify_set(root1, old, backend.L)
    assert verify_set_host(root1, old, backend.L)[0] == 11
    for p in (p0, p1):
        p.free()
    for d in (dev0, dev1):
        backend.free_input(d)
    run.free()
    for hs in hss:
        hs.free()
