"""A whole run checked on the GPU before it is proved: cm_link_diff (which cells break a link), cm_check_run / cm_check_chain
(every segment's AIR verdict and every link in one call).

References: tests/link_diff_ref.py (numpy, from the cm_memory_cell rows alone) for the cells, cm_check_constraints on the segment
adapter's input for the AIR reports, cm_verify_run on the proved run for the link verdicts and their words."""
import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, Run, check_chain, link_diff, prover_input_arrays, run_segment, runner_segment_arrays,
                             verify_run, vm_run, vm_segment)
from tests.link_diff_ref import link_diff_ref
from tests.test_gpu_adapter import scatter_store_program

pytestmark = pytest.mark.gpu
P = (1 << 31) - 1
SIZES = (0, 1, 63, 64, 65, 1025)       # one row, both sides of a wave / of a 64-row boundary, more than one 256-row block plus one


# ---- 1. op level -----------------------------------------------------------------------------------------------------------
def _rows(n_prev, n_next, mutate, seed):
    """(prev final rows, next initial rows): the same cells on both sides, then — with `mutate` — differences of every kind at the
    first row, the last common row and both sides of the 64-row boundary, and zero-valued cells on one side only"""
    rng = np.random.default_rng(seed)
    n = max(n_prev, n_next)
    rows = np.zeros((n, 7), dtype=np.uint32)
    rows[:, 0] = 3 * np.arange(n, dtype=np.uint32) + 5
    rows[:, 1:5] = rng.integers(1, P, size=(n, 4), dtype=np.uint32)
    rows[:, 5] = rng.integers(0, 1 << 20, size=n, dtype=np.uint32)
    rows[:, 6] = 1
    a, b = rows[:n_prev].copy(), rows[:n_next].copy()
    b[:, 5] = 0                                                   # (clocks and multiplicities are not leaves: never a difference)
    b[:, 6] = P - 1
    if not mutate:
        return a, b
    common = min(n_prev, n_next)
    for r in (0, common - 1, 63, 64):                             # kind 1
        if 0 <= r < common:
            b[r, 1 + r % 4] = (int(b[r, 1 + r % 4]) + 1) % P
    for r in (1, 62, 65, common - 2):                             # kind 3 and kind 2 on neighbouring addresses
        if 2 <= r + 1 < common:
            a[r, 0] += 1
    for r in (2, 66):                                             # zero-only on prev's side, kind 2 on next's
        if r < common - 1:
            a[r, 0] += 1
            a[r, 1:5] = 0
    for arr, k in ((a, n_next), (b, n_prev)):                     # tails: present on one side only, some of them all zero
        if len(arr) > k:
            arr[k::3, 1:5] = 0
    return a, b


def _upload(backend, keep, **arrays):
    inp = ArrayInput(arrays)
    keep.append(inp)
    return backend.upload_input(inp)


@pytest.mark.parametrize("n_prev", SIZES)
def test_link_diff_equals_the_numpy_reference(backend, n_prev):
    for n_next in SIZES:
        for mutate in ((True, False) if n_prev == n_next else (True,)):
            a, b = _rows(n_prev, n_next, mutate, seed=1000 * n_prev + n_next)
            want, totals = link_diff_ref(a, b)
            keep = []
            prev = _upload(backend, keep, final_memory=a, regs=[0, 0, 9, 4], roots=[1, 7])
            nxt = _upload(backend, keep, initial_memory=b, regs=[9, 5, 0, 0], roots=[7, 2])
            tag = (n_prev, n_next, mutate)
            for cap in sorted({len(want) + 3, 0, 1, max(len(want) - 1, 0)}):
                d = link_diff(prev, nxt, cap, lib=backend.L)
                r = d.report
                assert d.n_total == len(want) == r.n_total, (tag, cap, d.n_total, len(want))
                assert np.array_equal(d.cell_words(), want[:cap]), (tag, cap)
                assert d.truncated == (cap < len(want))
                got_totals = {k: getattr(r, k) for k in totals}
                assert got_totals == totals, (tag, got_totals, totals)
                assert (r.pc_equal, r.fp_equal, r.roots_equal) == (1, 0, 1)
                assert (r.prev_final_pc, r.prev_final_fp, r.next_initial_pc, r.next_initial_fp) == (9, 4, 9, 5)
                assert (r.prev_final_root, r.next_initial_root) == (7, 7)
                assert r.first_sentence == "run: segment 1 initial_fp != segment 0 final_fp"
                assert (". %d cells differ: " % len(want) in r.message) == (len(want) > 0), r.message
            if not mutate:
                assert len(want) == 0 and totals["n_zero_only"] == 0
            backend.free_input(prev); backend.free_input(nxt)
    if n_prev == 1025:                                            # every kind and the zero-only rule were exercised
        a, b = _rows(1025, 1025, True, seed=1)
        _, totals = link_diff_ref(a, b)
        assert all(totals[k] > 0 for k in totals), totals


def test_link_diff_refuses_unsorted_rows_and_a_short_struct(backend):
    a, _ = _rows(65, 65, False, seed=3)
    bad = a.copy()
    bad[[10, 11]] = bad[[11, 10]]
    keep = []
    prev, nxt = _upload(backend, keep, final_memory=a), _upload(backend, keep, initial_memory=bad)
    with pytest.raises(CmError) as e:
        link_diff(prev, nxt, 8, lib=backend.L)
    assert "status 1:" in str(e.value) and "ascending address order" in str(e.value)
    import ctypes as C
    from cairo_m_amd.lib import LinkReport
    rep, n = LinkReport(), C.c_uint64(0)                           # struct_size left at 0
    assert backend.L.cm_link_diff(prev, prev, C.byref(rep), None, C.c_uint64(0), C.byref(n)) == 1
    backend.free_input(prev); backend.free_input(nxt)


# ---- runs ------------------------------------------------------------------------------------------------------------------
def _segments(prog, parts=None, max_steps=None, **kw):
    if max_steps is None:
        h = vm_run(prog, **kw)
        max_steps = -(-h.steps // parts)
        h.free()
    first = vm_segment(prog, max_steps=max_steps, segment=0, **kw)
    n = first.n_segments
    first.free()
    assert parts is None or n == parts
    return [vm_segment(prog, max_steps=max_steps, segment=s, **kw) for s in range(n)]


def _adapter_arrays(backend, hss):
    """the segment adapter's inputs, downloaded: one dict of arrays per segment"""
    out = []
    for hs in hss:
        dev = backend.adapt_segment(hs)
        back = backend.download_input(dev)
        out.append(prover_input_arrays(back.view))
        back.free(); backend.free_input(dev)
    return out


def test_scatter_store_run_names_the_cells_of_every_broken_link(backend):
    hss = _segments(scatter_store_program(300), parts=3)
    rc = backend.check_run(hss, cap=256)
    arrays = _adapter_arrays(backend, hss)
    proofs = backend.prove_run(hss, inflight=1)
    assert verify_run(proofs) == (11, "run: segment 1 initial_root != segment 0 final_root")
    assert not rc.ok and rc.summary.startswith("link 1: run: segment 1 initial_root != segment 0 final_root. ")
    assert rc.segments[0].link is None
    for i in (1, 2):
        seg = rc.segments[i]
        assert seg.check.status == 0, seg.check.message
        rep = seg.link.report
        assert rep.roots_equal == 0 and rep.pc_equal == 1 and rep.fp_equal == 1
        assert [rep.prev_final_root, rep.next_initial_root] == [arrays[i - 1]["roots"][1], arrays[i]["roots"][0]]
        want, totals = link_diff_ref(arrays[i - 1]["final_memory"], arrays[i]["initial_memory"])
        assert 0 < len(want) <= 256 and seg.link.n_total == len(want)
        assert np.array_equal(seg.link.cell_words(), want), i
        assert {k: getattr(rep, k) for k in totals} == totals
        # the words of cm_verify_run for this link (it numbers the pair it is given 0 and 1)
        assert verify_run(proofs[i - 1:i + 1]) == (11, "run: segment 1 initial_root != segment 0 final_root")
        assert rep.first_sentence == f"run: segment {i} initial_root != segment {i - 1} final_root"
        assert rep.message.endswith(f"; first address {want[0, 1]}")
    # the same links from inputs adapted one by one
    devs = [backend.adapt_segment(hs) for hs in hss]
    chain = check_chain(devs, cap=256, lib=backend.L)
    assert chain.summary == rc.summary and chain.segments[0].check is None
    for i in (1, 2):
        assert bytes(chain.segments[i].link.report) == bytes(rc.segments[i].link.report)
        assert np.array_equal(chain.segments[i].link.cell_words(), rc.segments[i].link.cell_words())
    for d in devs:
        backend.free_input(d)
    for p in proofs:
        p.free()
    for hs in hss:
        hs.free()


@pytest.mark.parametrize("name", ["chain", "high"])
def test_runs_that_chain_pass_and_leave_the_image_of_adapt_next(backend, name):
    from tests.test_oracle_air import CHAIN_PROG
    if name == "chain":
        hss = _segments(CHAIN_PROG, max_steps=2)
        assert len(hss) == 4
    else:
        hss = _segments(scatter_store_program(300, base=(1 << 28) - 1 - 400), parts=3)
    run = Run.from_segment(backend, hss[0])
    rc = run.check(hss)
    proofs = backend.prove_run(hss, inflight=1)
    verdict = verify_run(proofs)
    assert verdict == (0, "")
    assert rc.ok and rc.summary == "" and len(rc.segments) == len(hss)
    for i, seg in enumerate(rc.segments):
        assert seg.check.status == 0 and seg.check.message == "", (i, seg.check.message)
        if i:
            rep = seg.link.report
            assert rep.ok and rep.message == "" and seg.link.n_total == 0 and seg.link.cells == []
            assert rep.prev_final_root == rep.next_initial_root
    other = Run.from_segment(backend, hss[0])
    for hs in hss:
        backend.free_input(other.adapt_next(hs))
    for got, want in zip(run.memory(), other.memory()):
        assert np.array_equal(got, want)
    run.free(); other.free()
    for p in proofs:
        p.free()
    for hs in hss:
        hs.free()


def test_an_unprovable_segment_is_reported_like_cm_check_constraints(backend):
    a = 0x12345678
    prog = [[23, a & 0xFFFF, a >> 16, 0], [23, 0, 0, 2], [18, 0, 2, 12, 14], [11]]      # u32 division by zero in the third step
    hss = _segments(prog, max_steps=2, entry_pc=0, args=(), n_returns=0)
    assert len(hss) == 2
    rc = backend.check_run(hss)
    alone = []
    for hs in hss:
        dev = backend.adapt_segment(hs)
        alone.append(backend.check(dev))
        backend.free_input(dev)
    assert [r.status for r in alone] == [0, 2] and alone[1].message == "U32StoreDivFpFp: constraint 13 fails on row 0"
    for i, (seg, want) in enumerate(zip(rc.segments, alone)):
        for field, _ in type(want)._fields_:
            x, y = getattr(seg.check, field), getattr(want, field)
            assert (x == y) if isinstance(x, (int, str)) else (bytes(x) == bytes(y)), (i, field)
        assert bytes(seg.check) == bytes(want), i
    assert not rc.ok and rc.summary == "segment 1: U32StoreDivFpFp: constraint 13 fails on row 0"
    assert rc.segments[1].link.report.ok
    for hs in hss:
        hs.free()


def test_a_refused_segment_ends_the_call_with_its_status(backend):
    hss = _segments(scatter_store_program(300), parts=3)
    run = Run.from_segment(backend, hss[0])
    items = [run_segment(hs) for hs in hss]
    items[1] = run_segment(hss[1], n_memory_end=1)                     # below the current length: status 1
    with pytest.raises(CmError) as e:
        run.check(items)
    assert "status 1:" in str(e.value) and "below its current length" in str(e.value), str(e.value)
    partial = e.value.partial
    assert len(partial.segments) == 1 and partial.segments[0].check.status == 0 and partial.segments[0].link is None
    start1 = runner_segment_arrays(hss[1].view)
    lo, hp = run.memory()
    assert np.array_equal(lo, start1["initial_memory"]) and np.array_equal(hp, start1["initial_heap"])
    rest = run.check(hss[1:])                                           # the run goes on from there
    assert [s.check.status for s in rest.segments] == [0, 0] and rest.segments[0].link is None
    assert rest.segments[1].link.report.roots_equal == 0
    run.free()
    for hs in hss:
        hs.free()


def test_a_check_leaves_nothing_but_the_image(backend):
    hss = _segments(scatter_store_program(300), parts=3)
    backend.pool_trim()
    base = backend.mem_stats().live_bytes
    other = Run.from_segment(backend, hss[0])
    for hs in hss:
        backend.free_input(other.adapt_next(hs))
    image = backend.mem_stats().live_bytes - base                       # the image after the same three segments
    other.free()
    assert image > 0 and backend.mem_stats().live_bytes == base
    run = Run.from_segment(backend, hss[0])
    rc = run.check(hss)
    assert len(rc.segments) == 3
    assert backend.mem_stats().live_bytes == base + image
    run.free()
    assert backend.mem_stats().live_bytes == base
    backend.check_run(hss)                                              # makes and frees its own run
    assert backend.mem_stats().live_bytes == base
    for hs in hss:
        hs.free()
