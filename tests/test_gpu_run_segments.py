"""The run path (cm_run_adapt_next: adapter_run.inc) on hand-built chained segments (tests/adapter_segments.py): every array of
every segment against the numpy reference of the same segment over the carried image, the public entries the device input holds
(cm_device_input_public_entries: k_run_public without a proof) against the entries derived from the reference's rows, the image
after every advance (cm_run_memory: k_run_advance, region growth) against the image computed in numpy, in both tree modes; the gap
ladder as the first segment of a run; the refusals, each leaving the image as it was.  No proofs."""
import numpy as np
import pytest

from cairo_m_amd.lib import CmError, Run, adapt_segment_host, prover_input_arrays
from tests import adapter_segments as S
from tests.test_gpu_adapter import _same

pytestmark = pytest.mark.gpu


def _adapt_next(backend, run, seg, n_lo_end, n_hi_end):
    a = seg.array_segment()
    dev = run.adapt_next(a.run_segment(n_lo_end, n_hi_end))
    back = backend.download_input(dev)
    out, pub = prover_input_arrays(back.view), backend.public_entries(dev)
    back.free()
    backend.free_input(dev)
    return out, pub


def _same_memory(run, lo, hi):
    got_lo, got_hi = run.memory()
    assert got_lo.shape == lo.shape and got_hi.shape == hi.shape, (got_lo.shape, got_hi.shape)
    assert np.array_equal(got_lo, lo) and np.array_equal(got_hi, hi)


@pytest.mark.parametrize("device_trees", [False, True], ids=["default", "device_trees"])
@pytest.mark.parametrize("n_segments,ranges", [(2, "public"), (3, "public"), (3, "empty")])
def test_chained_segments(backend, monkeypatch, n_segments, ranges, device_trees):
    if device_trees:
        monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    case = S.run_case(n_segments, ranges)
    run = Run(backend, case[0][0].image, case[0][0].heap, case[0][0].ranges)
    try:
        for k, (seg, n_lo_end, n_hi_end) in enumerate(case):
            ref = S.reference(seg)
            got, pub = _adapt_next(backend, run, seg, n_lo_end, n_hi_end)
            _same(ref, got)
            _same(S.public_entries(ref), pub)
            _same_memory(run, *S.image_after(seg, n_lo_end, n_hi_end))
    finally:
        run.free()


def test_gap_ladder_as_first_segment(backend):
    seg = S.gap_ladder()
    h = adapt_segment_host(seg.array_segment())
    want = prover_input_arrays(h.view)
    h.free()
    run = Run(backend, seg.image, seg.heap, seg.ranges)
    try:
        got, pub = _adapt_next(backend, run, seg, S.LADDER_END, S.LADDER_HEAP)
        # the boundary memory of a run holds what cm_adapt_segment_host's does: the image and the touched cells
        _same(want, got)
        _same(S.public_entries(want), pub)
        lo, hi = run.memory()
        assert lo.shape[0] == S.LADDER_END and hi.shape[0] == S.LADDER_HEAP
        fin = want["final_memory"]
        inside = fin[fin[:, 0] < S.LADDER_END]
        expect = np.zeros((S.LADDER_END, 4), dtype=np.uint32)
        expect[inside[:, 0]] = inside[:, 1:5]
        assert np.array_equal(lo, expect)
        top = fin[fin[:, 0] > S.MAX_ADDRESS - S.LADDER_HEAP]
        assert np.array_equal(hi[S.MAX_ADDRESS - top[:, 0]], top[:, 1:5]) and top.shape[0] == S.LADDER_HEAP
    finally:
        run.free()


def _refused(backend, run, seg, ends, needle):
    lo0, hi0 = run.memory()
    with pytest.raises(CmError, match=needle) as e:
        _adapt_next(backend, run, seg, *ends)
    assert "status 1:" in str(e.value)
    _same_memory(run, lo0, hi0)


def test_refusals_leave_the_image_unchanged(backend):
    rng = np.random.default_rng(4)
    image, heap = S._values(rng, 12), S._values(rng, 3)
    v = lambda: S._values(rng, 1)[0]
    ok = S.build([(0, 1, [9, 5, 6], [(5, v())]), (1, 1, [4, 1, 2, 3], [(14, np.zeros(4, dtype=np.int64)), (S.MAX_ADDRESS - 1, v())])], image, heap)
    run = Run(backend, ok.image, ok.heap, ok.ranges)
    try:
        # a touched cell that is outside both regions when the segment ends and is not zero
        bad = S.build([(0, 1, [9, 5, 6], [(5, v())]), (1, 1, [4, 1, 2, 3], [(14, v()), (S.MAX_ADDRESS - 1, v())])], ok.image, ok.heap)
        _refused(backend, run, bad, (12, 3), "not zero")
        # an address beyond MAX_ADDRESS
        bad = S.build([(0, 1, [9, 5, 6], [(5, v())]), (1, 1, [4, 1, 2, 3], [(S.MAX_ADDRESS + 1, v()), (7, v())])], ok.image, ok.heap)
        _refused(backend, run, bad, (12, 3), "beyond MAX_ADDRESS")
        # every input error of the segment adapter
        for name, (seg, needle) in sorted(S.refusals().items()):
            r2 = Run(backend, seg.image, seg.heap, seg.ranges)
            try:
                _refused(backend, r2, seg, (40, 0), needle)
            finally:
                r2.free()
        # the run goes on: the good segment adapts from the unchanged image
        ref = S.reference(ok)
        got, pub = _adapt_next(backend, run, ok, 12, 3)
        _same(ref, got)
        _same_memory(run, *S.image_after(ok, 12, 3))
    finally:
        run.free()


@pytest.mark.parametrize("new_words", [(4, 1, 2, 3), (50, 1, 2)], ids=["other_size", "same_size"])
def test_rewritten_code_is_refused_by_name(backend, new_words):
    seg = S.rewritten_code(new_words)
    run = Run(backend, seg.image, seg.heap, seg.ranges)
    try:
        _refused(backend, run, seg, (40, 0), "logged opcode differs from the memory at segment start")
    finally:
        run.free()
