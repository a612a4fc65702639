"""A whole run (header revision 10): cm_run keeps the program's memory on the device from segment to segment, cm_prove_run proves
the segments behind one serial adapter, cm_verify_run checks the chain.

Reference for every comparison: the host adapter (cm_vm_run / cm_synth_fibonacci) and the synthetic VM's own segments
(cm_vm_segment), which tests/test_adapter.py and tests/test_gpu_adapter.py pin — never the run path itself.

Two cases differ from the plain reading of "every run, cut, accepted":
  * `scatter_store_program(300, base=(1 << 27) + 12345)` ("wide") is run as ONE segment.  Its first write grows the synthetic
    VM's heap vector to 2^27 - 12345 cells (2 GiB; host_adapter.hpp VM::put grows the nearer vector), so the host reference of a
    second segment would need 1.3e8 map entries and two 5e8-leaf trees.  The carried image with 28-bit addresses across links is
    covered by "high": the same program with its base 400 cells below MAX_ADDRESS, cut in 3, whose heap grows by a few hundred
    cells.
  * `cm_verify_run` answers what the HOST adapter's registers and roots predict, for every run.  That is "accept" for all but
    `scatter_store_program(3000)` cut in 4 (and "high"): a segment that first-writes cells beyond the memory it was handed gives
    them the written value as initial value (adapter/memory.rs:493-503, restated as is; tests/test_gpu_ref_cases.py::
    test_hash_continuity_with_max_steps_10), so its initial root is not its predecessor's final root and the named refusal is
    the right answer."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, Run, prover_input_arrays, run_segment, runner_segment_arrays, segment_end_lengths,
                             synth_fibonacci, synth_fibonacci_segment, verify_run, vm_run, vm_segment)
from tests.test_gpu_adapter import _same, scatter_store_program

pytestmark = pytest.mark.gpu


def _steps(prog, **kw):
    h = vm_run(prog, **kw)
    n = h.steps
    h.free()
    return n


def _cut(prog, parts, **kw):
    return -(-_steps(prog, **kw) // parts)


def _runs():
    from tests.casm_fixtures import heap_program
    from tests.test_oracle_air import CHAIN_PROG, u32_loop_program
    hp, hentry, hnret, _ = heap_program()
    wide = scatter_store_program(300, base=(1 << 27) + 12345)
    high = scatter_store_program(300, base=(1 << 28) - 1 - 400)
    big = scatter_store_program(3000)
    u32 = u32_loop_program(50)

    def vm(prog, **kw):
        return (lambda s, ms: vm_run(prog, max_steps=ms, segment=s, **kw)), (lambda s, ms: vm_segment(prog, max_steps=ms, segment=s, **kw))
    return {
        "chain": vm(CHAIN_PROG) + (2, 4),
        "heap": vm(hp, entry_pc=hentry, n_returns=hnret) + (8, None),
        "scatter3000": vm(big) + (_cut(big, 4), 4),
        "wide": vm(wide) + (1 << 30, 1),
        "high": vm(high) + (_cut(high, 3), 3),
        "u32_loop": vm(u32) + (_cut(u32, 5), 5),
        "fibonacci": ((lambda s, ms: synth_fibonacci(1000, max_steps=ms, segment=s)),
                      (lambda s, ms: synth_fibonacci_segment(1000, max_steps=ms, segment=s)), 1500, 7),
    }


RUN_NAMES = ["chain", "heap", "scatter3000", "wide", "high", "u32_loop", "fibonacci"]
MUST_CHAIN = ["chain", "heap", "wide", "u32_loop", "fibonacci"]     # (the host adapter agrees: asserted below)


def _segments(name):
    """[(HostInput, HostSegment)] of every segment of the run"""
    mk_input, mk_segment, max_steps, n_expected = _runs()[name]
    first = mk_segment(0, max_steps)
    n = getattr(first, "n_segments", None) or n_expected
    first.free()
    assert n_expected is None or n == n_expected, (name, n)
    return [(mk_input(s, max_steps), mk_segment(s, max_steps)) for s in range(n)]


def _free(segs):
    for hi, hs in segs:
        hi.free(); hs.free()


def _expected_chain_answer(segs):
    """what cm_verify_run has to say, from the host adapter's own registers and roots"""
    a = [prover_input_arrays(hi.view) for hi, _ in segs]
    for i in range(1, len(a)):
        for field, x, y in (("pc", a[i]["regs"][0], a[i - 1]["regs"][2]), ("fp", a[i]["regs"][1], a[i - 1]["regs"][3]),
                            ("root", a[i]["roots"][0], a[i - 1]["roots"][1])):
            if x != y:
                return f"run: segment {i} initial_{field} != segment {i - 1} final_{field}"
    return ""


def _same_inputs_and_images(backend, segs):
    run = Run.from_segment(backend, segs[0][1])
    try:
        for k, (hi, hs) in enumerate(segs):
            dev = run.adapt_next(hs)
            back = backend.download_input(dev)
            _same(prover_input_arrays(hi.view), prover_input_arrays(back.view))
            back.free()
            backend.free_input(dev)
            if k + 1 < len(segs):
                lo, hp = run.memory()
                want = runner_segment_arrays(segs[k + 1][1].view)
                assert lo.shape == want["initial_memory"].shape and hp.shape == want["initial_heap"].shape, (k, lo.shape, hp.shape)
                assert np.array_equal(lo, want["initial_memory"]) and np.array_equal(hp, want["initial_heap"]), k
            else:
                assert run.lengths() == segment_end_lengths(hs)
    finally:
        run.free()


def _check_run(backend, oracle, name):
    segs = _segments(name)
    _same_inputs_and_images(backend, segs)
    hss = [hs for _, hs in segs]
    want = backend.prove_many_segments(hss, inflight=2)
    got = backend.prove_run(hss, inflight=2)
    assert len(got) == len(want) == len(segs)
    for k, (p, q) in enumerate(zip(got, want)):
        assert np.array_equal(p.words(), q.words()), (name, k)
    if name == "heap":
        for k, (hi, _) in enumerate(segs):
            words, _ = oracle.prove(hi.view)
            assert np.array_equal(got[k].words(), words), k
    rc, msg = verify_run(got)
    expect = _expected_chain_answer(segs)
    print(name, "segments", len(segs), "verify_run:", rc, msg, "| host adapter predicts:", expect or "accept")
    assert (rc, msg) == ((0, "") if not expect else (11, expect))
    if name in MUST_CHAIN:
        assert rc == 0
    # public data through the ABI = the input's scalars
    for (hi, _), p in zip(segs, got):
        a, pd = prover_input_arrays(hi.view), p.public_data()
        assert [pd["initial_pc"], pd["initial_fp"], pd["final_pc"], pd["final_fp"]] == a["regs"]
        assert [pd["initial_root"], pd["final_root"]] == a["roots"] and pd["clock"] == hi.steps
    for p in got + want:
        p.free()
    _free(segs)


@pytest.mark.parametrize("name", RUN_NAMES)
def test_run_matches_the_segment_adapter(backend, oracle, name):
    """Same input (every array of every segment), same image after every segment, same proofs as cm_prove_many_segments, and
    cm_verify_run answers what the host adapter's registers and roots predict."""
    _check_run(backend, oracle, name)


@pytest.mark.parametrize("name", RUN_NAMES)
def test_run_with_device_trees_for_small_memories(backend, oracle, monkeypatch, name):
    """CM_ADAPTER_DEVICE_TREE_MIN=1: the run path leaves the small-memory cut-over and hashes its trees on the device from the
    device-built leaves; inputs, images and proofs still equal the segment adapter's."""
    monkeypatch.setenv("CM_ADAPTER_DEVICE_TREE_MIN", "1")
    _check_run(backend, oracle, name)


def test_a_run_is_continued_by_later_calls(backend):
    """cm_prove_run, then cm_run_adapt_next, then cm_prove_run again on one run: the proofs are those of the segment adapter"""
    segs = _segments("u32_loop")
    hss = [hs for _, hs in segs]
    want = backend.prove_many_segments(hss, inflight=2)
    run = Run.from_segment(backend, hss[0])
    got = run.prove(hss[:2], inflight=2)
    dev = run.adapt_next(hss[2])
    got.append(backend.prove_device(dev))
    backend.free_input(dev)
    got += run.prove(hss[3:], inflight=1)
    assert len(got) == len(want) == 5
    for k, (p, q) in enumerate(zip(got, want)):
        assert np.array_equal(p.words(), q.words()), k
    assert verify_run(got) == (0, "")
    assert run.lengths() == segment_end_lengths(hss[-1])
    run.free()
    for p in got + want:
        p.free()
    _free(segs)


def test_prove_run_error_contract(backend):
    """a segment that cannot be adapted fails the call with its status and message, the segments before it are proved, nothing
    behind it is started, the image stays at that segment's start, and the run goes on from there"""
    segs = _segments("u32_loop")
    hss = [hs for _, hs in segs]
    want = backend.prove_many_segments(hss, inflight=2)
    run = Run.from_segment(backend, hss[0])
    items = [run_segment(hs) for hs in hss]
    items[2] = run_segment(hss[2], n_memory_end=1)                            # below the current length: status 1
    with pytest.raises(CmError) as e:
        run.prove(items, inflight=2)
    assert "status 1:" in str(e.value) and "below its current length" in str(e.value), str(e.value)
    partial = e.value.partial
    assert [p is not None for p in partial] == [True, True, False, False, False]
    start2 = runner_segment_arrays(hss[2].view)
    lo, hp = run.memory()
    assert np.array_equal(lo, start2["initial_memory"]) and np.array_equal(hp, start2["initial_heap"])
    got = partial[:2] + run.prove(hss[2:], inflight=2)
    for k, (p, q) in enumerate(zip(got, want)):
        assert np.array_equal(p.words(), q.words()), k
    run.free()
    for p in got + want:
        p.free()
    _free(segs)


def test_chain_refusals(backend):
    from tests.test_oracle_air import u32_loop_program
    segs = _segments("chain")
    proofs = backend.prove_run([hs for _, hs in segs], inflight=2)
    assert verify_run(proofs) == (0, "")
    assert verify_run(proofs[:1]) == (0, "")                                   # n = 1: nothing to chain
    swapped = [proofs[0], proofs[2], proofs[1], proofs[3]]
    rc, msg = verify_run(swapped)
    assert rc == 11 and msg == "run: segment 1 initial_pc != segment 0 final_pc", msg
    other = vm_segment(u32_loop_program(50))
    foreign = backend.prove_run([other], inflight=1)[0]
    rc, msg = verify_run([proofs[0], foreign, proofs[2], proofs[3]])
    assert rc == 11 and msg == "run: segment 1 initial_pc != segment 0 final_pc", msg     # (it starts at pc 0, segment 0 stopped at pc 2)
    foreign.free(); other.free()
    for p in proofs:
        p.free()
    _free(segs)


def test_input_refusals_leave_the_run_usable(backend):
    """the three status-1 cases of cm_run_adapt_next; after each the image is what it was and the segment still adapts"""
    prog = scatter_store_program(40)
    hi, hs = vm_run(prog), vm_segment(prog)
    run = Run.from_segment(backend, hs)
    lo0, hp0 = run.memory()
    n_mem_end, n_heap_end = segment_end_lengths(hs)
    assert n_mem_end > lo0.shape[0]                                          # the program writes beyond the memory it starts with
    cases = {
        "not zero": run_segment(hs, n_memory_end=lo0.shape[0]),              # a written cell left outside both regions
        "below its current length": run_segment(hs, n_memory_end=lo0.shape[0] - 1),
        "overlap": run_segment(hs, n_heap_end=(1 << 28) - n_mem_end + 1),
    }
    for needle, seg in cases.items():
        with pytest.raises(CmError) as e:
            run.adapt_next(seg)
        assert "status 1:" in str(e.value) and needle in str(e.value), str(e.value)
        lo, hp = run.memory()
        assert np.array_equal(lo, lo0) and np.array_equal(hp, hp0), needle
    dev = run.adapt_next(hs)
    back = backend.download_input(dev)
    _same(prover_input_arrays(hi.view), prover_input_arrays(back.view))
    back.free(); backend.free_input(dev)
    assert run.memory()[0].shape[0] == n_mem_end
    run.free(); hi.free(); hs.free()


def test_image_is_counted_and_returned(backend):
    backend.pool_trim()
    start = backend.mem_stats().live_bytes
    lo = np.zeros((1 << 16, 4), dtype=np.uint32)
    lo[0] = [11, 0, 0, 0]                                                    # (a ret at pc 0: never executed here)
    run = backend.run_begin(lo, np.zeros((1 << 12, 4), dtype=np.uint32), [0, 1, 1, 1, 1, 1])
    live = backend.mem_stats().live_bytes
    assert live - start >= ((1 << 16) + (1 << 12)) * 16, (start, live)
    got_lo, got_hp = run.memory()
    assert np.array_equal(got_lo, lo) and got_hp.shape == (1 << 12, 4)
    run.free()
    backend.pool_trim()
    assert backend.mem_stats().live_bytes == start
