"""Device-memory accounting, estimate and budget on the GPU: a lone proof stays under cm_estimate_memory's bound and above the
floor of its committed LDE columns, the pool's counters agree with the driver, the per-phase peaks add up, and a budget lowers
the concurrency of cm_prove_many* and nothing else."""
import ctypes as C
import threading
import time
import os

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, Proof, estimate_memory, mem_reset_peak, mem_stats, set_memory_budget, synth_fibonacci,
                             synth_fibonacci_segment)

pytestmark = pytest.mark.gpu
GRANULE = 8 << 20     # what tests/test_gpu_prove.py::test_pool_trim_releases_parked_teardown allows the driver


def free_bytes(L):
    f, t = C.c_uint64(0), C.c_uint64(0)
    assert L.cm_device_mem_info(C.byref(f), C.byref(t)) == 0
    return f.value


def lde_floor(backend, dev, blowup):
    """4 B x sum over components of (trace + interaction columns) x 2^(log + blowup): trees 1 and 2 when the queries are answered"""
    total = 0
    for c in range(34):
        n_tr, n_it, _ = backend.component_info(c)
        total += 4 * (n_tr + n_it) << (backend.component_log_size(dev, c) + blowup)
    return total


CASES = [("fib20000", lambda: synth_fibonacci(20000), None),
         ("configs1", lambda: synth_fibonacci(100_000), None),
         ("metric", lambda: synth_fibonacci(419_000), None),
         ("continuation", lambda: synth_fibonacci(30, max_steps=100, segment=1), None),
         ("blowup2", lambda: synth_fibonacci(20000), (5, 2, 0, 12))]


@pytest.mark.parametrize("name,make,cfg", CASES, ids=[c[0] for c in CASES])
def test_lone_proof_is_under_the_bound_and_over_the_floor(backend, name, make, cfg):
    L = backend.L
    inp = make()
    backend.pool_trim()
    dev = backend.upload_input(inp)
    est = estimate_memory(view=inp.view, cfg=cfg, lib=L)
    logs = [backend.component_log_size(dev, c) for c in range(34)]
    assert estimate_memory(log_sizes=logs, cfg=cfg, lib=L).working_bytes == est.working_bytes
    try:
        for rep in range(2):     # from an empty pool (every block exact) and from a warm one (best-fit reuse, parked teardown)
            p = backend.prove_device(dev, cfg)
            m = p.memory()
            used = m.peak_live_bytes - m.start_live_bytes
            print(f"{name} rep {rep}: peak-start {used} working_bytes {est.working_bytes} ratio {est.working_bytes / max(used, 1):.3f} "
                  f"start {m.start_live_bytes} input {m.input_bytes} allocs {m.driver_allocs}")
            assert used <= est.working_bytes
            assert m.peak_live_bytes >= lde_floor(backend, dev, cfg[1] if cfg else 1)
            assert m.input_bytes == est.input_bytes
            p.free()
    finally:
        backend.free_input(dev)
        inp.free()
        backend.pool_trim()


def test_sharded_ranks_are_under_the_bound_per_rank(backend):
    from tests.test_gpu_sharded_threads import Loopback, LoopbackRank
    from cairo_m_amd.sharded import shard_plan
    world = 2
    inp = synth_fibonacci(30_000)
    est = estimate_memory(view=inp.view, world=world, lib=backend.L)
    _, words = shard_plan(inp, world, backend.L, None)
    shared = Loopback(backend, world, words, False)
    ranks = [LoopbackRank(shared, r) for r in range(world)]
    dev = backend.upload_input(inp)
    mem, err = [None] * world, [None] * world

    def work(r):
        h = C.c_void_p()
        rc = backend.L.cm_prove_sharded(dev, None, C.byref(ranks[r].c), C.byref(h))
        if rc != 0:
            err[r] = rc
            return
        pr = Proof(backend.L, h)
        m = pr.memory()
        mem[r] = (m.peak_live_bytes, m.start_live_bytes, m.n_phases)
        pr.free()
    ts = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    deadline = time.monotonic() + 120     # the threads' own teardown (streams, pool) runs while the OS thread exits
    while any(os.path.exists(f"/proc/self/task/{t.native_id}") for t in ts) and time.monotonic() < deadline:
        time.sleep(0.01)
    backend.free_input(dev)
    shared.free()
    inp.free()
    assert err == [None] * world, err
    for r in range(world):
        peak, start, n_phases = mem[r]
        print(f"world {world} rank {r}: peak-start {peak - start} working_bytes {est.working_bytes}")
        assert n_phases > 0 and 0 < peak - start <= est.working_bytes


def _report(L, p):
    m = p.memory()
    n = C.c_uint64(0)
    n_ms = L.cm_proof_stats(p.h, C.byref(n), C.byref(n), (C.c_double * 32)(), C.c_uint32(32))
    assert m.n_phases == n_ms > 0                         # same count as cm_proof_stats' phase_ms
    peaks = tuple(m.phase_peak_live_bytes[i] for i in range(m.n_phases))
    assert max(peaks) == m.peak_live_bytes and m.peak_reserved_bytes >= m.peak_live_bytes >= m.start_live_bytes
    assert set(p.stats()) >= {"cells", "steps", "phase_ms", "memory"}
    return (m.start_live_bytes, m.peak_live_bytes, m.peak_reserved_bytes, m.input_bytes, peaks), m.driver_allocs


def test_counters_agree_with_the_driver_and_phases_add_up(backend):
    L = backend.L
    inp = synth_fibonacci(20000)
    backend.pool_trim()
    r0, f0 = mem_stats(L).reserved_bytes, free_bytes(L)
    dev = backend.upload_input(inp)
    try:
        backend.prove_device(dev).free()          # (the thread's streams, pinned buffers and code objects exist from here on)
        backend.pool_trim()
        mem_reset_peak(L)
        rb, fb = mem_stats(L).reserved_bytes, free_bytes(L)
        p = backend.prove_device(dev)
        ra, fa = mem_stats(L).reserved_bytes, free_bytes(L)
        print(f"across one proof: reserved grew {ra - rb}, driver free dropped {fb - fa}, two-sided gap {(fb - fa) - (ra - rb)}")
        assert ra > rb and fb - fa >= (ra - rb) - GRANULE
        _report(L, p)
        p.free()
        backend.prove_device(dev).free()          # warm-up: from here every proof starts with its predecessor's parked blocks
        reports = []
        for _ in range(2):
            p = backend.prove_device(dev)
            rep, allocs = _report(L, p)
            print("driver_allocs of a repeated proof:", allocs)
            reports.append(rep)
            p.free()
        assert reports[0] == reports[1]
    finally:
        backend.free_input(dev)
        inp.free()
    backend.pool_trim()
    assert mem_stats(L).reserved_bytes == r0
    assert free_bytes(L) + GRANULE >= f0
    s = mem_stats(L)
    assert s.live_bytes <= s.reserved_bytes and s.pinned_host_bytes >= (32 << 20) and s.proofs_in_flight == 0


def _many(backend, kind, items, inflight):
    if kind == "device":
        return backend.prove_many(items, inflight=inflight)
    if kind == "host":
        return backend.prove_many_host(items, inflight=inflight)
    return backend.prove_many_segments(items, inflight=inflight)


@pytest.mark.parametrize("kind", ["device", "host", "segments"])
def test_budget_lowers_concurrency_and_nothing_else(backend, kind):
    L = backend.L
    n, fib = 8, 20000
    inp = synth_fibonacci(fib)
    est = estimate_memory(view=inp.view, lib=L)
    lone = backend.prove(inp)
    want = lone.words().copy()
    lone.free()
    backend.pool_trim()
    host = [synth_fibonacci(fib) for _ in range(n)] if kind == "host" else []
    segs = [synth_fibonacci_segment(fib) for _ in range(n)] if kind == "segments" else []
    devs = [backend.upload_input(inp) for _ in range(n)] if kind == "device" else []
    items = devs or host or segs
    # resident inputs: all eight for the device form, at most inflight + producers for the streaming forms (counted at eight here too)
    budget = 8 * est.input_bytes + est.working_bytes + est.working_bytes // 2
    try:
        mem_reset_peak(L)
        proofs = _many(backend, kind, items, 4)
        s = mem_stats(L)
        print(f"{kind}: no budget: peak in flight {s.peak_proofs_in_flight}, peak live {s.peak_live_bytes}")
        assert s.peak_proofs_in_flight >= 2
        for p in proofs:
            assert np.array_equal(p.words(), want)
            p.free()
        set_memory_budget(budget, L)
        mem_reset_peak(L)
        proofs = _many(backend, kind, items, 4)
        s = mem_stats(L)
        print(f"{kind}: budget {budget}: peak in flight {s.peak_proofs_in_flight}, peak live {s.peak_live_bytes}, peak reserved {s.peak_reserved_bytes}")
        for p in proofs:
            assert np.array_equal(p.words(), want)
            p.free()
        assert s.peak_proofs_in_flight == 1
        assert s.peak_live_bytes <= budget
    finally:
        set_memory_budget(0, L)
        for d in devs:
            backend.free_input(d)
        for h in host + segs + [inp]:
            h.free()


def test_an_item_over_the_budget_is_refused_before_any_gpu_work(backend):
    L = backend.L
    small, big = synth_fibonacci(3000), synth_fibonacci(100_000)
    e_small, e_big = estimate_memory(view=small.view, lib=L), estimate_memory(view=big.view, lib=L)
    assert e_big.working_bytes > e_small.working_bytes
    want = backend.prove(small)
    want_words = want.words().copy()
    want.free()
    devs = [backend.upload_input(x) for x in (small, big, small)]
    # room for everything resident and one small proof, not for the big one
    budget = 2 * e_small.input_bytes + e_big.input_bytes + e_small.working_bytes + (e_big.working_bytes - e_small.working_bytes) // 2
    assert e_big.input_bytes + e_big.working_bytes > budget >= e_small.input_bytes + e_small.working_bytes
    try:
        set_memory_budget(budget, L)
        # a lone proof applies the same rule: refused with status 2, both numbers named, no allocation made for it
        mem_reset_peak(L)
        with pytest.raises(CmError) as ex:
            backend.prove_device(devs[1])
        msg = str(ex.value)
        assert "status 2:" in msg and str(e_big.input_bytes) in msg and str(e_big.working_bytes) in msg, msg
        assert mem_stats(L).driver_allocs == 0
        with pytest.raises(CmError) as ex:
            backend.prove_many(devs, inflight=2)
        msg = str(ex.value)
        assert "status 2:" in msg and str(e_big.input_bytes) in msg and str(e_big.working_bytes) in msg, msg
        got = ex.value.partial
        assert got[1] is None and got[0] is not None and got[2] is not None
        for p in (got[0], got[2]):
            assert np.array_equal(p.words(), want_words)
            p.free()
        set_memory_budget(0, L)               # back to today's behaviour: everything is proved
        proofs = backend.prove_many(devs, inflight=2)
        assert all(p is not None for p in proofs)
        assert np.array_equal(proofs[0].words(), want_words)
        for p in proofs:
            p.free()
    finally:
        set_memory_budget(0, L)
        for d in devs:
            backend.free_input(d)
        small.free(); big.free()
