"""cm_estimate_memory / cm_estimate_memory_logs (host code, no GPU): monotone in every component's log size and in the blowup,
the two forms agree, bad arguments are refused, input_bytes is the pool-rounded sum of the input's arrays, and the bound leaves
room for what the library already runs on one 288 GB MI355X.  CPU only."""
import ctypes as C

import pytest

from cairo_m_amd.lib import (CmError, ProverInputView, estimate_memory, load_library, synth_fibonacci, vm_run)

HBM_BYTES = 288 * 10**9          # MI355X
TABLE_LOGS = [8, 16, 20, 18]     # range_check_8 / _16 / _20, bitwise: fixed sizes
SIZES = {"bundle": 48, "data_access": 16, "memory_cell": 28, "clock_update": 24, "merkle_node": 32}   # include/cairom_hip.h


@pytest.fixture(scope="module")
def L():
    return load_library()


def pool_round(b):
    """Pool::round of cairo_m_amd/csrc/pool.hip; an empty array still is a 4-byte request"""
    b = max(b, 4)
    return (b + 511) & ~511 if b <= (1 << 20) else (b + (1 << 21) - 1) & ~((1 << 21) - 1)


def log_size_for(n):
    l = 4
    while (1 << l) < n:
        l += 1
    return l


def view_of(inp):
    return C.cast(inp.view, C.POINTER(ProverInputView)).contents


def component_rows(v):
    rows = [int(v.n_bundles[i]) for i in range(26)]
    tree = int(v.n_initial_tree + v.n_final_tree)
    return rows + [int(v.n_initial_memory + v.n_final_memory), tree, int(v.n_clock_updates), tree]


def component_logs(v):
    return [log_size_for(r) for r in component_rows(v)] + TABLE_LOGS


BASES = [[4] * 30 + TABLE_LOGS,
         [12 + (7 * i) % 9 for i in range(30)] + TABLE_LOGS,
         [18] + [4] * 25 + [10, 14, 4, 14] + TABLE_LOGS,
         [25] * 34]


@pytest.mark.parametrize("world", [1, 2, 4, 8])
def test_working_bytes_is_monotone_in_every_log_size_and_in_the_blowup(L, world):
    for base in BASES:
        for blowup in (1, 2, 3, 4):
            cfg = (16, blowup, 0, 80)
            w0 = estimate_memory(log_sizes=base, cfg=cfg, world=world, lib=L).working_bytes
            assert w0 > 0
            for c in range(34):
                if base[c] >= 26:
                    continue
                up = list(base)
                up[c] += 1
                assert estimate_memory(log_sizes=up, cfg=cfg, world=world, lib=L).working_bytes >= w0, (base, c, blowup)
            if blowup < 4:
                assert estimate_memory(log_sizes=base, cfg=(16, blowup + 1, 0, 80), world=world, lib=L).working_bytes >= w0


def test_input_form_equals_the_logs_form_and_input_bytes_is_the_rounded_sum(L):
    for inp in (synth_fibonacci(5, lib=L), synth_fibonacci(20000, lib=L)):
        v = view_of(inp)
        logs = component_logs(v)
        for world in (1, 2):
            for cfg in (None, (16, 2, 0, 80)):
                a = estimate_memory(view=inp.view, cfg=cfg, world=world, lib=L)
                b = estimate_memory(log_sizes=logs, cfg=cfg, world=world, lib=L)
                assert (a.working_bytes, a.cached_bytes) == (b.working_bytes, b.cached_bytes)
                assert b.input_bytes == 0
        want = sum(pool_round(int(v.n_bundles[i]) * SIZES["bundle"]) for i in range(26))
        want += pool_round(int(v.n_data_accesses) * SIZES["data_access"])
        want += pool_round(int(v.n_initial_memory) * SIZES["memory_cell"]) + pool_round(int(v.n_final_memory) * SIZES["memory_cell"])
        want += pool_round(int(v.n_clock_updates) * SIZES["clock_update"])
        want += pool_round(int(v.n_initial_tree) * SIZES["merkle_node"]) + pool_round(int(v.n_final_tree) * SIZES["merkle_node"])
        assert estimate_memory(view=inp.view, lib=L).input_bytes == want
        inp.free()


def test_bad_arguments_are_status_1_with_a_message(L):
    ok = [10] * 30 + TABLE_LOGS
    for kw in (dict(log_sizes=[27] + ok[1:]), dict(log_sizes=ok, cfg=(16, 0, 0, 80)), dict(log_sizes=ok, cfg=(16, 5, 0, 80)),
               dict(log_sizes=ok, world=3), dict(log_sizes=ok, world=0), dict(log_sizes=ok, world=16)):
        with pytest.raises(CmError) as e:
            estimate_memory(lib=L, **kw)
        assert "status 1:" in str(e.value) and len(str(e.value)) > 30
    from cairo_m_amd.lib import MemEstimate
    e = MemEstimate()
    e.struct_size = C.sizeof(MemEstimate)
    logs = (C.c_uint32 * 34)(*ok)
    assert L.cm_estimate_memory_logs(None, None, C.c_uint32(1), C.byref(e)) == 1
    assert L.cm_estimate_memory_logs(logs, None, C.c_uint32(1), None) == 1
    assert L.cm_estimate_memory(None, None, C.c_uint32(1), C.byref(e)) == 1
    e.struct_size = 8
    assert L.cm_estimate_memory_logs(logs, None, C.c_uint32(1), C.byref(e)) == 1


def test_the_bound_admits_what_the_library_already_runs(L):
    """README: four proofs of the metric config in flight, and the all-opcodes loop of 2^26 rows, both on one 288 GB GPU."""
    from cairo_m_amd.workloads import all_opcodes_program
    # all-opcodes loop at 1_545_000 iterations (bench.py --big-mixed-iters): every component's row count is linear in the
    # iteration count, so two short runs of the generator's program give the counts of the long one without running it
    rows = {}
    for iters in (200, 400):
        prog, _ = all_opcodes_program(iters)
        inp = vm_run(prog, entry_pc=0, args=(), n_returns=0, lib=L)
        rows[iters] = component_rows(view_of(inp))
        inp.free()
    big = 1_545_000
    logs = []
    for r200, r400 in zip(rows[200], rows[400]):
        per_iter = (r400 - r200) / 200.0
        logs.append(log_size_for(int(r200 + per_iter * (big - 200)) + 1))
    assert max(logs) >= 21
    e = estimate_memory(log_sizes=logs + TABLE_LOGS, lib=L)
    steps = sum(int(rows[200][i] + (rows[400][i] - rows[200][i]) / 200.0 * (big - 200)) for i in range(26))
    input_bytes = steps * (SIZES["bundle"] + 4 * SIZES["data_access"])     # at most four data accesses per step
    print("all-opcodes 2^26: working", e.working_bytes, "input <=", input_bytes)
    assert input_bytes + e.working_bytes < HBM_BYTES
    inp = synth_fibonacci(419_000, lib=L)     # the metric config (bench.py FIB_N)
    m = estimate_memory(view=inp.view, lib=L)
    inp.free()
    print("metric config: working", m.working_bytes, "input", m.input_bytes)
    assert 4 * m.working_bytes + 5 * m.input_bytes < HBM_BYTES
