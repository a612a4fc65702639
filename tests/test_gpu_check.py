"""The PCS-free AIR check on the GPU (cm_check_constraints, Backend.check): whole segments against the CPU oracle's
orc_assert_constraints (the twin of the reference's debug_tools::assert_constraints), the per-relation sums (relation tracker)
against the claimed sums and the oracle's interaction claims, tampered inputs with one failing row or one broken relation, the
metric config and configs[4], and proof bytes before / after a check."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, N_COMPONENTS, RELATION_NAMES, prover_input_arrays, synth_fibonacci, vm_run)
from cairo_m_amd.workloads import all_opcodes_program, sha256_program
from tests import casm_fixtures
from tests.test_oracle_air import felt_program, u32_loop_program, u32_program

pytestmark = pytest.mark.gpu
P = (1 << 31) - 1


def qsum(words):
    """sum of QM31 values given as [..., 4] words (coordinate-wise modulo P)"""
    return (np.asarray(words, dtype=np.int64).reshape(-1, 4).sum(axis=0) % P).astype(np.uint32)


def assert_sums_consistent(rep):
    rs, cs, pub = rep.relation_sums, rep.claimed_sums, rep.public_sums
    for c in range(N_COMPONENTS):
        assert np.array_equal(qsum(rs[c]), cs[c]), f"component {c}: relation sums != claimed sum"
    for r in range(8):
        assert np.array_equal(qsum(np.concatenate([rs[:, r], pub[r:r + 1]])), np.zeros(4, np.uint32)), RELATION_NAMES[r]
    assert np.array_equal(qsum(np.concatenate([cs, pub])), np.asarray(rep.total, dtype=np.uint32))


def check_valid(backend, inp):
    rep = backend.check(inp)
    assert rep.status == 0, rep.message
    assert rep.message == ""
    assert list(rep.failing_rows) == [0] * N_COMPONENTS
    assert list(rep.first_constraint) == [-1] * N_COMPONENTS
    assert list(rep.total) == [0, 0, 0, 0]
    assert_sums_consistent(rep)
    return rep


def valid_inputs():
    yield "fib5", synth_fibonacci(5)
    yield "fib40", synth_fibonacci(40)
    yield "fib1000", synth_fibonacci(1000)
    yield "felt", vm_run(felt_program(), entry_pc=0, args=(), n_returns=1)
    yield "u32", vm_run(u32_program(), entry_pc=0, args=(), n_returns=0)
    yield "u32_loop", vm_run(u32_loop_program(60), entry_pc=0, args=(), n_returns=0)
    prog, _ = all_opcodes_program(300)
    yield "all_opcodes300", vm_run(prog, entry_pc=0, args=(), n_returns=0)
    prog, _ = sha256_program(b"abc")
    yield "sha256", vm_run(prog, entry_pc=0, args=(), n_returns=0)


def test_valid_programs_pass_and_sums_match_the_oracle(backend, oracle):
    for name, inp in valid_inputs():
        rc, err = oracle.assert_constraints(inp.view)
        assert rc == 0, (name, err)
        rep = check_valid(backend, inp)
        # every claimed sum = the oracle's InteractionClaim under the relations the check drew
        dev = backend.upload_input(inp)
        rel = rep.relation_words
        for c in range(N_COMPONENTS):
            n_int = backend.component_info(c)[1]
            lg = backend.component_log_size(dev, c)
            _, cs = oracle.component_interaction(inp.view, c, rel, n_int, lg)
            assert np.array_equal(cs, rep.claimed_sums[c]), (name, c)
        backend.free_input(dev)
        inp.free()


def test_default_relations_equal_explicit_ones(backend):
    inp = synth_fibonacci(40)
    a = backend.check(inp)
    rng = np.random.default_rng(7)
    rel = rng.integers(0, P, size=a.relation_words.size, dtype=np.uint32)
    b = backend.check(inp, relations=rel)
    assert b.status == 0, b.message
    assert np.array_equal(b.relation_words, rel)
    assert not np.array_equal(b.claimed_sums, a.claimed_sums)
    c = backend.check(inp, relations=a.relation_words)
    assert np.array_equal(c.claimed_sums, a.claimed_sums) and np.array_equal(c.relation_sums, a.relation_sums)
    inp.free()


def test_all_compiler_programs_agree_with_the_oracle(backend, oracle):
    n = 0
    for fx in casm_fixtures.load():
        inp, _ = casm_fixtures.run_case(fx, fx["cases"][0])
        rc, err = oracle.assert_constraints(inp.view)
        rep = backend.check(inp)
        assert rep.status == rc, (fx["name"], rep.message, err)
        if rc == 0:
            assert rep.message == "" and list(rep.total) == [0, 0, 0, 0], fx["name"]
        if rc == 1:
            assert err.startswith("lookup value out of range for ")
            table = err[len("lookup value out of range for "):].split(":")[0]
            assert rep.message.startswith("lookup value out of range for " + table + ":"), (fx["name"], rep.message, err)
        if rc == 2:
            assert rep.message.split(":")[0] == err.split(":")[0], (fx["name"], rep.message, err)
        if rc == 3:
            assert rep.message.startswith("LogUp sums do not cancel")
        if "U32StoreEq" in (fx.get("unprovable_reason") or ""):
            assert rep.status == 3 and rep.unbalanced_relations() == ["memory"], (fx["name"], rep.message)
            assert list(rep.failing_rows) == [0] * N_COMPONENTS
        inp.free()
        n += 1
    assert n == 122


def u32_div_by_zero_input():
    a = 0x12345678
    prog = [[23, a & 0xFFFF, a >> 16, 0], [23, 0, 0, 2], [18, 0, 2, 12, 14], [11]]
    return vm_run(prog, entry_pc=0, args=(), n_returns=0)


def tampered_fib40(edit):
    inp = synth_fibonacci(40)
    a = prover_input_arrays(inp.view)
    inp.free()
    edit(a)
    return ArrayInput(a)


def dst_access(a, row=40):
    return int(a["bundles6"][row][10]) + 2   # the third data access of the StoreFpFp bundle (its destination)


def bump(a, name, idx, col):
    a[name][idx][col] = (int(a[name][idx][col]) + 1) % P


@pytest.mark.parametrize("case", ["u32_div_by_zero", "store_fp_fp_value"])
def test_one_failing_row_gives_the_oracle_message(backend, oracle, case):
    if case == "u32_div_by_zero":
        inp = u32_div_by_zero_input()
        want = "U32StoreDivFpFp: constraint 13 fails on row 0"
    else:
        inp = tampered_fib40(lambda a: bump(a, "data_accesses", dst_access(a), 3))
        want = "StoreFpFp: constraint 7 fails on row 40"
    rc, err = oracle.assert_constraints(inp.view)
    assert rc == 2 and err == want
    rep = backend.check(inp)
    assert rep.status == 2
    assert rep.message == err
    assert rep.row == int(want.rsplit(" ", 1)[1]) and rep.constraint == int(want.split("constraint ")[1].split(" ")[0])
    assert rep.failing_rows[rep.component] == 1 and sum(rep.failing_rows) == 1
    assert rep.first_row[rep.component] == rep.row and rep.first_constraint[rep.component] == rep.constraint
    inp.free()


@pytest.mark.parametrize("case,relation", [("final_pc", "registers"), ("prev_value", "memory")])
def test_tamper_breaks_exactly_one_relation(backend, oracle, case, relation):
    if case == "final_pc":
        inp = tampered_fib40(lambda a: a["regs"].__setitem__(2, (int(a["regs"][2]) + 1) % P))
    else:
        inp = tampered_fib40(lambda a: bump(a, "data_accesses", dst_access(a), 2))
    rc, err = oracle.assert_constraints(inp.view)
    assert rc == 3, err
    rep = backend.check(inp)
    assert rep.status == 3, rep.message
    assert rep.message.startswith("LogUp sums do not cancel")
    assert rep.unbalanced_relations() == [relation]
    assert relation in rep.message
    assert list(rep.failing_rows) == [0] * N_COMPONENTS
    for c in range(N_COMPONENTS):   # the relation tracker still adds up to each component's claimed sum
        assert np.array_equal(qsum(rep.relation_sums[c]), rep.claimed_sums[c])
    inp.free()


def test_metric_config(backend, oracle):
    inp = synth_fibonacci(419_000)
    assert inp.steps == 4_190_012
    check_valid(backend, inp)
    a = prover_input_arrays(inp.view)
    inp.free()
    row = 300_000
    bump(a, "data_accesses", dst_access(a, row), 3)
    bad = ArrayInput(a)
    rc, err = oracle.assert_constraints(bad.view)
    assert rc == 2, err
    rep = backend.check(bad)
    assert rep.status == 2 and rep.message == err
    assert sum(rep.failing_rows) == 1


def test_configs4_all_opcodes_at_2pow26_rows(backend):
    """the reference's test_all_opcodes_constraints at the BASELINE configs[4] size (67 207 510 steps, 2^26 rows)"""
    from cairo_m_amd.lib import vm_segment

    def free_hbm():
        f, t = C.c_uint64(0), C.c_uint64(0)
        assert backend.L.cm_device_mem_info(C.byref(f), C.byref(t)) == 0
        return f.value
    if free_hbm() < 150 * 2**30:
        pytest.skip("needs ~116 GiB of free HBM")
    prog, steps = all_opcodes_program(1_545_000)
    assert 2**26 < steps < 2**26 + 2**18
    hs = vm_segment(prog, entry_pc=0, args=(), n_returns=0)
    dev = backend.adapt_segment(hs)
    hs.free()
    try:
        rep = backend.check(dev)
        assert rep.status == 0, rep.message
        assert list(rep.failing_rows) == [0] * N_COMPONENTS and list(rep.total) == [0, 0, 0, 0]
        assert_sums_consistent(rep)
    finally:
        backend.free_input(dev)
        assert backend.L.cm_pool_trim() == 0


def test_proof_bytes_unchanged_by_a_check(backend):
    inp = synth_fibonacci(1000)
    dev = backend.upload_input(inp)
    p0 = backend.prove_device(dev)
    w0 = p0.words().copy()
    p0.free()
    rep = backend.check(dev)
    assert rep.status == 0, rep.message
    p1 = backend.prove_device(dev)
    assert np.array_equal(p1.words(), w0)
    p1.free()
    backend.free_input(dev)
    inp.free()
