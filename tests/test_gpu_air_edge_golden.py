"""The HIP witness, histogram, LogUp and constraint kernels on EDGE operands (tests/edge_programs.py), against cells derived
mechanically from the reference's closures (tests/golden/air_witness_edge.npz, air_logup_edge.npz, air_witness_div0.npz) —
HIP vs reference-derived data with no oracle in between wherever the fixtures reach; the oracle is on the expected side only for
the constraint accumulator and the whole proof, which the fixtures do not hold.  CPU twin, the edge guard and the coverage of the
edge list: tests/test_air_edge_golden.py.  Every comparison is equality of M31 words."""
import numpy as np
import pytest

from cairo_m_amd.lib import N_COMPONENTS, N_PREPROCESSED, PREPROCESSED_LOG, vm_run
from tests.edge_programs import div_by_zero_program, edge_program
from tests.test_air_edge_golden import (C_DIV_FP, C_DIV_IMM, DIV0, LOG, MULT_LOGS, NAMES, WIT, check_logup_columns, describe_mismatch,
                                        edge_table, expected_multiplicities, relation_words)

pytestmark = pytest.mark.gpu
P = 2**31 - 1


def check_histogram(backend, dev, gold, tag):
    """cm_trace_write + cm_histogram of the 26 opcode components, accumulated, against expected_multiplicities(gold)"""
    mult = [backend.upload(np.zeros(1 << lg, dtype=np.uint32)) for lg in MULT_LOGS]
    for cid in range(26):
        n_tr, _, _ = backend.component_info(cid)
        log = backend.component_log_size(dev, cid)
        cols = [backend.col_alloc(1 << log) for _ in range(n_tr)]
        backend.trace_write(dev, cid, cols)
        backend.histogram(cid, cols, log, *mult)
        for h in cols:
            backend.col_free(h)
    want = expected_multiplicities(gold)
    for name, h, lg, w in zip(("range_check_8", "range_check_16", "range_check_20", "bitwise"), mult, MULT_LOGS, want):
        got = backend.download(h, 1 << lg)
        bad = np.flatnonzero(got != w)
        assert bad.size == 0, f"{tag}: {name} multiplicities differ at entries {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, reference-derived {w[bad[:5]].tolist()}"
        backend.col_free(h)


@pytest.fixture(scope="module")
def edge_input():
    prog, steps, edges = edge_program()
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps == int(WIT["steps"][0]) and edges == edge_table(WIT)
    yield inp
    inp.free()


@pytest.fixture(scope="module")
def div0_input():
    prog, steps, _ = div_by_zero_program()
    inp = vm_run(prog, entry_pc=0, args=(), n_returns=0)
    assert inp.steps == steps == int(DIV0["steps"][0])
    yield inp
    inp.free()


def _hip_trace(backend, dev, cid, n_cols):
    log = backend.component_log_size(dev, cid)
    cols = [backend.col_alloc(1 << log) for _ in range(n_cols)]
    backend.trace_write(dev, cid, cols)
    got = np.stack([backend.download(h, 1 << log) for h in cols])
    for h in cols:
        backend.col_free(h)
    return got


def test_hip_witness_equals_reference_derived_cells(backend, edge_input):
    dev = backend.upload_input(edge_input)
    edges = edge_table(WIT)
    for cid, name in enumerate(NAMES):
        want = WIT[name]
        msg = describe_mismatch(name, cid, _hip_trace(backend, dev, cid, want.shape[0]), want, edges)
        assert msg is None, msg
    backend.free_input(dev)


def test_hip_histogram_equals_bincounts_of_the_reference_lookups(backend, edge_input):
    dev = backend.upload_input(edge_input)
    check_histogram(backend, dev, WIT, "edge program")
    backend.free_input(dev)


@pytest.mark.parametrize("cid", range(27), ids=NAMES[:27])
def test_hip_logup_columns_equal_reference_derived_fractions(backend, cid):
    """the fixture's TRACE through cm_interaction_write under the seeded relations tools/rsref/rs_logup.py used"""
    name = NAMES[cid]
    want, trace = LOG[name].astype(np.int64), WIT[name]
    n = trace.shape[1]
    n_trace, n_inter, _ = backend.component_info(cid)
    assert trace.shape[0] == n_trace and want.shape == (n_inter // 4, n, 4)
    h_tr = [backend.upload(np.ascontiguousarray(trace[c])) for c in range(n_trace)]
    h_pp = [backend.upload(np.zeros(n, dtype=np.uint32)) for _ in range(N_PREPROCESSED)]     # only the lookup tables read them
    h_out = [backend.col_alloc(n) for _ in range(n_inter)]
    try:
        cs = backend.interaction_write(cid, h_tr, h_pp, n.bit_length() - 1, relation_words(LOG), h_out)
        got = np.stack([backend.download(h, n) for h in h_out]).astype(np.int64).reshape(n_inter // 4, 4, n)
        check_logup_columns(name, got, cs, want)
        assert np.any(want[-1] % P)
    finally:
        for h in h_tr + h_pp + h_out:
            backend.col_free(h)


def test_check_constraints_accepts_the_edge_program(backend, edge_input):
    rep = backend.check(edge_input)
    assert rep.status == 0 and rep.message == "", rep.message
    assert list(rep.failing_rows) == [0] * N_COMPONENTS
    assert rep.unbalanced_relations() == [] and list(rep.total) == [0, 0, 0, 0]


def test_constraint_accumulator_equals_oracle_per_component(backend, oracle, edge_input):
    """cm_constraints_accumulate on the evaluation domain, component by component (the form of tests/test_gpu_components.py)"""
    from tests.test_gpu_components import _lde
    rng = np.random.default_rng(0xED6E)
    tw = backend.twiddles(22)
    pp_lde = []
    for k in range(N_PREPROCESSED):
        h = backend.col_alloc(1 << PREPROCESSED_LOG[k])
        backend.preprocessed_column(k, h)
        host = backend.download(h, 1 << PREPROCESSED_LOG[k])
        backend.col_free(h)
        pp_lde.append(_lde(backend, [host], PREPROCESSED_LOG[k], tw)[0])
    rel = relation_words(LOG)
    dev = backend.upload_input(edge_input)
    for cid, name in enumerate(NAMES):
        n_tr, n_it, n_cons = backend.component_info(cid)
        log = backend.component_log_size(dev, cid)
        trace = _hip_trace(backend, dev, cid, n_tr)
        h_tr = [backend.upload(c) for c in trace]
        h_pp = [backend.upload(np.zeros(1 << log, dtype=np.uint32)) for _ in range(N_PREPROCESSED)]
        out = [backend.col_alloc(1 << log) for _ in range(n_it)]
        cs = backend.interaction_write(cid, h_tr, h_pp, log, rel, out)
        inter = np.stack([backend.download(h, 1 << log) for h in out])
        coeff = rng.integers(0, P, size=4 * n_cons, dtype=np.uint32)
        tr_lde, it_lde = _lde(backend, list(trace), log, tw), _lde(backend, list(inter), log, tw)
        acc = [backend.upload(np.zeros(2 << log, dtype=np.uint32)) for _ in range(4)]
        backend.constraints_accumulate(cid, tr_lde, it_lde, pp_lde, log, rel, coeff, cs, acc)
        got = np.stack([backend.download(h, 2 << log) for h in acc])
        want = oracle.component_constraints(edge_input.view, cid, rel, coeff, log)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name} (component {cid}): accumulator differs first at (coordinate, point) {bad[:4].tolist()}"
        for h in h_tr + h_pp + out + tr_lde + it_lde + acc:
            backend.col_free(h)
    backend.free_input(dev)
    for h in pp_lde:
        backend.col_free(h)
    backend.twiddles_free(tw)


@pytest.mark.parametrize("cid", [C_DIV_IMM, C_DIV_FP], ids=["u32_store_div_fp_imm", "u32_store_div_fp_fp"])
def test_hip_division_by_zero_witness_equals_reference_derived_cells(backend, div0_input, cid):
    dev = backend.upload_input(div0_input)
    want = DIV0[NAMES[cid]]
    msg = describe_mismatch(NAMES[cid], cid, _hip_trace(backend, dev, cid, want.shape[0]), want, edge_table(DIV0))
    backend.free_input(dev)
    assert msg is None, msg


def test_check_constraints_names_the_division_by_zero_row(backend, oracle, div0_input):
    rep = backend.check(div0_input)
    rc, err = oracle.assert_constraints(div0_input.view)
    assert rep.status == 2 == rc and rep.message == err, (rep.message, err)
    assert rep.component in (C_DIV_IMM, C_DIV_FP) and rep.row == 0
    assert rep.failing_rows[C_DIV_IMM] == 1 and rep.failing_rows[C_DIV_FP] == 1 and sum(rep.failing_rows) == 2
    assert rep.first_row[C_DIV_IMM] == 0 and rep.first_row[C_DIV_FP] == 0


def test_edge_program_proof_bit_exact_and_verifies(backend, oracle, edge_input):
    p = backend.prove(edge_input)
    want, _ = oracle.prove(edge_input.view)
    got = p.words()
    assert got.size == want.size and np.array_equal(got, want)
    rc, err = p.verify()
    assert rc == 0, err
    assert backend.verify_many([p]) == [(0, "")]
    p.free()
