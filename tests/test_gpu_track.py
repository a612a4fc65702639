"""The relation tracker on whole segments (cm_track_relations, Backend.track_relations): valid inputs leave no tuple behind with
every relation forced through emit / sort / net, tampered inputs name exactly the orphaned tuples computed here from the input
arrays, the summary of every unbalanced input adds up to the per-relation sums the check reports (which the check's own tests tie
to the oracle), truncation, verdicts 1 and 2, the metric config, and proof bytes before / after a tracker call."""
import ctypes as C
import re

import numpy as np
import pytest

from cairo_m_amd.lib import (ArrayInput, CmError, N_COMPONENTS, RELATION_NAMES, RelationEntry, prover_input_arrays, synth_fibonacci)
from tests import casm_fixtures
from tests.test_gpu_air_eval_golden import qadd, qscale, qsub
from tests.test_gpu_check import bump, dst_access, tampered_fib40, u32_div_by_zero_input, valid_inputs
from tests.test_gpu_check_golden import qinv

pytestmark = pytest.mark.gpu
P = (1 << 31) - 1
STORE_FP_FP = 6
ALL = 0xFF


def strip(values):
    v = [int(x) % P for x in values]
    while v and v[-1] == 0:
        v.pop()
    return tuple(v)


def last_step(a):
    """(component, row, bundle) of the step with the highest clock"""
    best = None
    for c in range(26):
        for row, b in enumerate(a[f"bundles{c}"]):
            if best is None or int(b[2]) > int(best[2][2]):
                best = (c, row, b)
    return best


def final_pc_tamper():
    inp = synth_fibonacci(40)
    a = prover_input_arrays(inp.view)
    inp.free()
    true_pc, fp = int(a["regs"][2]), int(a["regs"][3])
    a["regs"][2] = (true_pc + 1) % P
    c, row, b = last_step(a)
    steps = sum(len(a[f"bundles{k}"]) for k in range(26))
    assert int(b[2]) == steps
    want = {("registers", strip([true_pc, fp, steps + 1])): (1, c, row),
            ("registers", strip([true_pc + 1, fp, steps + 1])): (P - 1, N_COMPONENTS, 0)}
    return ArrayInput(a), want


def prev_value_tamper(n=40, row=40):
    inp = synth_fibonacci(n)
    a = prover_input_arrays(inp.view)
    inp.free()
    i = dst_access(a, row)
    addr, prev_clock, v = (int(x) for x in a["data_accesses"][i][:3])
    bump(a, "data_accesses", i, 2)
    want = {("memory", strip([addr, prev_clock, v])): (1, None, None),
            ("memory", strip([addr, prev_clock, v + 1])): (P - 1, STORE_FP_FP, row)}
    return ArrayInput(a), want


def assert_entries(summary, want):
    assert summary.n_total == len(want) == len(summary.entries), str(summary)
    for e in summary.entries:
        key = (e.relation_name, e.tuple)
        assert key in want, str(summary)
        mult, comp, row = want[key]
        assert e.multiplicity == mult and e.n_entries == 1, str(summary)
        if comp is not None:
            assert (e.first_component, e.first_row) == (comp, row), str(summary)
    assert summary.as_dict() == {k: v[0] for k, v in want.items()}


def assert_consistent_with_the_check(summary, relations=range(8)):
    """per relation: sum over the entries of mult / (sum_i alpha^i v_i - z) == sum_c relation_sum[c][r] + public_sum[r]"""
    assert not summary.truncated
    rep = summary.report
    rel = rep.relation_words
    z = rel[:32].reshape(8, 4)
    apow = rel[32:].reshape(8, 16, 4)
    balance = rep.relation_balance()
    for r in relations:
        s = (0, 0, 0, 0)
        for e in summary.entries:
            if e.relation != r:
                continue
            den = (0, 0, 0, 0)
            for i, v in enumerate(e.tuple):
                den = qadd(den, qscale(tuple(int(x) for x in apow[r][i]), v))
            s = qadd(s, qscale(qinv(qsub(den, tuple(int(x) for x in z[r]))), int(e.multiplicity)))
        assert s == tuple(int(x) for x in balance[r]), (RELATION_NAMES[r], str(summary))


def test_valid_inputs_leave_nothing_behind(backend):
    for name, inp in valid_inputs():
        s = backend.track_relations(inp)
        assert s.report.status == 0 and s.n_total == 0 and s.entries == [] and not s.truncated, (name, str(s))
        s = backend.track_relations(inp, mask=ALL)
        assert s.report.status == 0 and s.n_total == 0, (name, str(s))
        inp.free()


def test_tampered_final_pc(backend):
    inp, want = final_pc_tamper()
    s = backend.track_relations(inp)
    assert s.report.status == 3 and s.report.unbalanced_relations() == ["registers"]
    assert_entries(s, want)
    assert_consistent_with_the_check(s)
    assert_entries(backend.track_relations(inp, mask=ALL), want)
    text = str(s)
    assert text.splitlines()[0] == "registers" and " -> -1   (PublicData row 0, 1 entries)" in text and " -> 1   (" in text


def test_tampered_prev_value(backend):
    inp, want = prev_value_tamper()
    s = backend.track_relations(inp)
    assert s.report.status == 3 and s.report.unbalanced_relations() == ["memory"]
    assert_entries(s, want)
    assert_consistent_with_the_check(s)
    assert all(isinstance(e, RelationEntry) for e in s.entries)
    assert_entries(backend.track_relations(inp, mask=ALL), want)
    # caller-supplied relations: the same tuples (their order follows the key, so it may differ)
    rel = np.random.default_rng(11).integers(1, P, size=s.report.relation_words.size, dtype=np.uint32)
    t = backend.track_relations(inp, relations=rel)
    assert np.array_equal(t.report.relation_words, rel)
    assert_entries(t, want)
    assert_consistent_with_the_check(t)


def test_truncation(backend):
    inp, _ = prev_value_tamper()
    two = backend.track_relations(inp, relations=None, cap=2)
    one = backend.track_relations(inp, relations=two.report.relation_words, cap=1)
    assert one.n_total == 2 and one.truncated and len(one.entries) == 1
    assert bytes(one.entries[0]) == bytes(two.entries[0])
    none = backend.track_relations(inp, cap=0)
    assert none.n_total == 2 and none.truncated and none.entries == []
    # the same through the C ABI with entries = NULL
    dev = backend.upload_input(inp)
    n = C.c_uint64(0)
    assert backend.L.cm_track_relations(dev, None, C.c_uint32(0), None, None, C.c_uint64(0), C.byref(n)) == 0
    assert n.value == 2
    backend.free_input(dev)


def unprovable_fixtures(word):
    for fx in casm_fixtures.load():
        if word in (fx.get("unprovable_reason") or ""):
            inp, _ = casm_fixtures.run_case(fx, fx["cases"][0])
            yield fx["name"], inp


def test_u32_store_eq_fixtures_name_memory_tuples(backend):
    n = 0
    for name, inp in unprovable_fixtures("U32StoreEq"):
        s = backend.track_relations(inp)
        assert s.report.status == 3, (name, s.report.message)
        assert s.n_total >= 2 and {e.relation_name for e in s.entries} == {"memory"}, (name, str(s))
        assert_consistent_with_the_check(s)
        inp.free()
        n += 1
    assert n == 5


def test_a_failing_constraint_does_not_stop_the_tracker(backend):
    inp = u32_div_by_zero_input()
    s = backend.track_relations(inp)
    assert s.report.status == 2 and s.report.message == "U32StoreDivFpFp: constraint 13 fails on row 0"
    tracked = {RELATION_NAMES.index(n) for n in s.report.unbalanced_relations()}
    assert {e.relation for e in s.entries} <= tracked
    assert_consistent_with_the_check(s)
    inp.free()


def test_out_of_range_lookups_show_up_as_tuples_nobody_emits(backend):
    n = 0
    for name, inp in unprovable_fixtures("range_check_20"):
        s = backend.track_relations(inp)
        assert s.report.status == 1, (name, s.report.message)
        got = s.as_dict()
        assert ("range_check_20", (P - 1,)) in got, (name, str(s))
        assert got[("range_check_20", (P - 1,))] > P // 2, (name, str(s))
        assert_consistent_with_the_check(s)
        inp.free()
        n += 1
    assert n == 3


def free_hbm(backend):
    f, t = C.c_uint64(0), C.c_uint64(0)
    assert backend.L.cm_device_mem_info(C.byref(f), C.byref(t)) == 0
    return f.value


def track_or_skip(backend, inp, **kw):
    try:
        return backend.track_relations(inp, **kw)
    except CmError as e:
        m = re.search(r"needs (\d+) bytes of device memory", str(e))
        if m and free_hbm(backend) < int(m.group(1)):
            pytest.skip(f"needs {m.group(1)} bytes of free HBM")
        raise


def test_metric_config(backend):
    inp = synth_fibonacci(419_000)
    assert inp.steps == 4_190_012
    s = track_or_skip(backend, inp, mask=ALL)
    assert s.report.status == 0 and s.n_total == 0, str(s)
    inp.free()
    bad, want = prev_value_tamper(419_000, 300_000)
    s = track_or_skip(backend, bad)
    assert s.report.status == 3 and s.report.unbalanced_relations() == ["memory"]
    assert_entries(s, want)
    assert_consistent_with_the_check(s)


def test_proof_bytes_unchanged_by_a_tracker_call(backend):
    inp = synth_fibonacci(1000)
    dev = backend.upload_input(inp)
    p0 = backend.prove_device(dev)
    w0 = p0.words().copy()
    p0.free()
    s = backend.track_relations(dev, mask=ALL)
    assert s.report.status == 0 and s.n_total == 0
    p1 = backend.prove_device(dev)
    assert np.array_equal(p1.words(), w0)
    p1.free()
    backend.free_input(dev)
    inp.free()
