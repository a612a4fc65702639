"""The relation tracker at the op level (cm_relation_entries: k_track_emit, sort, net, k_track_recover) pinned to reference-derived
data, not to this repository's reading of the AIR: tests/golden/air_eval_vectors.json holds, for all 34 components, rows of arbitrary
field elements with the relation entries [name, mult, values] that the reference's own `evaluate` text produces.  The columns are
those of tests/test_gpu_check_golden.py::golden_columns (2^4 rows repeating the golden rows cyclically), so most tuples are the sum
of several equal entries and the netting is exercised, not just the emit.  The expectation is the aggregation in plain Python:
strip trailing zeros, add the multiplicities modulo P, drop the zeros.

Counted on the CPU over the JSON (no GPU) before relying on it: for every component the expected set is non-empty and far below the
cap passed here: between 4 (Poseidon2C) and 281 (U32StoreDivFpImm) tuples against CAP = 4096; every component has at least one
golden entry of multiplicity zero, which must not be counted.  test_expected_sets_are_usable re-checks that."""
import numpy as np
import pytest

from cairo_m_amd.lib import RELATION_NAMES, RelationEntry
from tests.test_gpu_air_eval_golden import GOLD, REL_ID, _names
from tests.test_gpu_check_golden import LOG, golden_columns, random_relations

pytestmark = pytest.mark.gpu
P = 2**31 - 1
CAP = 4096


def expected_summary(g, only=None):
    """{(relation id, values): [net multiplicity, entries merged, lowest row]} of the 2^LOG-row columns"""
    rows = g["rows"]
    agg = {}
    for r in range(1 << LOG):
        for rname, mult, vals in rows[r % len(rows)]["relations"]:
            if mult % P == 0 or (only is not None and REL_ID[rname] != only):
                continue
            v = [x % P for x in vals]
            while v and v[-1] == 0:
                v.pop()
            e = agg.setdefault((REL_ID[rname], tuple(v)), [0, 0, r])
            e[0] = (e[0] + mult) % P
            e[1] += 1
    return {k: e for k, e in agg.items() if e[0]}


def test_expected_sets_are_usable():
    for name, g in GOLD.items():
        assert 0 < len(expected_summary(g)) < CAP, name


def compare(summary, want, cid, name):
    assert summary.n_total == len(want) and not summary.truncated, (name, summary.n_total, len(want))
    got = {}
    for e in summary.entries:
        assert isinstance(e, RelationEntry) and e.multiplicity != 0 and e.first_component == cid
        assert all(v == 0 for v in e.values[e.n_values:]) and (e.n_values == 0 or e.values[e.n_values - 1] != 0)
        key = (e.relation, e.tuple)
        assert key not in got, (name, key)
        got[key] = [int(e.multiplicity), int(e.n_entries), int(e.first_row)]
    assert set(got) == set(want), name
    for k in want:
        assert got[k] == want[k], (name, RELATION_NAMES[k[0]], k[1], got[k], want[k])
    order = [e.relation for e in summary.entries]
    assert order == sorted(order)
    assert summary.as_dict() == {(RELATION_NAMES[k[0]], k[1]): e[0] for k, e in want.items()}


@pytest.mark.parametrize("name", sorted(GOLD))
def test_entries_equal_the_aggregated_reference_entries(backend, oracle, name):
    cid = _names(oracle)[name]
    g = GOLD[name]
    n_trace, _, _ = backend.component_info(cid)
    rel, _, _ = random_relations(9300 + cid)
    _, h_tr, h_pp = golden_columns(backend, g, n_trace)
    try:
        compare(backend.relation_entries(cid, h_tr, h_pp, LOG, rel, mask=0, cap=CAP), expected_summary(g), cid, name)
    finally:
        for h in h_tr + h_pp:
            backend.col_free(h)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_a_one_relation_mask_gives_that_relation_alone(backend, oracle, name):
    cid = _names(oracle)[name]
    g = GOLD[name]
    n_trace, _, _ = backend.component_info(cid)
    rel, _, _ = random_relations(9400 + cid)
    used = sorted({k[0] for k in expected_summary(g)})
    _, h_tr, h_pp = golden_columns(backend, g, n_trace)
    try:
        for r in (used[0], used[-1]):
            compare(backend.relation_entries(cid, h_tr, h_pp, LOG, rel, mask=1 << r, cap=CAP), expected_summary(g, only=r), cid, name)
        unused = [r for r in range(8) if r not in {REL_ID[e[0]] for row in g["rows"] for e in row["relations"]}]
        if unused:
            assert backend.relation_entries(cid, h_tr, h_pp, LOG, rel, mask=1 << unused[0], cap=CAP).n_total == 0
    finally:
        for h in h_tr + h_pp:
            backend.col_free(h)
