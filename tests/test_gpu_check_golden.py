"""The check kernels (cm_relation_sums / k_relsum, cm_constraints_check / k_check) pinned to reference-derived data, not to the oracle:
  * tests/golden/air_eval_vectors.json (rows of arbitrary field elements with their constraint values and relation entries, from the
    reference's `evaluate` text) on a 2^4-row trace domain whose rows repeat the golden rows cyclically: the relation sums equal
    sum_rows sum_entries mult / (sum_i alpha^i v_i - z) computed here in plain Python, and with interaction columns from
    cm_interaction_write the row status is the lowest k with a non-zero golden constraint;
  * tests/golden/air_witness_vectors.npz (the reference's write_trace on a real run): every row passes; one changed cell fails its
    row alone."""
import json
import os

import numpy as np
import pytest

from tests.test_gpu_air_eval_golden import GOLD, PP_INDEX, REL_ID, _names, cmul, qadd, qmul, qscale, qsub
from tests.test_gpu_logup_golden import LOG as LOGUP, NAMES, TABLE_PP, WIT, relation_words

pytestmark = pytest.mark.gpu
P = 2**31 - 1
N_REL, MAX_REL, N_PP = 8, 16, 7
LOG = 4
NONE = 0xFFFFFFFF


def cinv(x):
    n = pow((x[0] * x[0] + x[1] * x[1]) % P, P - 2, P)
    return (x[0] * n % P, (P - x[1]) * n % P)


def qinv(x):
    """(a + b u)^-1 = (a - b u) / (a^2 - (2 + i) b^2)"""
    a, b = x[:2], x[2:]
    aa, bb = cmul(a, a), cmul(cmul(b, b), (2, 1))
    d = cinv(((aa[0] - bb[0]) % P, (aa[1] - bb[1]) % P))
    ra, rb = cmul(a, d), cmul(b, d)
    return (ra[0], ra[1], (P - rb[0]) % P, (P - rb[1]) % P)


def random_relations(seed):
    rng = np.random.default_rng(seed)
    rel = rng.integers(1, P, size=(N_REL + N_REL * MAX_REL) * 4, dtype=np.uint32)
    z = [tuple(int(x) for x in rel[4 * r:4 * r + 4]) for r in range(N_REL)]
    ap = rel[4 * N_REL:].reshape(N_REL, MAX_REL, 4)
    apow = [[tuple(int(x) for x in ap[r, i]) for i in range(MAX_REL)] for r in range(N_REL)]
    return rel, z, apow


def golden_columns(backend, g, n_trace):
    """2^LOG rows repeating the golden rows: (row -> golden row, trace handles, preprocessed handles)"""
    rows = g["rows"]
    n = 1 << LOG
    src = [r % len(rows) for r in range(n)]
    tr = np.zeros((n_trace, n), dtype=np.uint32)
    pp = np.zeros((N_PP, n), dtype=np.uint32)
    for r, k in enumerate(src):
        tr[:, r] = np.asarray(rows[k]["trace"], dtype=np.uint32)
        for cid_str, v in rows[k].get("preproc", {}).items():
            pp[PP_INDEX[cid_str], r] = v
    return src, [backend.upload(tr[c]) for c in range(n_trace)], [backend.upload(pp[i]) for i in range(N_PP)]


@pytest.mark.parametrize("name", sorted(GOLD))
def test_relation_sums_equal_reference_derived_entries(backend, oracle, name):
    cid = _names(oracle)[name]
    g = GOLD[name]
    n_trace, _, _ = backend.component_info(cid)
    rel, z, apow = random_relations(9100 + cid)
    src, h_tr, h_pp = golden_columns(backend, g, n_trace)
    try:
        got = backend.relation_sums(cid, h_tr, h_pp, LOG, rel)
        want = [(0, 0, 0, 0)] * N_REL
        for k in src:
            for rname, mult, vals in g["rows"][k]["relations"]:
                r = REL_ID[rname]
                den = (0, 0, 0, 0)
                for i, v in enumerate(vals):
                    den = qadd(den, qscale(apow[r][i], v))
                want[r] = qadd(want[r], qscale(qinv(qsub(den, z[r])), mult % P))
        for r in range(N_REL):
            assert tuple(int(x) for x in got[r]) == want[r], (name, r)
        assert got.any()
    finally:
        for h in h_tr + h_pp:
            backend.col_free(h)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_row_status_is_the_lowest_failing_golden_constraint(backend, oracle, name):
    cid = _names(oracle)[name]
    g = GOLD[name]
    n_trace, n_inter, _ = backend.component_info(cid)
    n = 1 << LOG
    rel, _, _ = random_relations(9200 + cid)
    src, h_tr, h_pp = golden_columns(backend, g, n_trace)
    h_it = [backend.col_alloc(n) for _ in range(n_inter)]
    h_st = backend.col_alloc(n)
    try:
        cs = backend.interaction_write(cid, h_tr, h_pp, LOG, rel, h_it)     # every LogUp constraint vanishes
        n_fail, first_k, first_row = backend.constraints_check(cid, h_tr, h_it, h_pp, LOG, rel, cs, h_st)
        status = backend.download(h_st, n)
        want = []
        for k in src:
            bad = [j for j, c in enumerate(g["rows"][k]["constraints"]) if c % P]
            want.append(bad[0] if bad else NONE)
        assert [int(x) for x in status] == want, name
        failing = [r for r in range(n) if want[r] != NONE]
        assert n_fail == len(failing)
        if failing:
            assert (first_row, first_k) == (failing[0], want[failing[0]])
        else:
            assert first_k == -1
    finally:
        for h in h_tr + h_pp + h_it + [h_st]:
            backend.col_free(h)


@pytest.mark.parametrize("cid", range(34), ids=NAMES)
def test_live_witness_rows_pass_and_one_changed_cell_fails_its_row(backend, cid):
    name = NAMES[cid]
    trace = np.array(LOGUP[name + "_mults"][None, :] if name in TABLE_PP else WIT[name], dtype=np.uint32)
    n = trace.shape[1]
    log = n.bit_length() - 1
    n_trace, n_inter, _ = backend.component_info(cid)
    pp = np.zeros((N_PP, n), dtype=np.uint32)
    for k, idx in enumerate(TABLE_PP.get(name, [])):
        pp[idx] = LOGUP[name + "_values"][k]
    rel = relation_words()
    h_tr = [backend.upload(np.ascontiguousarray(trace[c])) for c in range(n_trace)]
    h_pp = [backend.upload(np.ascontiguousarray(pp[i])) for i in range(N_PP)]
    h_it = [backend.col_alloc(n) for _ in range(n_inter)]
    h_st = backend.col_alloc(n)
    try:
        cs = backend.interaction_write(cid, h_tr, h_pp, log, rel, h_it)
        n_fail, first_k, _ = backend.constraints_check(cid, h_tr, h_it, h_pp, log, rel, cs, h_st)
        assert n_fail == 0 and first_k == -1, name
        assert (backend.download(h_st, n) == NONE).all(), name
        # one cell of one live row changed, the interaction columns kept: that row's constraints no longer hold, no other row reads it
        row = 1
        cell = trace.copy()
        cell[0, row] = (int(cell[0, row]) + 1) % P
        backend.col_free(h_tr[0])
        h_tr[0] = backend.upload(np.ascontiguousarray(cell[0]))
        n_fail, first_k, first_row = backend.constraints_check(cid, h_tr, h_it, h_pp, log, rel, cs, h_st)
        status = backend.download(h_st, n)
        assert n_fail == 1 and first_row == row and first_k >= 0, (name, n_fail, first_row)
        assert int(status[row]) == first_k and (np.delete(status, row) == NONE).all()
    finally:
        for h in h_tr + h_pp + h_it + [h_st]:
            backend.col_free(h)
