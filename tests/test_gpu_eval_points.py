"""The provers' out-of-domain sampling kernels — k_oods_maps, k_point_tables_multi, k_eval_partial_multi and
k_reduce_partials_multi behind eval_at_point_multi (kernels_poly.hip) — through cm_eval_at_points_op, on inputs the tests choose.
Whole proofs reach these kernels only with what a transcript picks: about 20 jobs, log sizes of 4 and up, pseudo-random
coefficients, one felt.  Every comparison is bit for bit against tests/eval_points_ref.py (eval_fold, oods_point) and, in the
host-point form, against the CPU oracle as well.  The sizes are the smallest that reach the branch they name (EAP2_LOW_BITS = 10:
a chunk is 2^10 coefficients; EAP2_GROUP = 32: a block walks up to 32 chunks); none is the workload's size.

The accumulation bound of k_eval_partial_multi (four raw products on a folded remainder: 4 (2^31-1)^2 + 3 * 2^32 < 2^64) is tight
only when the high-table words are near P as well.  Those words are products of doubled x values of the point and cannot be
steered through it, so the bound is NOT pinned at its exact worst case here: columns of P-1 at log_n = 15 (one full group, eight
folds) are the closest input that can be reached."""
import numpy as np
import pytest

from cairo_m_amd.lib import EVAL_GUARD, EVAL_GUARD_WORDS
from tests import eval_points_ref as ref
from tests import field_edges as fe
from tests.field_edges import P

pytestmark = pytest.mark.gpu
_REF = {}        # references computed once, shared by the tests that need them and left unchanged


def _want(key, col, pt):
    if key not in _REF:
        v = ref.eval_fold(col, pt[:4], pt[4:])
        v.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def _run(backend, jobs, t=None, landing=False):
    """jobs: dicts with log_n, cols (arrays) and point or shift.  Uploads, runs one call, frees; checks the guard words."""
    hs = [[backend.upload(c) for c in j["cols"]] for j in jobs]
    try:
        res = backend.eval_at_points([dict(log_n=j["log_n"], coeffs=h, point=j.get("point", (0,) * 8), shift=j.get("shift"))
                                      for j, h in zip(jobs, hs)], t=t, landing=landing)
    finally:
        for h in hs:
            for x in h:
                backend.col_free(x)
    assert len(res["values"]) == len(jobs)
    for k, g in enumerate(res["guards"]):
        assert g.size == EVAL_GUARD_WORDS and (g == EVAL_GUARD).all(), ("guard behind job", k, g)
    for k, v in enumerate(res["values"]):
        assert (v < P).all(), ("job", k, "a word that is no canonical M31 (unwritten or unreduced)", v)
    return res


def _ladder_columns(rng, n):
    return [fe.const(P - 1, n), fe.near_p(rng, n), fe.edge_mix(rng, n), fe.alt(n), rng.integers(0, P, size=n, dtype=np.uint32)]


# ---- 1. the size ladder ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [0, 1, 3, 9, 10, 11, 12, 13, 15, 16, 17])
def test_size_ladder(backend, oracle, log_n):
    """One job per size.  0, 1, 3, 9: fewer low indices than a block has lanes times four, idle lanes, full_low false; 10: one
    chunk, full_low, the bounds-tested branch; 11: two chunks, bounds-tested; 12: exactly one unrolled step; 13: two; 15: one full
    group of 32 chunks, eight folds (const(P-1) here is the closest reachable input to the accumulation bound); 16: two groups, so
    k_reduce_partials_multi sums more than one partial; 17: four groups."""
    n = 1 << log_n
    rng = np.random.default_rng(6100 + log_n)
    cols = _ladder_columns(rng, n)
    for pi, pt in enumerate((rng.integers(0, P, size=8, dtype=np.uint32), fe.edge_mix(rng, 8))):
        got = _run(backend, [dict(log_n=log_n, cols=cols, point=pt)])["values"][0]
        for ci, c in enumerate(cols):
            assert np.array_equal(got[ci], _want(("ladder", log_n, pi, ci), c, pt)), (log_n, pi, ci)
            assert np.array_equal(got[ci], oracle.eval_at_point(c, pt)), (log_n, pi, ci, "oracle")
        if log_n == 0:
            assert all(tuple(g) == (int(c[0]), 0, 0, 0) for g, c in zip(got, cols))


# ---- 2. a high table larger than the low table -------------------------------------------------------------------------------
def test_high_table_larger_than_low_table(backend, oracle):
    """log_n = 21: the high table (2^11 entries) is larger than the low one (2^10), so max_tab_blocks comes from the high bits of
    this job, and 64 groups per column are reduced.  The log_n = 3 jobs in front of it and behind it share the launch: their
    table blocks beyond the first return early."""
    rng = np.random.default_rng(6221)
    jobs = [dict(log_n=3, cols=[rng.integers(0, P, size=8, dtype=np.uint32)], point=rng.integers(0, P, size=8, dtype=np.uint32)),
            dict(log_n=21, cols=[fe.const(P - 1, 1 << 21), rng.integers(0, P, size=1 << 21, dtype=np.uint32)],
                 point=rng.integers(0, P, size=8, dtype=np.uint32)),
            dict(log_n=3, cols=[fe.edge_mix(rng, 8), fe.const(P - 1, 8)], point=fe.edge_mix(rng, 8))]
    got = _run(backend, jobs)["values"]
    for k, j in enumerate(jobs):
        for ci, c in enumerate(j["cols"]):
            assert np.array_equal(got[k][ci], _want(("high", k, ci), c, j["point"])), (k, ci)
            assert np.array_equal(got[k][ci], oracle.eval_at_point(c, j["point"])), (k, ci, "oracle")


# ---- 3. the block-to-job and column-to-job scans -------------------------------------------------------------------------------
def _scan_job(k):
    """Job k of the 64: log_n cycles through 4, 10, 11, 16 (1, 1, 1 and 2 groups per column) and n_cols through 1, 2, 3, so the
    block and column prefixes are uneven; every column and every point is drawn from a seed of its own."""
    log_n, n_cols = (4, 10, 11, 16)[k % 4], 1 + k % 3
    rng = np.random.default_rng(6300 + k)
    return dict(key=k, log_n=log_n, cols=[rng.integers(0, P, size=1 << log_n, dtype=np.uint32) for _ in range(n_cols)],
                point=rng.integers(0, P, size=8, dtype=np.uint32))


def _check_scan(backend, jobs, landing=False):
    res = _run(backend, jobs, landing=landing)
    for j, got in zip(jobs, res["values"]):
        assert got.shape == (len(j["cols"]), 4)
        for ci, c in enumerate(j["cols"]):
            assert np.array_equal(got[ci], _want(("scan", j["key"], ci), c, j["point"])), ("job", j["key"], "column", ci)
    return res


@pytest.mark.parametrize("case", ["one_job", "two_jobs_1_and_5_columns", "64_jobs", "64_jobs_reversed"])
def test_job_scan(backend, case):
    """Blocks and columns find their job by counting the starts at or below their index.  One job (no start counted), two jobs
    with 1 and 5 columns, 64 jobs (every slot of EapStarts in use) with uneven block and column counts, and the same 64 the other
    way round.  Every column of every job is checked — the first and the last of a job sit on the boundaries — and all data is
    distinct, so a block or column handed to the wrong job cannot give an equal value.  The guard words behind every job's slice
    stay as they were (checked by _run)."""
    if case == "one_job":
        jobs = [_scan_job(3)]
    elif case == "two_jobs_1_and_5_columns":
        a, b = _scan_job(0), _scan_job(100)
        rng = np.random.default_rng(6299)
        b = dict(key=100, log_n=11, cols=[rng.integers(0, P, size=1 << 11, dtype=np.uint32) for _ in range(5)], point=b["point"])
        jobs = [a, b]
        assert [len(j["cols"]) for j in jobs] == [1, 5]
    else:
        jobs = [_scan_job(k) for k in range(64)]
        assert len({j["cols"][0][:4].tobytes() for j in jobs}) == 64 and len({j["point"].tobytes() for j in jobs}) == 64
        if case == "64_jobs_reversed":
            jobs = jobs[::-1]
    _check_scan(backend, jobs)


# ---- 4. the device-point form ------------------------------------------------------------------------------------------------
def _probe_columns(rng, n):
    """c[1] = 1 evaluates to m_0 = y and c[2] = 1 to m_1 = x: the first two values of a job ARE the point it sampled at."""
    py, px = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    py[1], px[2] = 1, 1
    return [py, px, rng.integers(0, P, size=n, dtype=np.uint32), fe.const(P - 1, n)]


@pytest.mark.parametrize("name,t", ref.gpu_felts(), ids=[n for n, _ in ref.gpu_felts()])
def test_device_point_form(backend, name, t):
    """k_oods_maps: the point ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)) of the uploaded felt, per job plus its shift, and the per-bit
    factors from it.  Felts: 0 (the point (1, 0)), 1, all words P-1, a draw from the edge words, a random one; a felt with
    1 + t^2 = 0 (t = +-i) is left out — the inverse of zero is not defined by the reference and no transcript reaches it.  Eight
    jobs per call, log_n 4 and 11, each unshifted, shifted as the previous-row mask is ((step.x, -step.y) of the subgroup generator
    of that size) and by the two circle points with a coordinate equal to P-1; the per-job points handed in are garbage that must
    be ignored.  The probe columns read the point back; the others go through the whole evaluation."""
    rng = np.random.default_rng(6400)
    jobs, pts = [], []
    for log_n in ref.GPU_POINT_LOGS:
        for sname, s in ref.gpu_shifts(log_n):
            jobs.append(dict(log_n=log_n, cols=_probe_columns(rng, 1 << log_n), shift=s, point=fe.near_p(rng, 8)))
            pts.append(ref.oods_point(t, s))
    res = _run(backend, jobs, t=t, landing=True)
    for k, (j, (x, y)) in enumerate(zip(jobs, pts)):
        got = res["values"][k]
        assert tuple(int(w) for w in got[0]) == y and tuple(int(w) for w in got[1]) == x, (name, k, "the point")
        for ci in (2, 3):
            assert np.array_equal(got[ci], ref.eval_fold(j["cols"][ci], x, y)), (name, k, ci)
        assert np.array_equal(res["land_values"][k], got), (name, k, "landing")
    if name == "zero":
        assert pts[0] == ((1, 0, 0, 0), (0, 0, 0, 0))
    n_shifts = len(ref.gpu_shifts(4))
    for base in range(0, len(jobs), n_shifts):      # jobs of one call with different shifts sample at different points
        seen = {(res["values"][k][1].tobytes(), res["values"][k][0].tobytes()) for k in range(base, base + n_shifts)}
        assert len(seen) == n_shifts, (name, base)


# ---- 5. the landing buffer -----------------------------------------------------------------------------------------------------
def test_landing_buffer(backend):
    """The second store of k_reduce_partials_multi: with the flag set every job's values also land in the pinned buffer — equal to
    the device words, no 0xFFFFFFFF left inside a slice, and the bytes outside the slices still 0xFF.  Without the flag the
    kernels store to device memory only and the values are the same."""
    jobs = [_scan_job(k) for k in range(12)]
    res = _check_scan(backend, jobs, landing=True)
    for k, (dv, lv, lg) in enumerate(zip(res["values"], res["land_values"], res["land_guards"])):
        assert np.array_equal(lv, dv), ("job", k)
        assert not (lv == 0xFFFFFFFF).any(), ("job", k, "a landing word was not written")
        assert (lg == 0xFFFFFFFF).all(), ("job", k, "a word outside the slices was written", lg)
    plain = _check_scan(backend, jobs, landing=False)
    assert "land_values" not in plain and all(np.array_equal(a, b) for a, b in zip(plain["values"], res["values"]))


# ---- 6. the worst-case columns of test_gpu_field_edges.test_eval_at_point_edges, through this path ---------------------------
@pytest.mark.parametrize("log_n", [3, 11, 12, 13, 15])
def test_worst_case_columns_on_both_paths(backend, oracle, log_n):
    """The four columns and two points of test_eval_at_point_edges (same seeds) through eval_at_point_multi, and through the older
    cm_eval_at_point next to it: both equal the reference, hence each other."""
    n = 1 << log_n
    rng = np.random.default_rng(500 + log_n)
    cols = [fe.const(P - 1, n), fe.near_p(rng, n), fe.edge_mix(rng, n), fe.alt(n)]
    hs = [backend.upload(c) for c in cols]
    try:
        for pi, pt in enumerate((rng.integers(0, P, size=8, dtype=np.uint32), fe.edge_mix(rng, 8))):
            new = backend.eval_at_points([dict(log_n=log_n, coeffs=hs, point=pt)])
            assert (new["guards"][0] == EVAL_GUARD).all()
            old = backend.eval_at_point(hs, log_n, pt)
            for ci, c in enumerate(cols):
                want = _want(("worst", log_n, pi, ci), c, pt)
                assert np.array_equal(new["values"][0][ci], want), ("multi", log_n, pi, ci)
                assert np.array_equal(old[ci], want), ("batch", log_n, pi, ci)
                assert np.array_equal(want, oracle.eval_at_point(c, pt)), ("oracle", log_n, pi, ci)
    finally:
        for h in hs:
            backend.col_free(h)
