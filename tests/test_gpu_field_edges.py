"""The lazily folded field arithmetic of the hot path (field.hpp, gpu_air.hpp, kernels_fri.hip, kernels_poly.hip) at the
words its unit-count bounds are tight at — 0 (negative carried as P), P-1 in every slot, 2^30 / 2^30-1 (doubled operands) —
op by op through the C ABI, bit-exact against the CPU oracle and, where tests/field_edges.py has one, against the Python
big-integer reference.  The shapes are the smallest that reach each code path; none is the workload's size."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import N_COMPONENTS, N_PREPROCESSED, PREPROCESSED_LOG, synth_fibonacci
from tests import field_edges as fe
from tests.field_edges import EDGE, P

pytestmark = pytest.mark.gpu
PM1_4 = (P - 1,) * 4
ALPHAS = [PM1_4, (0, P - 1, 0, P - 1), (2**30,) * 4]
C_RET, C_POSEIDON2, C_RC8 = 4, 29, 30


def _free(backend, hs):
    for h in hs:
        backend.col_free(h)


def _secure(kind, rng, n):
    """Four coordinate columns of one kind."""
    if kind == "const":
        return [fe.const(P - 1, n) for _ in range(4)]
    return [fe.near_p(rng, n) if kind == "near_p" else fe.edge_mix(rng, n) for _ in range(4)]


# ---- 1. inverses ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
def test_batch_inverse_qm31_edges(backend, oracle, shuffled):
    """k_inverse_qm31: QM31 operator*, CM31 operator*, inv(CM31) and m31_fold64 over all of E6^4 but zero — 1295 elements, an odd
    length on purpose; again after a seeded shuffle because the prefix products of a batch inverse depend on the order."""
    xs = fe.e6_tuples()
    if shuffled:
        xs = [xs[i] for i in np.random.default_rng(31).permutation(len(xs))]
    n = len(xs)
    a = np.array(xs, dtype=np.uint32)
    hs = [backend.upload(np.ascontiguousarray(a[:, k])) for k in range(4)]
    ho = [backend.col_alloc(n) for _ in range(4)]
    backend.batch_inverse_qm31(hs, ho, n)
    got = np.stack([backend.download(o, n) for o in ho], axis=1)
    _free(backend, hs + ho)
    assert np.array_equal(got, oracle.qm31_inv(a.reshape(-1)).reshape(n, 4))
    assert all(fe.q_mul(x, tuple(int(w) for w in g)) == (1, 0, 0, 0) for x, g in zip(xs, got))


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_batch_inverse_m31_edges(backend, oracle, n):
    """k_inverse_m31 (M31 operator* on the doubled operand) over EDGE without 0, tiled to one element, one block less one, one
    block, one block and one."""
    a = np.resize(np.array([w for w in EDGE if w], dtype=np.uint32), n)
    h, o = backend.upload(a), backend.col_alloc(n)
    backend.batch_inverse_m31(h, o, n)
    got = backend.download(o, n)
    _free(backend, [h, o])
    assert np.array_equal(got, oracle.m31_inv(a))
    assert all(fe.m_mul(int(x), int(y)) == 1 for x, y in zip(a, got))


# ---- 2. powers -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("felt", [PM1_4, (0, P - 1, 0, P - 1), (P - 1, 0, P - 1, 0), (2**30,) * 4, (0, 0, 0, 1), (0, 0, 1, 0)])
def test_secure_powers_edges(backend, felt):
    """cm_generate_secure_powers: a chain of QM31 products (20 mads, 2 partial folds each) started at the operands whose
    negatives and doubles are the extreme ones."""
    pw = backend.secure_powers(np.array(felt, dtype=np.uint32), 9)
    assert [tuple(int(w) for w in r) for r in pw] == [fe.q_pow(felt, k) for k in range(9)]


# ---- 3. transforms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [1, 5, 11, 13, 18])
def test_transforms_edges(backend, oracle, log_n):
    """The FFT passes: mul_tw2 with a = P-1, butterfly add and sub at both ends (0 +- 0, (P-1) +- (P-1), 0 - (P-1)) — interpolate,
    evaluate to log_n + 1 and interpolate_extend out of place on const(P-1), alt and edge_mix; 2^18 is the smallest size of the
    fused sweep.  The transform of a constant column is the constant term alone: that needs no oracle."""
    n = 1 << log_n
    cols = [fe.const(P - 1, n), fe.alt(n), fe.edge_mix(np.random.default_rng(300 + log_n), n)]
    want_c = [oracle.interpolate(c) for c in cols]
    want_l = [oracle.evaluate(c, log_n + 1) for c in want_c]
    assert want_c[0][0] == P - 1 and not want_c[0][1:].any()
    tw = backend.twiddles(log_n + 1)
    hs = [backend.upload(c) for c in cols]
    backend.interpolate(hs, log_n, tw)
    got_c = [backend.download(h, n) for h in hs]
    ho = [backend.col_alloc(2 * n) for _ in cols]
    backend.evaluate(hs, log_n, log_n + 1, tw, ho)
    got_l = [backend.download(h, 2 * n) for h in ho]
    ev = [backend.upload(c) for c in cols]
    co, ld = [backend.col_alloc(n) for _ in cols], [backend.col_alloc(2 * n) for _ in cols]
    backend.interpolate_extend(ev, co, ld, log_n, tw)
    got_c2, got_l2 = [backend.download(h, n) for h in co], [backend.download(h, 2 * n) for h in ld]
    _free(backend, hs + ho + ev + co + ld)
    backend.twiddles_free(tw)
    assert got_c[0][0] == P - 1 and not got_c[0][1:].any()
    for k in range(3):
        assert np.array_equal(got_c[k], want_c[k]), ("interpolate", k)
        assert np.array_equal(got_l[k], want_l[k]), ("evaluate", k)
        assert np.array_equal(got_c2[k], want_c[k]), ("interpolate_extend coefficients", k)
        assert np.array_equal(got_l2[k], want_l[k]), ("interpolate_extend extension", k)


# ---- 4. eval_at_point ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [3, 11, 12, 13, 15])
def test_eval_at_point_edges(backend, oracle, log_n):
    """cm_eval_at_point, which runs eval_at_point_batch: k_point_table (the QM31 products of the point tables),
    k_eval_at_point_partial (one block per chunk of 2^EAP_LOW_BITS = 2^12 coefficients, a QM31 * M31 product per coefficient, the
    block's sum times the chunk's high-table entry) and k_reduce_partials.  2^3 and 2^11 are less than a chunk, 2^12 is exactly
    one, 2^13 is two — the path's own chunk boundary — and 2^15 is eight.  The provers do not sample through this path: their
    kernels (k_eval_partial_multi and the rest of eval_at_point_multi) get the same columns and points, from the same seeds, in
    test_worst_case_columns_on_both_paths of tests/test_gpu_eval_points.py, the file that steers those kernels further."""
    n = 1 << log_n
    rng = np.random.default_rng(500 + log_n)
    cols = [fe.const(P - 1, n), fe.near_p(rng, n), fe.edge_mix(rng, n), fe.alt(n)]
    hs = [backend.upload(c) for c in cols]
    for pt in (rng.integers(0, P, size=8, dtype=np.uint32), fe.edge_mix(rng, 8)):
        got = backend.eval_at_point(hs, log_n, pt)
        for g, c in zip(got, cols):
            assert np.array_equal(g, oracle.eval_at_point(c, pt)), pt
    _free(backend, hs)


# ---- 5. FRI folds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", [2, 8])
def test_fri_folds_edges(backend, oracle, log_n):
    """k_fold_line and k_fold_circle (QM31 * QM31 with alpha, QM31 * M31 with the doubled inverse twiddle, the sums and
    differences of both ends) with source and destination const(P-1), near_p, edge_mix and alpha at its extreme words."""
    n = 1 << log_n
    tw = backend.twiddles(log_n + 1)
    for ki, kind in enumerate(["const", "near_p", "edge_mix"]):
        rng = np.random.default_rng(600 + 10 * log_n + ki)
        src, dst = _secure(kind, rng, n), _secure(kind, rng, n // 2)
        hs = [backend.upload(c) for c in src]
        for alpha in ALPHAS:
            a = np.array(alpha, dtype=np.uint32)
            ho = [backend.col_alloc(n // 2) for _ in range(4)]
            backend.fri_fold_line(hs, a, log_n, tw, ho)
            got = np.stack([backend.download(h, n // 2) for h in ho])
            assert np.array_equal(got, oracle.fold_line(src, log_n, a)), ("fold_line", kind, alpha)
            hd = [backend.upload(c) for c in dst]
            backend.fri_fold_circle_into_line(hd, hs, a, log_n, tw)
            got = np.stack([backend.download(h, n // 2) for h in hd])
            assert np.array_equal(got, oracle.fold_circle_into_line(dst, src, log_n, a)), ("fold_circle", kind, alpha)
            _free(backend, ho + hd)
        _free(backend, hs)
    backend.twiddles_free(tw)


@pytest.mark.parametrize("mode", ["line", "line+circle", "circle"])
def test_fold_line_leaves_edges(backend, oracle, mode):
    """k_fold_leaf at 2^15, the smallest size it serves, in its three modes: the folded layer equals the oracle's fold_line /
    fold_circle_into_line and every leaf hash the oracle's commitment layer over the four coordinate columns."""
    log_n = 15
    n, n_out = 1 << log_n, 1 << (log_n - 1)
    tw = backend.twiddles(log_n + 1)
    for ki, kind in enumerate(["const", "near_p", "edge_mix"]):
        rng = np.random.default_rng(700 + ki)
        src, circ = _secure(kind, rng, n), _secure(kind, rng, n)
        hs = [backend.upload(c) for c in src] if mode != "circle" else None
        hq = [backend.upload(c) for c in circ] if mode != "line" else None
        for alpha in ALPHAS:
            a = np.array(alpha, dtype=np.uint32)
            want = np.zeros((4, n_out), dtype=np.uint32)
            if hs:
                want = oracle.fold_line(src, log_n, a)
            if hq:
                want = oracle.fold_circle_into_line(want, circ, log_n, a)
            ho = [backend.col_alloc(n_out) for _ in range(4)]
            hh = backend.col_alloc(8 * n_out)
            backend.fri_fold_line_leaves(hs, a if hs else None, log_n, tw, ho, hh, circle4=hq, alpha_circle=a if hq else None)
            got = np.stack([backend.download(h, n_out) for h in ho])
            got_h = backend.download(hh, 8 * n_out).reshape(-1, 8)
            _free(backend, ho + [hh])
            assert np.array_equal(got, want), (kind, alpha)
            _, layers = oracle.merkle_commit([np.ascontiguousarray(want[k]) for k in range(4)])
            assert np.array_equal(got_h, layers.reshape(-1, 8)[:n_out]), (kind, alpha)
        _free(backend, (hs or []) + (hq or []))
    backend.twiddles_free(tw)


# ---- 6. DEEP quotients ---------------------------------------------------------------------------------------------------
Q_SIZES = [1, 3, 4, 5, 7, 8, 9, 16, 17, 25, 40]
Q_MAX = 40
# random_coeff kinds.  "ones": coeff = 1 and a sample point whose y has words 2 and 3 equal to 2^30, so that conj_u(y) - y =
# (0, 0, -2^31, -2^31) = (0, 0, P-1, P-1) is EVERY entry's coefficient.  "u": coeff = u = (0, 0, 1, 0) with the same point, the
# powers cycle through the coordinates: -(1 + i) u^(k+1) puts small negatives into coordinates 0 and 1 too.  "high01": a fixed
# coefficient (found by a seeded search with the Python reference, point y = (.., 2^30, 2^30)) under which coordinates 0 and 1
# each carry five consecutive entries whose raw products with P-1 do not fit a u64 together.  "uniform": seeded.
Q_COEFFS = {"ones": (1, 0, 0, 0), "u": (0, 0, 1, 0), "high01": (1711792828, 3870524, 83707791, 1705168718), "uniform": None}


def _quotient_cases():
    """(first batch size, batches, column kind, sample-value kind, coefficient kind).  Every size runs its worst case — const(P-1)
    columns under the all-(P-1) coefficients — with one and with two batches, and a second variant that rotates through the other
    column, value and coefficient kinds; one case has three batches."""
    kinds, vals, coefs = ["near_p", "edge_mix", "const"], ["uniform", "pm1"], ["u", "uniform", "high01", "ones"]
    cases, r = [], 0
    for n0 in Q_SIZES:
        for nb in (1, 2):
            cases.append((n0, nb, "const", "pm1" if nb == 1 else "uniform", "ones"))
            cases.append((n0, nb, kinds[r % 3], vals[r % 2], coefs[r % 4]))
            r += 1
    cases.append((Q_MAX, 2, "const", "pm1", "u"))
    cases.append((Q_MAX, 1, "const", "pm1", "high01"))
    cases.append((17, 3, "const", "pm1", "ones"))
    return cases


def _quotient_inputs(case, log_n, cols_by_kind):
    n0, nb, kind, vkind, ckind = case
    rng = np.random.default_rng(8000 + 97 * n0 + 7 * nb + log_n)
    points = rng.integers(0, P, size=(nb, 8), dtype=np.uint32)   # all words random: not on the domain, no zero denominator
    if ckind in ("ones", "u", "high01"):
        points[:, 6:8] = 2**30
    batches = [list(range(n0)), list(range(0, n0, 3)), list(range(0, n0, 5))][:nb]
    col_index = np.array(sum(batches, []), dtype=np.uint32)
    batch_off = np.cumsum([0] + [len(b) for b in batches]).astype(np.uint32)
    values = rng.integers(0, P, size=(col_index.size, 4), dtype=np.uint32) if vkind == "uniform" else np.full((col_index.size, 4), P - 1, dtype=np.uint32)
    coeff = Q_COEFFS[ckind]
    if ckind == "uniform":
        coeff = rng.integers(0, P, size=4, dtype=np.uint32)
    return cols_by_kind[kind][:n0], points, batch_off, col_index, values, np.array(coeff, dtype=np.uint32)


@pytest.fixture(scope="module")
def quotient_refs(oracle):
    """Host columns per (log_n, kind) and the oracle's result per (log_n, case): computed once, shared by the launch paths of a
    size (the three kernels at 2^14 must all give these words)."""
    cols, refs = {}, {}

    def get(log_n, case):
        if log_n not in cols:
            rng = np.random.default_rng(77 + log_n)
            n = 1 << log_n
            cols[log_n] = {"const": [fe.const(P - 1, n) for _ in range(Q_MAX)], "near_p": [fe.near_p(rng, n) for _ in range(Q_MAX)],
                           "edge_mix": [fe.edge_mix(rng, n) for _ in range(Q_MAX)]}
        if (log_n, case) not in refs:
            c, points, off, ci, values, coeff = _quotient_inputs(case, log_n, cols[log_n])
            refs[(log_n, case)] = oracle.accumulate_quotients(log_n, c, points, off, ci, values, coeff)
        return cols[log_n], refs[(log_n, case)]
    return get


def _runs_at_least(flags, k):
    best = cur = 0
    for f in flags:
        cur = cur + 1 if f else 0
        best = max(best, cur)
    return best >= k


@pytest.mark.parametrize("quot_rows,log_n", [(2, 14), (4, 14), (1, 14), (None, 10), (None, 3)],
                         ids=["rows2", "rows4", "one_row_16_group", "slices8", "slices64"])
def test_accumulate_quotients_edges(backend, oracle, quotient_refs, quot_rows, log_n):
    """cm_accumulate_quotients with resolved entry columns, one launch path per case: quot_rows = 2 / 4 at 2^14 reach
    k_quotients_rows<2> (the kernel the prover runs) / <4> — CH = 8 / 4 columns per step, a fold every fourth column, the
    one-column tail, one shared inversion of the 2R denominators; quot_rows = 1 reaches k_quotients<1> with its 16-group, 8-group
    and tail loops; 2^10 and 2^3 reach the column-sliced k_quotients<8> / <64>; three batches fall back to k_quotients<1> under
    every setting.  The first-batch sizes cross every loop boundary of the three kernels (multiples of 4, 8 and 16, one less, one
    more), the second batch is every third column.  The LEAF variant of k_quotients_rows shares the accumulation code tested here;
    its leaf hashes, and every kernel here on a row range, are held to the oracle by test_quotient_leaf and test_quotient_rows
    of tests/test_gpu_fri_rows.py.

    The coefficient a kernel multiplies a column by is coeff^(k+1) * (conj_u(y) - y); its words 0 and 1 are zero whenever coeff
    lies in CM31, so all four words of EVERY entry cannot be P-1 at once.  What is asserted below, from the Python reference, about
    the cases that ran: coordinates 2 and 3 carry a word >= P-8 in at least eight consecutive entries of a batch (all forty, under
    "ones"); coordinates 0 and 1 carry a word >= P-8 within eight consecutive entries (under "u"), and five consecutive entries
    whose products with P-1 overflow a u64 when summed unfolded (under "high01") — so a fold one column late is caught in each
    of the four coordinates."""
    L = backend.L
    if quot_rows is not None:
        assert L.cm_set_tuning(b"quot_rows", C.c_int32(quot_rows)) == 0
    tw = backend.twiddles(log_n)
    n = 1 << log_n
    dev = {}
    ho = [backend.col_alloc(n) for _ in range(4)]
    eight, within8, overflow5 = [False] * 4, [False] * 4, [False] * 4
    try:
        for case in _quotient_cases():
            host_cols, want = quotient_refs(log_n, case)
            if not dev:
                dev = {k: [backend.upload(c) for c in v] for k, v in host_cols.items()}
            _, points, off, ci, values, coeff = _quotient_inputs(case, log_n, host_cols)
            if case[4] != "uniform":
                coefs = fe.quotient_coefs(coeff, points[0][4:], case[0])
                for j in range(4):
                    hi = [c[j] >= P - 8 for c in coefs]
                    eight[j] |= _runs_at_least(hi, 8)
                    within8[j] |= len(coefs) >= 8 and any(any(hi[s:s + 8]) for s in range(len(coefs) - 7))
                    overflow5[j] |= any(sum((P - 1) * c[j] for c in coefs[s:s + 5]) >= 2**64 for s in range(max(0, len(coefs) - 4)))
            backend.accumulate_quotients(log_n, dev[case[2]][:case[0]], points, off, ci, values, coeff, ho, tw)
            got = np.stack([backend.download(h, n) for h in ho])
            assert np.array_equal(got, want), (case, np.argwhere(got != want)[:4].tolist())
    finally:
        if quot_rows is not None:
            L.cm_set_tuning(b"quot_rows", C.c_int32(2))
        _free(backend, ho + [h for v in dev.values() for h in v])
        backend.twiddles_free(tw)
    assert eight[2] and eight[3], eight
    assert all(within8), within8
    assert all(overflow5), overflow5


# ---- 7. LogUp denominators, norms and the constraint accumulator ---------------------------------------------------------
def _lde(backend, cols, log, tw):
    hs = [backend.upload(c) for c in cols]
    backend.interpolate(hs, log, tw)
    out = [backend.col_alloc(2 << log) for _ in cols]
    backend.evaluate(hs, log, log + 1, tw, out)
    _free(backend, hs)
    return out


@pytest.fixture(scope="module")
def fib_components(backend, oracle):
    """synth_fibonacci(37): the preprocessed columns and their extensions, and every component's trace columns on the device
    (checked against the oracle once) — what test_trace_histogram_interaction_constraints_per_component sets up per run."""
    tw = backend.twiddles(22)
    pp_cols = []
    for k in range(N_PREPROCESSED):
        h = backend.col_alloc(1 << PREPROCESSED_LOG[k])
        backend.preprocessed_column(k, h)
        pp_cols.append(h)
    pp_lde = [_lde(backend, [backend.download(h, 1 << PREPROCESSED_LOG[k])], PREPROCESSED_LOG[k], tw)[0] for k, h in enumerate(pp_cols)]
    inp = synth_fibonacci(37)
    dev = backend.upload_input(inp)
    mult = [backend.upload(np.zeros(1 << lg, dtype=np.uint32)) for lg in (8, 16, 20, 18)]
    comps = []
    for cid in range(N_COMPONENTS):
        n_tr, n_it, n_cons = backend.component_info(cid)
        log = backend.component_log_size(dev, cid)
        if cid <= C_POSEIDON2:
            cols = [backend.col_alloc(1 << log) for _ in range(n_tr)]
            backend.trace_write(dev, cid, cols)
            if cid < 26:
                backend.histogram(cid, cols, log, *mult)
        else:
            cols = [mult[cid - C_RC8]]
        host = np.stack([backend.download(h, 1 << log) for h in cols])
        assert np.array_equal(host, oracle.component_trace(inp.view, cid)), (cid, "trace")
        tr_lde = _lde(backend, list(host), log, tw) if log <= 12 else []
        comps.append(dict(cid=cid, log=log, n_it=n_it, n_cons=n_cons, cols=cols, host=host, tr_lde=tr_lde))
    yield dict(tw=tw, pp_cols=pp_cols, pp_lde=pp_lde, inp=inp, comps=comps)
    for c in comps:
        _free(backend, c["tr_lde"] + (c["cols"] if c["cid"] <= C_POSEIDON2 else []))
    _free(backend, mult + pp_cols + pp_lde)
    backend.free_input(dev)
    inp.free()
    backend.twiddles_free(tw)


@pytest.mark.parametrize("name,rel", fe.relation_settings(), ids=[s[0] for s in fe.relation_settings()])
def test_logup_and_constraints_under_steered_relations(backend, oracle, fib_components, name, rel):
    """dev_combine (QAcc::add / QAcc::value), the entry-wise LogUp norm re / im of flush(), and the constraint accumulator
    (QAcc::add_q) for all 34 components of fibonacci(37): with rel_z_only every LogUp denominator is exactly -z, all four words
    chosen by the test ((1, P-1, 0, P-1) makes the norm's P - b0 equal P while b1d = 2P - 2); rel_all(P-1) puts P-1 into every
    alpha power; the constraint powers are all P-1, then drawn from EDGE.  Interaction columns and claimed sums equal
    oracle.component_interaction, accumulators oracle.component_constraints (constraints for log <= 12 as in
    test_gpu_components.py)."""
    f = fib_components
    for c in f["comps"]:
        cid, log = c["cid"], c["log"]
        out = [backend.col_alloc(1 << log) for _ in range(c["n_it"])]
        cs = backend.interaction_write(cid, c["cols"], f["pp_cols"], log, rel, out)
        got_it = np.stack([backend.download(h, 1 << log) for h in out])
        _free(backend, out)
        want_it, want_cs = oracle.component_interaction(f["inp"].view, cid, rel, c["n_it"], log)
        assert np.array_equal(got_it, want_it), (name, cid, "interaction", np.argwhere(got_it != want_it)[:4].tolist())
        assert np.array_equal(cs, want_cs), (name, cid, "claimed sum")
        if cid == C_RET and name.startswith("z_only"):
            b0, b4 = fe.ret_row0_reference(tuple(int(w) for w in rel[:4]), int(c["host"][0][0]))
            assert tuple(int(w) for w in got_it[0:4, 0]) == b0 and tuple(int(w) for w in got_it[16:20, 0]) == b4
        if log <= 12:
            it_lde = _lde(backend, list(got_it), log, f["tw"])
            for kind in ("pm1", "edge"):
                coeff = fe.constraint_coeffs(kind, c["n_cons"], cid)
                acc = [backend.upload(np.zeros(2 << log, dtype=np.uint32)) for _ in range(4)]
                backend.constraints_accumulate(cid, c["tr_lde"], it_lde, f["pp_lde"], log, rel, coeff, cs, acc)
                got_acc = np.stack([backend.download(h, 2 << log) for h in acc])
                _free(backend, acc)
                want_acc = oracle.component_constraints(f["inp"].view, cid, rel, coeff, log)
                assert np.array_equal(got_acc, want_acc), (name, cid, kind, "constraints", np.argwhere(got_acc != want_acc)[:4].tolist())
            _free(backend, it_lde)
