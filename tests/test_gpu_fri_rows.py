"""The row-range and prover-only forms of the FRI and quotient kernels, op by op through the C ABI (shard_ops.hip), bit for bit:
k_fold_line / k_fold_circle with i0 != 0 and the challenge in device memory, k_fold_leaf with row0 != 0, the quotient kernels on a
row range, k_quotients_rows<2, LEAF>, and k_quotient_coeffs with the quotient launch on the coefficients it left on the device.
A row range's reference is the matching slice of the oracle's whole-domain result; k_quotient_coeffs has the Python-integer
reference of tests/shard_ref.py.  A slice handle is a column handle plus a word offset (a handle is the device address).  The
shapes are the smallest the wrappers' thresholds admit; none is the workload's size."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd import CmError
from cairo_m_amd.lib import set_framing
from tests import field_edges as fe
from tests import shard_ref as sr
from tests.field_edges import P
from tests.test_gpu_field_edges import ALPHAS, _quotient_inputs, _secure

pytestmark = pytest.mark.gpu
GUARD = 0xA5A5A5A5          # no M31 word
KINDS = ["const", "near_p", "edge_mix"]


def _free(backend, hs):
    for h in hs:
        backend.col_free(h)


def _at(h, words):
    """The handle of the slice of column h that starts `words` words in."""
    return int(h) + 4 * int(words)


def _ranges(n, parts):
    return [(k * (n // parts), n // parts) for k in range(parts)]


# ---- 1. fold rows --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fold_refs(oracle):
    """Per (log_n, kind): the source and destination columns and, per challenge, the oracle's whole-layer fold_line,
    fold_circle_into_line into a blank layer and fold_circle_into_line accumulating into dst.  Computed once."""
    cache = {}

    def get(log_n, kind):
        if (log_n, kind) not in cache:
            n = 1 << log_n
            rng = np.random.default_rng(900 + 10 * log_n + KINDS.index(kind))
            src, dst = _secure(kind, rng, n), _secure(kind, rng, n // 2)
            blank = [np.zeros(n // 2, dtype=np.uint32) for _ in range(4)]
            want = {}
            for alpha in ALPHAS:
                a = np.array(alpha, dtype=np.uint32)
                want[alpha] = {"line": oracle.fold_line(src, log_n, a), "circle": oracle.fold_circle_into_line(blank, src, log_n, a),
                               "circle+acc": oracle.fold_circle_into_line(dst, src, log_n, a)}
            cache[(log_n, kind)] = (src, dst, want)
        return cache[(log_n, kind)]
    return get


@pytest.mark.parametrize("log_n,ranges", [(10, _ranges(512, 2)), (10, _ranges(512, 4)), (10, _ranges(512, 8)), (11, _ranges(1024, 2)),
                                          (10, [(3, 301)])], ids=["2^10/2", "2^10/4", "2^10/8", "2^11/2", "2^10/i0=3,n=301"])
def test_fold_rows(backend, fold_refs, log_n, ranges):
    """cm_fri_fold_rows_op = fold_line_rows / fold_circle_into_line_rows: every range's outputs equal rows [i0, i0 + n_out) of the
    oracle's whole-layer fold — the twiddle is read at i0 + i, the data at the local i.  256, 128 and 64 outputs are one full block
    and then less than one (the i >= n_out guard), 512 are two blocks, (3, 301) is unaligned at both ends.  Both kernels, the circle
    fold blank and accumulating, the challenge as a kernel argument and in device memory, const(P-1) / near_p / edge_mix columns
    under every ALPHAS entry.  Each range writes into a slice of its own with a guard word behind it, which stays untouched."""
    half = 1 << (log_n - 1)
    tw = backend.twiddles(log_n + 1)
    try:
        for kind in KINDS:
            src, dst, want = fold_refs(log_n, kind)
            hs = [backend.upload(c) for c in src]
            # per coordinate, the ranges' output slices back to back: [n_out words | guard] ...
            offs = [int(o) for o in np.cumsum([0] + [n + 1 for _, n in ranges])]
            init = []
            for k in range(4):
                buf = np.full(offs[-1], GUARD, dtype=np.uint32)
                for (i0, n), o in zip(ranges, offs):
                    buf[o:o + n] = dst[k][i0:i0 + n]
                init.append(buf)
            try:
                for alpha in ALPHAS:
                    for mode in ("line", "circle", "circle+acc"):
                        for on_device in (False, True):
                            ho = [backend.upload(b) for b in init]
                            try:
                                for (i0, n), o in zip(ranges, offs):
                                    backend.fri_fold_rows([_at(h, o) for h in ho], [_at(h, 2 * i0) for h in hs], alpha, log_n, tw, i0, n,
                                                          circle=mode != "line", accumulate=mode == "circle+acc", alpha_on_device=on_device)
                                got = [backend.download(h, offs[-1]) for h in ho]
                            finally:
                                _free(backend, ho)
                            what = (kind, alpha, mode, "device challenge" if on_device else "host challenge")
                            for k in range(4):
                                for (i0, n), o in zip(ranges, offs):
                                    assert np.array_equal(got[k][o:o + n], want[alpha][mode][k][i0:i0 + n]), what + (k, i0, n)
                                    assert got[k][o + n] == GUARD, what + (k, i0, n, "guard")
            finally:
                _free(backend, hs)
        assert all(i0 + n <= half for i0, n in ranges)
    finally:
        backend.twiddles_free(tw)


# ---- 2. fold + leaves rows -----------------------------------------------------------------------------------------------
A_LINE, A_CIRCLE = ALPHAS[0], ALPHAS[2]      # two different challenges: one read in the other's place shows


@pytest.fixture(scope="module")
def leaf_refs(oracle):
    """Per (log_n, mode): edge_mix sources, the oracle's whole-layer fold and the leaf layer of oracle.merkle_commit over it."""
    cache = {}

    def get(log_n, mode):
        if (log_n, mode) not in cache:
            n, n_out = 1 << log_n, 1 << (log_n - 1)
            rng = np.random.default_rng(1700 + log_n)
            src, circ = _secure("edge_mix", rng, n), _secure("edge_mix", rng, n)
            want = np.zeros((4, n_out), dtype=np.uint32)
            if mode != "circle":
                want = oracle.fold_line(src, log_n, np.array(A_LINE, dtype=np.uint32))
            if mode != "line":
                want = oracle.fold_circle_into_line(want, circ, log_n, np.array(A_CIRCLE, dtype=np.uint32))
            _, layers = oracle.merkle_commit([np.ascontiguousarray(want[k]) for k in range(4)])
            cache[(log_n, mode)] = (src, circ, want, layers.reshape(-1, 8)[:n_out].copy())
        return cache[(log_n, mode)]
    return get


def _fold_leaves_ranges(backend, leaf_refs, log_n, mode, ranges, want_fused):
    src, circ, want, leaves = leaf_refs(log_n, mode)
    tw = backend.twiddles(log_n + 1)
    hs = [backend.upload(c) for c in src] if mode != "circle" else None
    hq = [backend.upload(c) for c in circ] if mode != "line" else None
    try:
        for row0, n in ranges:
            # four guard words behind the values, eight behind the hashes: both stay 16-byte aligned
            ho = [backend.upload(np.full(n + 4, GUARD, dtype=np.uint32)) for _ in range(4)]
            hh = backend.upload(np.full(8 * n + 8, GUARD, dtype=np.uint32))
            try:
                fused = backend.fri_fold_leaves_rows(None if hs is None else [_at(h, 2 * row0) for h in hs], A_LINE if hs else None, log_n, tw,
                                                     row0, n, ho, hh, circle4=None if hq is None else [_at(h, 2 * row0) for h in hq],
                                                     alpha_circle=A_CIRCLE if hq else None)
                got = np.stack([backend.download(h, n + 4) for h in ho])
                got_h = backend.download(hh, 8 * n + 8)
            finally:
                _free(backend, ho + [hh])
            assert fused == want_fused, (mode, row0, n)
            assert np.array_equal(got[:, :n], want[:, row0:row0 + n]), (mode, row0, n)
            assert np.array_equal(got_h[:8 * n].reshape(-1, 8), leaves[row0:row0 + n]), (mode, row0, n)
            assert (got[:, n:] == GUARD).all() and (got_h[8 * n:] == GUARD).all(), (mode, row0, n, "guard")
    finally:
        _free(backend, (hs or []) + (hq or []))
        backend.twiddles_free(tw)


@pytest.mark.parametrize("mode", ["line", "line+circle", "circle"])
@pytest.mark.parametrize("log_n,parts", [(16, 2), (17, 4)])
def test_fold_leaves_rows_fused(backend, leaf_refs, log_n, parts, mode):
    """k_fold_leaf<RFC, 0 | 1 | 2> on a row range (fold_line_leaf / fold_circle_leaf with row0, n_rows): ranges of 2^14 outputs, the
    smallest the wrapper serves, of a layer of 2^15 (two ranges) and 2^16 (four, so that row0 = 3 * 2^14 runs).  The twiddle
    pointers are offset by row0; values, sources and hashes are local.  `fused` is asserted, so a fall-back cannot pass for the
    kernel; the values equal the slice of the oracle's fold and the hashes the slice of the oracle's leaf layer."""
    _fold_leaves_ranges(backend, leaf_refs, log_n, mode, _ranges(1 << (log_n - 1), parts), 1)


@pytest.mark.parametrize("mode", ["line", "line+circle", "circle"])
def test_fold_leaves_rows_declined(backend, leaf_refs, mode):
    """What the wrapper declines runs the sharded prover's other route — the row-range folds with device challenges, then the leaf
    layer of the slice — with fused == 0 and the same values and hashes: ranges of 2^13 outputs (the first and one further in), a
    range of 2^14 whose row0 = 2^13 is no multiple of it, and any range under tuning "fri_fold_leaf" = 0."""
    _fold_leaves_ranges(backend, leaf_refs, 16, mode, [(0, 1 << 13), (3 << 13, 1 << 13), (1 << 13, 1 << 14)], 0)
    assert backend.L.cm_set_tuning(b"fri_fold_leaf", C.c_int32(0)) == 0
    try:
        _fold_leaves_ranges(backend, leaf_refs, 16, mode, [(1 << 14, 1 << 14)], 0)
    finally:
        backend.L.cm_set_tuning(b"fri_fold_leaf", C.c_int32(1))


# ---- 3. quotient rows ----------------------------------------------------------------------------------------------------
N_Q = 17


@pytest.fixture(scope="module")
def quot_refs(oracle):
    """Host columns per (log_n, kind) and the oracle's whole-domain quotients per (log_n, case); a case is a tuple of
    test_gpu_field_edges._quotient_cases' form.  Computed once and left unchanged."""
    cols, refs = {}, {}

    def get(log_n, case):
        if log_n not in cols:
            rng = np.random.default_rng(177 + log_n)
            n = 1 << log_n
            cols[log_n] = {"const": [fe.const(P - 1, n)] * N_Q, "edge_mix": [fe.edge_mix(rng, n) for _ in range(N_Q)]}
        if (log_n, case) not in refs:
            c, points, off, ci, values, coeff = _quotient_inputs(case, log_n, cols[log_n])
            refs[(log_n, case)] = oracle.accumulate_quotients(log_n, c, points, off, ci, values, coeff)
        return cols[log_n], refs[(log_n, case)]
    return get


def _quot_cases(nb_a, nb_b):
    """9 and 17 columns (every loop of every kernel has a tail) under the "ones" and "high01" coefficients on const(P-1) columns,
    and one case of edge_mix columns under a seeded coefficient, whose rows differ: a column read at the wrong row shows."""
    return [(9, nb_a, "const", "pm1", "ones"), (9, nb_b, "const", "uniform", "high01"), (17, nb_b, "const", "uniform", "ones"),
            (17, nb_a, "const", "pm1", "high01"), (17, nb_b, "edge_mix", "uniform", "uniform")]


@pytest.mark.parametrize("path,quot_rows,log_n,nb,parts", [
    ("rows2", 2, 14, (1, 2), (2, 4)), ("rows4", 4, 14, (1, 2), (2, 4)), ("one-row", 2, 14, (3, 3), (2, 4)),
    ("slices8", 2, 10, (1, 2), (2, 4)), ("slices64", 2, 5, (1, 2), (2,))], ids=["rows2", "rows4", "one_row", "slices8", "slices64"])
def test_quotient_rows(backend, quot_refs, path, quot_rows, log_n, nb, parts):
    """cm_accumulate_quotients_rows_op with row0 / n_rows, one launch path per case and the path word asserted: k_quotients_rows<2>
    and <4> at 2^14, k_quotients<1> (2^14 with three batches), k_quotients<8> at 2^10, k_quotients<64> at 2^5 — there two ranges of
    16 rows, multiples of the 4 rows of a block.  The domain point is taken at row0 + row, the columns at row: every range, run
    alone into a whole-domain buffer of guard words, equals the oracle's rows of that range and leaves every other word alone."""
    n = 1 << log_n
    assert backend.L.cm_set_tuning(b"quot_rows", C.c_int32(quot_rows)) == 0
    tw = backend.twiddles(log_n)
    dev = {}
    try:
        for case in _quot_cases(*nb):
            host_cols, want = quot_refs(log_n, case)
            if not dev:
                dev = {"const": [backend.upload(host_cols["const"][0])] * N_Q, "edge_mix": [backend.upload(c) for c in host_cols["edge_mix"]]}
            _, points, off, ci, values, coeff = _quotient_inputs(case, log_n, host_cols)
            for p in parts:
                for row0, m in _ranges(n, p):
                    ho = [backend.upload(np.full(n, GUARD, dtype=np.uint32)) for _ in range(4)]
                    try:
                        got_path = backend.accumulate_quotients_rows(log_n, [_at(h, row0) for h in dev[case[2]][:case[0]]], points, off, ci, values,
                                                                     coeff, [_at(h, row0) for h in ho], tw, row0=row0, n_rows=m)
                        got = np.stack([backend.download(h, n) for h in ho])
                    finally:
                        _free(backend, ho)
                    assert got_path == path, (case, row0, m)
                    assert np.array_equal(got[:, row0:row0 + m], want[:, row0:row0 + m]), (case, row0, m)
                    assert (got[:, :row0] == GUARD).all() and (got[:, row0 + m:] == GUARD).all(), (case, row0, m, "outside the range")
    finally:
        backend.L.cm_set_tuning(b"quot_rows", C.c_int32(2))
        _free(backend, dev.get("edge_mix", []) + dev.get("const", [])[:1])
        backend.twiddles_free(tw)


# ---- 4. quotient leaf ----------------------------------------------------------------------------------------------------
LEAF_CASES = [(9, 1, "const", "pm1", "ones"), (17, 2, "const", "uniform", "high01")]


@pytest.mark.parametrize("framing", ["", "hash_node=rfc"], ids=["raw", "rfc"])
@pytest.mark.parametrize("log_n,parts", [(17, 1), (18, 2)], ids=["2^17", "2^18/2"])
def test_quotient_leaf(backend, oracle, quot_refs, log_n, parts, framing):
    """k_quotients_rows<2, LEAF, RFC>, which both provers run for the largest size group: under "merkle_multi_top" = 17 (its lower
    bound) the whole domain of 2^17 rows (n_rows = 0, the single-GPU prover's launch) and 2^18 as two ranges of 2^17.  9 columns in
    one batch and 17 in two; the values equal the oracle's quotients, leaf_hashes the leaf layer of oracle.merkle_commit over the
    four output columns, under both hash_node framings; the path word is rows2-leaf."""
    n = 1 << log_n
    L = backend.L
    assert L.cm_set_tuning(b"merkle_multi_top", C.c_int32(17)) == 0
    tw = backend.twiddles(log_n)
    hc = None
    try:
        set_framing(framing, L)
        oracle.set_framing(framing)
        for case in LEAF_CASES:
            host_cols, want = quot_refs(log_n, case)
            if hc is None:
                hc = backend.upload(host_cols["const"][0])
            _, layers = oracle.merkle_commit([np.ascontiguousarray(want[k]) for k in range(4)])
            leaves = layers.reshape(-1, 8)[:n]
            _, points, off, ci, values, coeff = _quotient_inputs(case, log_n, host_cols)
            for row0, m in _ranges(n, parts):
                ho = [backend.upload(np.full(m + 4, GUARD, dtype=np.uint32)) for _ in range(4)]
                hh = backend.upload(np.full(8 * m + 8, GUARD, dtype=np.uint32))
                try:
                    got_path = backend.accumulate_quotients_rows(log_n, [_at(hc, row0)] * case[0], points, off, ci, values, coeff, ho, tw,
                                                                 row0=row0, n_rows=0 if parts == 1 else m, leaf_hashes=hh)
                    got = np.stack([backend.download(h, m + 4) for h in ho])
                    got_h = backend.download(hh, 8 * m + 8)
                finally:
                    _free(backend, ho + [hh])
                assert got_path == "rows2-leaf", (case, row0)
                assert np.array_equal(got[:, :m], want[:, row0:row0 + m]), (case, row0)
                assert np.array_equal(got_h[:8 * m].reshape(-1, 8), leaves[row0:row0 + m]), (case, row0)
                assert (got[:, m:] == GUARD).all() and (got_h[8 * m:] == GUARD).all(), (case, row0, "guard")
    finally:
        set_framing("", L)
        oracle.set_framing("")
        L.cm_set_tuning(b"merkle_multi_top", C.c_int32(19))
        if hc is not None:
            backend.col_free(hc)
        backend.twiddles_free(tw)


def test_quotient_leaf_refusals(backend):
    """The launches the LEAF kernel does not serve are refused by the entry, before any launch: three batches, "quot_rows" = 4, a
    range below 2^"merkle_multi_top" rows."""
    log_n, L = 17, backend.L
    n = 1 << log_n
    assert L.cm_set_tuning(b"merkle_multi_top", C.c_int32(17)) == 0
    tw = backend.twiddles(log_n)
    hc = backend.upload(fe.const(P - 1, n))
    ho = [backend.col_alloc(n) for _ in range(4)]
    hh = backend.col_alloc(8 * n)
    host = {"const": [None] * N_Q}

    def run(case, **kw):
        _, points, off, ci, values, coeff = _quotient_inputs(case, log_n, host)
        return backend.accumulate_quotients_rows(log_n, [hc] * case[0], points, off, ci, values, coeff, ho, tw, leaf_hashes=hh, **kw)
    try:
        assert run((9, 2, "const", "pm1", "ones")) == "rows2-leaf"
        with pytest.raises(CmError, match="does not serve"):
            run((9, 3, "const", "pm1", "ones"))
        with pytest.raises(CmError, match="does not serve"):
            run((9, 2, "const", "pm1", "ones"), row0=1 << 16, n_rows=1 << 16)
        assert L.cm_set_tuning(b"quot_rows", C.c_int32(4)) == 0
        with pytest.raises(CmError, match="does not serve"):
            run((9, 2, "const", "pm1", "ones"))
    finally:
        L.cm_set_tuning(b"quot_rows", C.c_int32(2))
        L.cm_set_tuning(b"merkle_multi_top", C.c_int32(19))
        _free(backend, [hc, hh] + ho)
        backend.twiddles_free(tw)


# ---- 5. k_quotient_coeffs ------------------------------------------------------------------------------------------------
COEF_SIZES = [1, 255, 256, 257, 600]
COEFFS = {"one": (1, 0, 0, 0), "u": (0, 0, 1, 0), "pm1": (P - 1,) * 4, "uniform": None}


def _sample_idx(rng, n_entries, n_samples):
    """Every sample at least once and the rest again: a permutation with repeats."""
    idx = np.concatenate([rng.permutation(n_samples), rng.integers(0, n_samples, size=n_entries - n_samples)])
    return rng.permutation(idx).astype(np.uint32)


@pytest.mark.parametrize("ckind", list(COEFFS))
def test_quotient_coeffs(backend, oracle, ckind):
    """k_quotient_coeffs through the entry's device_coeffs route: batches of 1, 255, 256, 257 and 600 entries in one call — one
    block each; the coeff^256 stride is taken only past 256 entries, once by 257 and twice by 600 — with sample_idx a permutation
    with repeats.  Sample values uniform, all P-1, and real (x, 0, 0, 0), whose a is 0; every point's y has words 2 and 3 at 2^30.
    Every word of coef_c, sum_a, sum_b and batch_coeff equals the Python-integer reference, and the quotients the launch then
    computes from them (2^5 rows, the column-sliced kernel: five batches) equal the oracle's."""
    rng = np.random.default_rng(2100 + list(COEFFS).index(ckind))
    coeff = COEFFS[ckind] or tuple(int(w) for w in rng.integers(0, P, size=4))
    log_n, n_cols, n_samples = 5, 3, 900
    off = np.cumsum([0] + COEF_SIZES).astype(np.uint32)
    n_entries = int(off[-1])
    points = rng.integers(0, P, size=(len(COEF_SIZES), 8), dtype=np.uint32)
    points[:, 6:8] = 2**30
    # (the oracle's binding regroups the entries column by column: within a batch the column index does not decrease, and every
    # batch starts at column 0, so that its grouping gives these batches back in this order)
    ci = np.concatenate([(np.arange(size) * n_cols) // size for size in COEF_SIZES]).astype(np.uint32)
    cols = [rng.integers(0, P, size=1 << log_n, dtype=np.uint32) for _ in range(n_cols)]
    tw = backend.twiddles(log_n)
    hs = [backend.upload(c) for c in cols]
    ho = [backend.col_alloc(1 << log_n) for _ in range(4)]
    try:
        for vkind in ("uniform", "pm1", "real"):
            samples = rng.integers(0, P, size=(n_samples, 4), dtype=np.uint32)
            if vkind == "pm1":
                samples[:] = P - 1
            if vkind == "real":
                samples[:, 1:] = 0
            si = _sample_idx(rng, n_entries, n_samples)
            path, cc, sum_a, sum_b, bc = backend.accumulate_quotients_rows(log_n, hs, points, off, ci, samples, coeff, ho, tw, sample_idx=si)
            got = np.stack([backend.download(h, 1 << log_n) for h in ho])
            assert path == "slices64"
            for k, size in enumerate(COEF_SIZES):
                lo, hi = int(off[k]), int(off[k + 1])
                w_cc, w_a, w_b, w_bc = sr.quotient_coeffs(coeff, points[k][4:], samples[si[lo:hi]])
                what = (ckind, vkind, size)
                assert [tuple(int(w) for w in r) for r in cc[lo:hi]] == w_cc, what
                assert tuple(int(w) for w in sum_a[k]) == w_a and tuple(int(w) for w in sum_b[k]) == w_b, what
                assert tuple(int(w) for w in bc[k]) == w_bc, what
                if vkind == "real":
                    assert w_a == (0, 0, 0, 0), what
            want = oracle.accumulate_quotients(log_n, cols, points, off, ci, samples[si], np.array(coeff, dtype=np.uint32))
            assert np.array_equal(got, want), (ckind, vkind)
    finally:
        _free(backend, hs + ho)
        backend.twiddles_free(tw)


def test_quotients_from_device_coefficients(backend, quot_refs):
    """The provers' route from samples to quotients at 2^14 rows x 17 columns: k_quotient_coeffs fills coef_c and the batch sums on
    the device and k_quotients_rows<2> reads them there — the whole domain, then two ranges; equal to the oracle's quotients."""
    log_n = 14
    n = 1 << log_n
    tw = backend.twiddles(log_n)
    dev = []
    try:
        for case in [(17, 2, "edge_mix", "uniform", "uniform"), (17, 2, "const", "uniform", "high01")]:
            host_cols, want = quot_refs(log_n, case)
            dev = dev or [backend.upload(c) for c in host_cols["edge_mix"]] + [backend.upload(host_cols["const"][0])]
            hcols = dev[:N_Q] if case[2] == "edge_mix" else [dev[N_Q]] * N_Q
            _, points, off, ci, values, coeff = _quotient_inputs(case, log_n, host_cols)
            si = np.random.default_rng(5).permutation(ci.size).astype(np.uint32)
            samples = np.empty_like(values)
            samples[si] = values                      # entry e's value sits at samples[si[e]]
            for row0, m in [(0, 0)] + _ranges(n, 2):
                ho = [backend.upload(np.full(n, GUARD, dtype=np.uint32)) for _ in range(4)]
                try:
                    res = backend.accumulate_quotients_rows(log_n, [_at(h, row0) for h in hcols], points, off, ci, samples, coeff,
                                                            [_at(h, row0) for h in ho], tw, row0=row0, n_rows=m, sample_idx=si)
                    got = np.stack([backend.download(h, n) for h in ho])
                finally:
                    _free(backend, ho)
                m = m or n
                assert res[0] == "rows2", (case, row0)
                assert np.array_equal(got[:, row0:row0 + m], want[:, row0:row0 + m]), (case, row0)
                assert (got[:, :row0] == GUARD).all() and (got[:, row0 + m:] == GUARD).all(), (case, row0, "outside the range")
    finally:
        _free(backend, dev)
        backend.twiddles_free(tw)
