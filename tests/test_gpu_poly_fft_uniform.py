"""GPU parity for the transform kernels whose wave-uniform twiddle indices come from scalar code (kernels_fft.hip,
CM_FFT_UNIFORM_TW): every round geometry and every uniform / per-lane classification at the smallest size where it occurs,
word for word against the CPU oracle.

  cm_interpolate_extend  2^18 .. 2^21   the fused sweep, W = 6 .. 9 (W = 9 is the one shape with a per-lane round), 1 and 3
                                        columns (blockIdx.y > 0)
  cm_interpolate / cm_evaluate  2^13 .. 2^17   the 2^11-tile strided passes, W = 1 .. 5
                                2^22           13 + 9: the 2^14-tile strided pass behind the 13-layer contiguous one
                                2^23           12 + 6 + 5: two strided passes, one column
  cm_evaluate zero-padded  10->12, 12->14, 16->19, 18->20   the first pass reads implicit zeros

Inputs: distinct random words (an affine map i -> a i + b mod P with random a != 0, b) and a column of P - 1 in every word,
the largest canonical value: the inverse scaling by 2^-n, done as a 31-bit rotation, must keep it canonical.  Inputs and the
oracle's answers are computed once per (kind, size) and shared.

The file sorts next to tests/test_gpu_poly_merkle.py on purpose: both allocate and free columns of many sizes straight from the
driver, and tests/test_gpu_memory.py, which compares the pool's counters with the driver's free bytes to within one 8 MiB granule
(the driver's cached 2 MiB chunks already take 6 of them in the suite's order), runs before either."""
import functools

import numpy as np
import pytest

from tests.fft_op_sizes import EVALUATE_PADDED

P = 2**31 - 1
pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def column(kind, log_n):
    """kind = "pm1": P - 1 everywhere; an integer: distinct random words from that seed.  Read-only."""
    if kind == "pm1":
        c = np.full(1 << log_n, P - 1, dtype=np.uint32)
    else:
        rng = np.random.default_rng(52000 + 100 * kind + log_n)
        a, b = int(rng.integers(1, P)), int(rng.integers(0, P))
        c = ((np.arange(1 << log_n, dtype=np.uint64) * np.uint64(a) + np.uint64(b)) % np.uint64(P)).astype(np.uint32)
    c.setflags(write=False)
    return c


def columns(ncols, log_n):
    return [column(k, log_n) for k in (0, "pm1", 1)[:ncols]]


_ORACLE_CACHE = {}


def ref_interpolate(oracle, kind, log_n):
    key = ("i", kind, log_n)
    if key not in _ORACLE_CACHE:
        r = oracle.interpolate(column(kind, log_n))
        r.setflags(write=False)
        _ORACLE_CACHE[key] = r
    return _ORACLE_CACHE[key]


def ref_extension(oracle, kind, log_n):
    """oracle's evaluation on the double domain of the oracle's coefficients of column(kind, log_n)"""
    key = ("e", kind, log_n)
    if key not in _ORACLE_CACHE:
        r = oracle.evaluate(ref_interpolate(oracle, kind, log_n), log_n + 1)
        r.setflags(write=False)
        _ORACLE_CACHE[key] = r
    return _ORACLE_CACHE[key]


KINDS = (0, "pm1", 1)


@pytest.mark.parametrize("ncols", [1, 3])
@pytest.mark.parametrize("log_n", [18, 19, 20, 21])
def test_fused_sweep(backend, oracle, log_n, ncols):
    from cairo_m_amd.lib import fft_extend_fused
    assert fft_extend_fused(log_n), "this size no longer takes the fused sweep: the test would not run k_fft_fused_rb"
    tw = backend.twiddles(log_n + 1)
    cols = columns(ncols, log_n)
    ev = [backend.upload(c) for c in cols]
    co = [backend.col_alloc(1 << log_n) for _ in cols]
    ld = [backend.upload(np.full(2 << log_n, 0x5A5A5A5A, dtype=np.uint32)) for _ in cols]   # a skipped word must not pass
    backend.interpolate_extend(ev, co, ld, log_n, tw)
    for kind, c_h, l_h in zip(KINDS, co, ld):
        assert np.array_equal(backend.download(c_h, 1 << log_n), ref_interpolate(oracle, kind, log_n)), (log_n, kind)
        assert np.array_equal(backend.download(l_h, 2 << log_n), ref_extension(oracle, kind, log_n)), (log_n, kind)
    for h in ev + co + ld:
        backend.col_free(h)
    backend.twiddles_free(tw)


def ref_evaluate(oracle, kind, n_in, n_out):
    """oracle's evaluation on the domain of 2^n_out of the words of column(kind, n_in) taken as coefficients"""
    key = ("f", kind, n_in, n_out)
    if key not in _ORACLE_CACHE:
        r = oracle.evaluate(column(kind, n_in), n_out)
        r.setflags(write=False)
        _ORACLE_CACHE[key] = r
    return _ORACLE_CACHE[key]


def _interpolate_evaluate(backend, oracle, log_n, kinds):
    """the plan of 2^n in both directions: cm_interpolate at 2^n; cm_evaluate onto 2^n from 2^n coefficients (every layer with
    its twiddles) and from 2^(n-1) (the extension by two: the top layer copies), each against the oracle"""
    tw = backend.twiddles(log_n)
    hs = [backend.upload(column(k, log_n)) for k in kinds]
    backend.interpolate(hs, log_n, tw)
    for kind, h in zip(kinds, hs):
        assert np.array_equal(backend.download(h, 1 << log_n), ref_interpolate(oracle, kind, log_n)), (log_n, kind)
    for h in hs:   # the same words again, now as coefficients
        backend.col_free(h)
    hs = [backend.upload(column(k, log_n)) for k in kinds]
    half = [backend.upload(column(k, log_n - 1)) for k in kinds]
    outs = [backend.upload(np.full(1 << log_n, 0x5A5A5A5A, dtype=np.uint32)) for _ in kinds]
    for src, n_in in ((hs, log_n), (half, log_n - 1)):
        backend.evaluate(src, n_in, log_n, tw, outs)
        for o, kind in zip(outs, kinds):
            assert np.array_equal(backend.download(o, 1 << log_n), ref_evaluate(oracle, kind, n_in, log_n)), (n_in, log_n, kind)
    for h in hs + half + outs:
        backend.col_free(h)
    backend.twiddles_free(tw)


@pytest.mark.parametrize("log_n", [13, 14, 15, 16, 17])
def test_short_strided_passes(backend, oracle, log_n):
    from cairo_m_amd.lib import fft_plan
    assert fft_plan(log_n)[-1] == (12, log_n, 11, 11 - (log_n - 12)), "the plan no longer ends with a 2^11-tile strided pass here"
    _interpolate_evaluate(backend, oracle, log_n, KINDS)


def test_thirteen_plus_nine(backend, oracle):
    from cairo_m_amd.lib import fft_plan
    assert fft_plan(22) == [(0, 13, 13, 0), (13, 22, 14, 5)]
    _interpolate_evaluate(backend, oracle, 22, KINDS)


@pytest.mark.parametrize("kind", [0, "pm1"])
def test_two_strided_passes(backend, oracle, kind):
    from cairo_m_amd.lib import fft_plan
    assert fft_plan(23) == [(0, 12, 12, 0), (12, 18, 14, 8), (18, 23, 11, 6)]
    _interpolate_evaluate(backend, oracle, 23, (kind,))


@pytest.mark.parametrize("n_in,n_out", EVALUATE_PADDED)
def test_zero_padded(backend, oracle, n_in, n_out):
    assert sorted(EVALUATE_PADDED) == [(10, 12), (12, 14), (16, 19), (18, 20)]
    tw = backend.twiddles(n_out)
    hs = [backend.upload(c) for c in columns(3, n_in)]
    outs = [backend.upload(np.full(1 << n_out, 0x5A5A5A5A, dtype=np.uint32)) for _ in hs]
    backend.evaluate(hs, n_in, n_out, tw, outs)
    for o, kind in zip(outs, KINDS):
        assert np.array_equal(backend.download(o, 1 << n_out), ref_evaluate(oracle, kind, n_in, n_out)), (n_in, n_out, kind)
    for h in hs + outs:
        backend.col_free(h)
    backend.twiddles_free(tw)
