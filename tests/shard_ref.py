"""References for the op-level tests of the row-range / prover-only FRI and quotient kernels and of the sharded prover's data
movement (tests/test_gpu_fri_rows.py, tests/test_gpu_shard_ops.py), each independent of the code under test.  A helper: no test
functions.

Folds, quotients and leaf hashes need nothing here: the reference for a row range is the matching slice of the oracle's
whole-domain result (`rows` / `src_rows` below only cut the slices).  k_quotient_coeffs: Python integers through
tests/field_edges.py.  The halo: the bit-reversal / previous-row model of cm::shifted_row (device_common.hpp), first written for
test_previous_row_halo_neighbours.  sum_copies / copy_segments: numpy with uint64 sums mod P and uint32 wrap-around."""
import functools

import numpy as np

from tests import field_edges as fe
from tests.field_edges import P


# ---- row ranges ----------------------------------------------------------------------------------------------------------
def rows(cols, r0, n):
    """Rows [r0, r0 + n) of every column."""
    return [np.ascontiguousarray(c[r0:r0 + n]) for c in cols]


def src_rows(cols, i0, n_out):
    """The source rows of fold outputs [i0, i0 + n_out): folds are pair-local."""
    return rows(cols, 2 * i0, 2 * n_out)


# ---- k_quotient_coeffs ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _power(rc, e):
    return fe.q_pow(rc, e)


def quotient_coeffs(coeff, point_y, values):
    """One batch: values = the sampled value of every entry in entry order.  Entry k gets alpha = coeff^(k+1); with v its value
    and Py the point's y: a = conj(v) - v, c = conj(Py) - Py, b = v c - a Py.  Returns (coef_c per entry = alpha c, sum_a = sum
    alpha a, sum_b = sum alpha b, batch_coeff = coeff^n), every power taken on its own by square and multiply."""
    rc, py = tuple(int(w) for w in coeff), tuple(int(w) for w in point_y)
    c = fe.q_sub(fe.q_conj_u(py), py)
    coef_c, sum_a, sum_b = [], (0, 0, 0, 0), (0, 0, 0, 0)
    for k, v in enumerate(values):
        v = tuple(int(w) for w in v)
        alpha = _power(rc, k + 1)
        a = fe.q_sub(fe.q_conj_u(v), v)
        b = fe.q_sub(fe.q_mul(v, c), fe.q_mul(a, py))
        coef_c.append(fe.q_mul(alpha, c))
        sum_a = fe.q_add(sum_a, fe.q_mul(alpha, a))
        sum_b = fe.q_add(sum_b, fe.q_mul(alpha, b))
    return coef_c, sum_a, sum_b, _power(rc, len(values))


# ---- the previous-row halo -----------------------------------------------------------------------------------------------
def brev(i, log):
    r = 0
    for b in range(log):
        r |= ((i >> b) & 1) << (log - 1 - b)
    return r


def shifted_row(r, n, trace_log, offset):
    """Model of cm::shifted_row: the storage row `offset` trace steps away from storage row r on bit-reversed storage of log n."""
    i = brev(r, n)
    half = 1 << (n - 1)
    mask = (1 << (n + 1)) - 1
    e = (1 + 4 * i) if i < half else (-(1 + 4 * (i - half))) & 0xffffffff
    e = (e + offset * (1 << (n + 1 - trace_log))) & mask
    j = (e - 1) // 4 if (e & 3) == 1 else half + (((mask + 1) - e - 1) & mask) // 4
    return brev(j, n)


def halo_sources(rank, log_ranks):
    """(rank whose even half, rank whose odd half) rank `rank` reads: bitrev(bitrev(R) - 1), bitrev(bitrev(R) + 1)."""
    n_ranks, rho = 1 << log_ranks, brev(rank, log_ranks)
    return brev((rho - 1) % n_ranks, log_ranks), brev((rho + 1) % n_ranks, log_ranks)


def halo_reference(column, row0, length, n, trace_log):
    """out[q] = column[shifted_row(row0 + q, n, trace_log, -1)]"""
    return np.array([column[shifted_row(row0 + q, n, trace_log, -1)] for q in range(length)], dtype=np.uint32)


def pack_parity(src, half_len, parity):
    return np.ascontiguousarray(src[parity:2 * half_len:2])


# ---- element-wise reductions and copies ----------------------------------------------------------------------------------
def sum_copies(buf, n_copies, stride, words, modular):
    """out[i] = sum_k buf[k * stride + i]: mod P (uint64 sums: n_copies * (P-1) stays far below 2^64) or wrapping at 2^32."""
    acc = np.zeros(words, dtype=np.uint64)
    for k in range(n_copies):
        acc += buf[k * stride:k * stride + words].astype(np.uint64)
    return (acc % np.uint64(P)).astype(np.uint32) if modular else (acc & np.uint64(0xFFFFFFFF)).astype(np.uint32)
