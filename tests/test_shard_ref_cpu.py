"""The references of tests/shard_ref.py, checked on the CPU against a second statement of the same thing, before the GPU tests
lean on them: the k_quotient_coeffs reference against fe.quotient_coefs and a term-by-term sum, the halo reference against the
exhaustive neighbour claim of test_previous_row_halo_neighbours, the numpy sums against Python integers."""
import numpy as np
import pytest

from tests import field_edges as fe
from tests import shard_ref as sr
from tests.field_edges import P


@pytest.mark.parametrize("coeff", [(1, 0, 0, 0), (0, 0, 1, 0), (P - 1,) * 4, (1711792828, 3870524, 83707791, 1705168718)])
@pytest.mark.parametrize("n", [1, 7, 300])
def test_quotient_coeffs_reference(coeff, n):
    """coef_c equals fe.quotient_coefs (a running product, where the reference takes every power on its own); the sums equal a
    term-by-term sum of Python integers built from the definitions a = conj(v) - v, b = v c - a Py with the running power; a real
    sample value has a = 0 and b = v c, so sum_b = v * sum(coef_c) when every value is the same real."""
    rng = np.random.default_rng(11 + n)
    py = (int(rng.integers(0, P)), int(rng.integers(0, P)), 2**30, 2**30)
    values = [tuple(int(w) for w in rng.integers(0, P, size=4)) for _ in range(n)]
    values[0] = (P - 1,) * 4
    coef_c, sum_a, sum_b, bc = sr.quotient_coeffs(coeff, py, values)
    assert coef_c == fe.quotient_coefs(coeff, py, n)
    c = fe.q_sub(fe.q_conj_u(py), py)
    assert c == (0, 0, P - 1, P - 1)
    alpha, want_a, want_b = (1, 0, 0, 0), [0] * 4, [0] * 4
    for v in values:
        alpha = fe.q_mul(alpha, coeff)
        a = (0, 0, (-2 * v[2]) % P, (-2 * v[3]) % P)          # conj(v) - v, word by word
        b = fe.q_sub(fe.q_mul(v, c), fe.q_mul(a, py))
        ta, tb = fe.q_mul(alpha, a), fe.q_mul(alpha, b)
        for j in range(4):
            want_a[j] += ta[j]
            want_b[j] += tb[j]
    assert sum_a == tuple(x % P for x in want_a) and sum_b == tuple(x % P for x in want_b)
    assert bc == alpha == fe.q_pow(coeff, n)
    real = [(12345, 0, 0, 0)] * n
    coef_r, sa_r, sb_r, _ = sr.quotient_coeffs(coeff, py, real)
    total = (0, 0, 0, 0)
    for cc in coef_r:
        total = fe.q_add(total, cc)
    assert sa_r == (0, 0, 0, 0) and sb_r == fe.q_scale(total, 12345)


def test_halo_reference_reads_only_the_two_neighbours_halves():
    """halo_reference (the column at the model's previous row) from the packed halves alone: for every rank of 2 / 4 / 8 at three
    sizes, out[q] is found in the half of parity q & 1 of halo_sources' rank at index qp >> 1 — the claim
    test_previous_row_halo_neighbours makes about owners and parities, here on values.  The previous row is a bijection."""
    for n in (6, 9, 11):
        column = np.arange(1 << n, dtype=np.uint32) * np.uint32(2654435761)
        assert sorted(sr.shifted_row(r, n, n - 1, -1) for r in range(1 << n)) == list(range(1 << n))
        for log_ranks in (1, 2, 3):
            length = 1 << (n - log_ranks)
            halves = {(r, par): sr.pack_parity(column[r * length:(r + 1) * length], length // 2, par)
                      for r in range(1 << log_ranks) for par in (0, 1)}
            for rank in range(1 << log_ranks):
                src_even, src_odd = sr.halo_sources(rank, log_ranks)
                want = sr.halo_reference(column, rank * length, length, n, n - 1)
                for q in range(length):
                    pr = sr.shifted_row(rank * length + q, n, n - 1, -1)
                    qp = pr & (length - 1)
                    assert pr >> (n - log_ranks) == (src_odd if q & 1 else src_even) and (qp & 1) == (q & 1)
                    assert halves[(src_odd if q & 1 else src_even, q & 1)][qp >> 1] == want[q], (n, log_ranks, rank, q)


def test_pack_parity_reference():
    src = np.arange(10, 30, dtype=np.uint32)
    assert sr.pack_parity(src, 5, 0).tolist() == [10, 12, 14, 16, 18] and sr.pack_parity(src, 5, 1).tolist() == [11, 13, 15, 17, 19]
    assert sr.pack_parity(src, 1, 1).tolist() == [11]


@pytest.mark.parametrize("n_copies,stride,words", [(1, 5, 5), (2, 9, 7), (8, 11, 11)])
def test_sum_copies_reference(n_copies, stride, words):
    rng = np.random.default_rng(5)
    for modular in (True, False):
        hi = P if modular else 2**32
        buf = rng.integers(hi - 9, hi, size=n_copies * stride, dtype=np.uint64).astype(np.uint32)
        want = []
        for i in range(words):
            t = sum(int(buf[k * stride + i]) for k in range(n_copies))
            want.append(t % P if modular else t % 2**32)
        assert sr.sum_copies(buf, n_copies, stride, words, modular).tolist() == want
    assert sr.sum_copies(np.full(2, P - 1, dtype=np.uint32), 2, 1, 1, True).tolist() == [P - 2]
    assert sr.sum_copies(np.array([1, P - 1], dtype=np.uint32), 2, 1, 1, True).tolist() == [0]
    assert sr.sum_copies(np.array([2**32 - 1, 2], dtype=np.uint32), 2, 1, 1, False).tolist() == [1]
