"""tests/eval_points_ref.py against the CPU oracle and against Python integers, and the steered felts and shifts of
tests/test_gpu_eval_points.py checked before a GPU sees them.  CPU only."""
import numpy as np
import pytest

from tests import eval_points_ref as ref
from tests import field_edges as fe
from tests.field_edges import P


def _columns(rng, n):
    return [rng.integers(0, P, size=n, dtype=np.uint32), fe.edge_mix(rng, n), fe.const(P - 1, n), fe.near_p(rng, n), fe.alt(n)]


def _points(rng):
    return [rng.integers(0, P, size=8, dtype=np.uint32), fe.edge_mix(rng, 8)]


@pytest.mark.parametrize("log_n", [1, 3, 10, 13])
def test_eval_fold_equals_the_oracle(oracle, log_n):
    rng = np.random.default_rng(8100 + log_n)
    for pt in _points(rng):
        for c in _columns(rng, 1 << log_n):
            assert np.array_equal(ref.eval_fold(c, pt[:4], pt[4:]), oracle.eval_at_point(c, pt)), (log_n, pt)


@pytest.mark.parametrize("log_n", range(7))
def test_eval_fold_equals_the_sum_over_index_bits(log_n):
    """sum_i c_i * prod_{bits k of i} m_k, term by term on Python integers; log_n = 0 is coeffs[0]."""
    rng = np.random.default_rng(8200 + log_n)
    n = 1 << log_n
    for pt in _points(rng):
        x, y = tuple(int(w) for w in pt[:4]), tuple(int(w) for w in pt[4:])
        maps = [y, x]
        for _ in range(2, log_n):
            s = fe.q_mul(maps[-1], maps[-1])
            maps.append(fe.q_sub(fe.q_add(s, s), (1, 0, 0, 0)))
        for c in _columns(rng, n):
            acc = (0, 0, 0, 0)
            for i in range(n):
                term = (int(c[i]), 0, 0, 0)
                for k in range(log_n):
                    if i >> k & 1:
                        term = fe.q_mul(term, maps[k])
                acc = fe.q_add(acc, term)
            assert tuple(int(w) for w in ref.eval_fold(c, x, y)) == acc
            if log_n == 0:
                assert acc == (int(c[0]), 0, 0, 0)


def _on_circle(p):
    return fe.q_add(fe.q_mul(p[0], p[0]), fe.q_mul(p[1], p[1])) == (1, 0, 0, 0)


def test_every_gpu_felt_has_a_point_on_the_circle():
    felts = dict(ref.gpu_felts())
    assert len(felts) == 5 and len(set(felts.values())) == 5
    assert ref.oods_point(felts["zero"]) == ((1, 0, 0, 0), (0, 0, 0, 0))
    assert felts["all_pm1"] == (P - 1,) * 4 and felts["one"] == (1, 0, 0, 0)
    assert all(w in fe.EDGE for w in felts["edge_mix"])
    for name, t in felts.items():
        assert fe.q_invertible(fe.q_add((1, 0, 0, 0), fe.q_mul(t, t))), name
        for log_n in ref.GPU_POINT_LOGS:
            pts = [ref.oods_point(t, s) for _, s in ref.gpu_shifts(log_n)]
            assert all(_on_circle(p) for p in pts), (name, log_n)
            assert len(set(pts)) == len(pts), (name, log_n)          # different shifts, different points


def test_a_shifted_point_is_the_circle_sum_of_the_point_and_the_shift():
    for name, t in ref.gpu_felts():
        base = ref.oods_point(t)
        for log_n in ref.GPU_POINT_LOGS:
            for sname, s in ref.gpu_shifts(log_n):
                if s is None:
                    continue
                assert (s[0] * s[0] + s[1] * s[1]) % P == 1, sname       # an M31 circle point
                assert ref.oods_point(t, s) == ref.cadd(base, ((s[0], 0, 0, 0), (s[1], 0, 0, 0))), (name, log_n, sname)


@pytest.mark.parametrize("log_n", [1, 4, 11, 26])
def test_prev_row_shift_is_the_conjugate_of_the_subgroup_generator(oracle, log_n):
    """The generator of the subgroup of 2^log_n points is the first point of the canonic domain one size below (for log_n >= 2),
    has order exactly 2^log_n, and the shift is its conjugate."""
    g = ref.circle_gen_pow(1 << (31 - log_n))
    assert ref.prev_row_shift(log_n) == (g[0], (-g[1]) % P)
    if log_n >= 2:
        assert oracle.domain_point(log_n - 1, 0) == g
    p = g
    for _ in range(log_n - 1):
        p = ((p[0] * p[0] - p[1] * p[1]) % P, (2 * p[0] * p[1]) % P)
    assert p == (P - 1, 0)                                              # order 2 after log_n - 1 doublings
