"""A plain reference for the provers' out-of-domain sampling (eval_at_point_multi in kernels_poly.hip): the evaluation of a
coefficient column at a QM31 circle point as the fold the reference prover performs, and the point a drawn felt stands for.
A helper: no test functions.

eval_fold works from the top index bit down on whole arrays — numpy uint64 words mod P = 2^31 - 1, every product of two
canonical words is below 2^62 and is reduced before anything is added to it, so the arithmetic is exact.  It shares nothing
with the kernels' decomposition into a low table, a high table and groups of chunks.  The scalars (the per-bit factors, the
point of a felt) are Python integers through the q_* helpers of tests/field_edges.py."""
import numpy as np

from tests.field_edges import P, edge_mix, q_add, q_inv, q_invertible, q_mul, q_scale, q_sub

ONE = (1, 0, 0, 0)
_P = np.uint64(P)
CIRCLE_GEN = (2, 1268011823)     # the generator of the M31 circle group (order 2^31)


def _cm(x0, x1, y0, y1):
    """(x0 + x1 i)(y0 + y1 i): arrays times scalars, every term reduced before it is combined."""
    return ((x0 * y0) % _P + _P - (x1 * y1) % _P) % _P, ((x0 * y1) % _P + (x1 * y0) % _P) % _P


def _qmul_scalar(v, m):
    """v[:, 4] (QM31 per row) times the QM31 scalar m: (a + b u)(c + d u) = ac + (2 + i) bd + (ad + bc) u."""
    c0, c1, d0, d1 = (np.uint64(w) for w in m)
    a0, a1, b0, b1 = v[:, 0], v[:, 1], v[:, 2], v[:, 3]
    ac0, ac1 = _cm(a0, a1, c0, c1)
    bd0, bd1 = _cm(b0, b1, d0, d1)
    ad0, ad1 = _cm(a0, a1, d0, d1)
    bc0, bc1 = _cm(b0, b1, c0, c1)
    r0, r1 = _cm(bd0, bd1, np.uint64(2), np.uint64(1))
    return np.stack([(ac0 + r0) % _P, (ac1 + r1) % _P, (ad0 + bc0) % _P, (ad1 + bc1) % _P], axis=1)


def fold_maps(x4, y4, log_n):
    """m_0 = y, m_1 = x, m_k = 2 m_{k-1}^2 - 1: the factor of index bit k."""
    x, y = tuple(int(w) for w in x4), tuple(int(w) for w in y4)
    maps = [y, x]
    while len(maps) < log_n:
        s = q_mul(maps[-1], maps[-1])
        maps.append(q_sub(q_add(s, s), ONE))
    return maps[:log_n]


def eval_fold(coeffs, x4, y4):
    """sum_i coeffs[i] * prod_{bits k of i} m_k by folding the top bit away, log_n times: c = c[:half] + c[half:] * m_k.
    Returns the four words of the value (uint32)."""
    c = np.asarray(coeffs, dtype=np.uint64)
    n = c.size
    log_n = n.bit_length() - 1
    assert n == 1 << log_n and (c < _P).all()
    maps = fold_maps(x4, y4, log_n)
    v = np.zeros((n, 4), dtype=np.uint64)
    v[:, 0] = c
    for k in range(log_n - 1, -1, -1):
        half = v.shape[0] // 2
        v = (v[:half] + _qmul_scalar(v[half:], maps[k])) % _P
    return v[0].astype(np.uint32)


def cadd(p, q):
    """The circle group's addition on points with QM31 coordinates: (px qx - py qy, px qy + py qx)."""
    return q_sub(q_mul(p[0], q[0]), q_mul(p[1], q[1])), q_add(q_mul(p[0], q[1]), q_mul(p[1], q[0]))


def oods_point(t4, shift=None):
    """The point of a drawn felt, ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)), plus the M31 point `shift` = (x, y) when there is one
    (q_scale multiplies a QM31 by an M31 word: the formula of cadd restated for that case).  1 + t^2 = 0 has no point."""
    t = tuple(int(w) for w in t4)
    t2 = q_mul(t, t)
    d = q_add(ONE, t2)
    assert q_invertible(d), "1 + t^2 = 0: the felt has no point"
    iv = q_inv(d)
    x, y = q_mul(q_sub(ONE, t2), iv), q_mul(q_add(t, t), iv)
    if shift is not None:
        sx, sy = int(shift[0]), int(shift[1])
        x, y = q_sub(q_scale(x, sx), q_scale(y, sy)), q_add(q_scale(x, sy), q_scale(y, sx))
    return x, y


def circle_gen_pow(idx):
    """CIRCLE_GEN^idx in the M31 circle group, by double-and-add on Python integers."""
    def add(p, q):
        return (p[0] * q[0] - p[1] * q[1]) % P, (p[0] * q[1] + p[1] * q[0]) % P
    res, cur = (1, 0), CIRCLE_GEN
    while idx:
        if idx & 1:
            res = add(res, cur)
        cur = add(cur, cur)
        idx >>= 1
    return res


def prev_row_shift(log_n):
    """The shift of the prover's previous-row mask at a component of 2^log_n rows: (step.x, -step.y) for step = the generator of
    the subgroup of that size."""
    sx, sy = circle_gen_pow(1 << (31 - log_n))
    return sx, (-sy) % P


# ---- the steered inputs of tests/test_gpu_eval_points.py (tests/test_eval_points_cpu.py checks them without a GPU) -----------
def gpu_felts():
    """(name, felt).  No felt with 1 + t^2 = 0 (t = +-i): the inverse of zero is not defined and no transcript reaches it."""
    rng = np.random.default_rng(7301)
    edge = tuple(int(w) for w in edge_mix(np.random.default_rng(7302), 4))
    return [("zero", (0, 0, 0, 0)), ("one", (1, 0, 0, 0)), ("all_pm1", (P - 1,) * 4), ("edge_mix", edge),
            ("random", tuple(int(w) for w in rng.integers(0, P, size=4)))]


GPU_POINT_LOGS = (4, 11)


def gpu_shifts(log_n):
    """(name, shift or None) of the device-point jobs at one size: none, the previous-row mask's, and the two circle points that
    have a coordinate equal to P-1."""
    return [("none", None), ("prev_row", prev_row_shift(log_n)), ("minus_one_x", (P - 1, 0)), ("minus_one_y", (0, P - 1))]
