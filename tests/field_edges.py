"""Worst-case words for the lazily folded field arithmetic (field.hpp, gpu_air.hpp, kernels_fri.hip, kernels_poly.hip), the
column generators built from them, and a Python big-integer restatement of the M31 / CM31 / QM31 tower (`%` on Python ints and
nothing else) that pins both the HIP kernels and the C++ oracle.  A helper: no test functions.

The unit-count bounds of the folded forms (`4 (2^31-1)^2 + 3 * 2^32 < 2^64`, negatives carried as `P - x` in [1, P], doubled
operands < 2^32 counted as two units) are tight only at the words below: 0 (whose negative is carried as P), P-1 in every slot,
and 2^30 / 2^30-1 (the doubled operands 2^31 and 2^31-2).  A uniform 31-bit word essentially never produces them."""
import itertools

import numpy as np

P = 2**31 - 1
EDGE = [0, 1, 2, P - 2, P - 1, 2**30 - 1, 2**30, 2**30 + 1, 2**16 - 1, 2**16, 0x55555555, 0x2AAAAAAA]
E6 = [0, 1, P - 2, P - 1, 2**30 - 1, 2**30]
RELATION_WORDS = 8 * 4 + 8 * 16 * 4   # cm_relations: z[8][4] then alpha_pow[8][16][4]


# ---- columns -------------------------------------------------------------------------------------------------------------
def const(v, n):
    return np.full(n, v, dtype=np.uint32)


def edge_mix(rng, n):
    return np.asarray(EDGE, dtype=np.uint32)[rng.integers(0, len(EDGE), size=n)]


def near_p(rng, n):
    return rng.integers(P - 8, P, size=n, dtype=np.uint32)


def alt(n):
    a = np.zeros(n, dtype=np.uint32)
    a[1::2] = P - 1
    return a


def e6_tuples(with_zero=False):
    """E6^4 in lexicographic order, (0,0,0,0) left out unless asked for: 1295 (odd) elements."""
    return [t for t in itertools.product(E6, repeat=4) if with_zero or any(t)]


# ---- Python-int reference ------------------------------------------------------------------------------------------------
def m_mul(a, b):
    return (a * b) % P


def m_pow(a, e):
    r = 1
    while e:
        if e & 1:
            r = (r * a) % P
        a = (a * a) % P
        e >>= 1
    return r


def m_inv(a):
    assert a % P != 0, "M31 inverse of zero"
    return m_pow(a % P, P - 2)


def c_mul(x, y):
    return ((x[0] * y[0] - x[1] * y[1]) % P, (x[0] * y[1] + x[1] * y[0]) % P)


def c_norm(x):
    return (x[0] * x[0] + x[1] * x[1]) % P


def c_inv(x):
    n = m_inv(c_norm(x))
    return ((x[0] * n) % P, (-x[1] * n) % P)


def q_add(x, y):
    return tuple((a + b) % P for a, b in zip(x, y))


def q_sub(x, y):
    return tuple((a - b) % P for a, b in zip(x, y))


def q_neg(x):
    return tuple((-a) % P for a in x)


def q_mul(x, y):
    """(a + b u)(c + d u) with u^2 = 2 + i; a QM31 is its four words (a.re, a.im, b.re, b.im)."""
    a, b, c, d = x[:2], x[2:], y[:2], y[2:]
    ac, bd, ad, bc = c_mul(a, c), c_mul(b, d), c_mul(a, d), c_mul(b, c)
    rbd = c_mul((2, 1), bd)
    return ((ac[0] + rbd[0]) % P, (ac[1] + rbd[1]) % P, (ad[0] + bc[0]) % P, (ad[1] + bc[1]) % P)


def q_norm(x):
    """a^2 - (2 + i) b^2 in CM31: zero only for x = 0."""
    a2, b2 = c_mul(x[:2], x[:2]), c_mul((2, 1), c_mul(x[2:], x[2:]))
    return ((a2[0] - b2[0]) % P, (a2[1] - b2[1]) % P)


def q_invertible(x):
    return c_norm(q_norm(x)) != 0


def q_inv(x):
    di = c_inv(q_norm(x))
    a, b = c_mul(x[:2], di), c_mul(x[2:], di)
    return (a[0], a[1], (-b[0]) % P, (-b[1]) % P)


def q_pow(x, e):
    r = (1, 0, 0, 0)
    while e:
        if e & 1:
            r = q_mul(r, x)
        x = q_mul(x, x)
        e >>= 1
    return r


def q_conj_u(x):
    return (x[0], x[1], (-x[2]) % P, (-x[3]) % P)


def q_scale(c4, x):
    return tuple((int(c) * int(x)) % P for c in c4)


def dot(c4_list, x_list):
    """sum_k c_k * x_k in QM31 (c_k four words, x_k an M31 word)."""
    acc = [0, 0, 0, 0]
    for c4, x in zip(c4_list, x_list):
        for j in range(4):
            acc[j] += int(c4[j]) * int(x)
    return tuple(a % P for a in acc)


def quotient_coefs(random_coeff, point_y, n):
    """The per-entry coefficients of a sample batch of n entries: coeff^(k+1) * (conj_u(y) - y), k = 0 .. n-1."""
    rc, y = tuple(int(w) for w in random_coeff), tuple(int(w) for w in point_y)
    cdiff = q_sub(q_conj_u(y), y)
    out, alpha = [], (1, 0, 0, 0)
    for _ in range(n):
        alpha = q_mul(alpha, rc)
        out.append(q_mul(alpha, cdiff))
    return out


# ---- relation words ------------------------------------------------------------------------------------------------------
def rel_z_only(z4):
    """Every alpha power 0, every relation's z = z4: dev_combine gives 0 - z, so every LogUp denominator is exactly -z4."""
    r = np.zeros(RELATION_WORDS, dtype=np.uint32)
    r[:32] = np.tile(np.asarray(z4, dtype=np.uint32), 8)
    return r


def rel_all(v, z_last=None):
    """Every word is v.  The denominators are then v (1 + i + u + iu) (sum_i v_i - 1): zero for EVERY v as soon as the values of one
    relation entry sum to 1, which fibonacci(37) has (the oracle's assert says so).  z_last replaces the fourth word of every z,
    after which no denominator can vanish (its words 0 and 3 differ) while every alpha power — all that the products of
    dev_combine see — is still v."""
    r = np.full(RELATION_WORDS, v, dtype=np.uint32)
    if z_last is not None:
        r[3:32:4] = z_last
    return r


def rel_edge_mix(rng):
    return edge_mix(rng, RELATION_WORDS)


# ---- the steered relation settings of the LogUp / constraint tests ------------------------------------------------------------
# (name, relation words).  tests/test_field_edges_cpu.py runs every one of them through the oracle alone first: a setting that
# makes a LogUp denominator zero ends the process there, on the CPU, and is replaced — change the constants, not the rule.
def relation_settings():
    zs = [(1, P - 1, 0, P - 1),   # the norm's P - b0 is P while b1d = 2P - 2
          (P - 1,) * 4, (0, 0, 0, 1), (0, 0, P - 1, 0), (1, 0, 0, 0), (2**30,) * 4]
    out = [("z_only_%d" % i, rel_z_only(z)) for i, z in enumerate(zs)]
    # rel_all(P - 1) as it stands divides by zero in the oracle (see rel_all): replaced by the same words with z = (P-1, P-1, P-1, P-2)
    out.append(("all_pm1", rel_all(P - 1, z_last=P - 2)))
    out.append(("edge_mix", rel_edge_mix(np.random.default_rng(4242))))
    return out


def ret_row0_reference(z4, enabler):
    """Row 0 of Ret under rel_z_only(z4), from the Python reference: every denominator is -z4, so the first batch is
    m0 / (-z) + m1 / (-z) with m0 = -enabler, m1 = enabler (the two register entries), and the fifth — the first two range checks,
    m = P-1 each, on top of four batches that cancel — is 2 (P-1) / (-z)."""
    di = q_inv(q_neg(z4))
    b0 = q_add(q_scale(di, (P - enabler) % P), q_scale(di, enabler))
    b4 = q_add(q_scale(di, P - 1), q_scale(di, P - 1))
    return b0, b4


def constraint_coeffs(kind, n_cons, cid):
    """The constraint powers of one component: all P-1, or drawn from EDGE (seeded by the component)."""
    if kind == "pm1":
        return const(P - 1, 4 * n_cons)
    return edge_mix(np.random.default_rng(9000 + cid), 4 * n_cons)
