"""The CPU oracle's field tower (oracle/ofield.hpp, 64-bit `%`) against the Python big-integer restatement of
tests/field_edges.py over the full cross products of the worst-case words, and the steered relation settings of
tests/test_gpu_field_edges.py through the oracle alone: a setting that makes a LogUp denominator zero trips the oracle's
assert (which ends the process) here, on the CPU, and not next to a GPU."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import N_COMPONENTS, load_library, synth_fibonacci
from tests import field_edges as fe
from tests.field_edges import E6, EDGE, P

C_RET = 4


def _words(tuples):
    return np.array(tuples, dtype=np.uint32).reshape(-1)


def test_m31_mul_inv_edges(oracle):
    pairs = [(a, b) for a in EDGE for b in EDGE]
    a, b = np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)
    assert oracle.m31_mul(a, b).tolist() == [fe.m_mul(x, y) for x, y in pairs]
    nz = [x for x in EDGE if x]
    inv = oracle.m31_inv(np.array(nz, dtype=np.uint32)).tolist()
    assert inv == [fe.m_inv(x) for x in nz]
    assert all(fe.m_mul(x, y) == 1 for x, y in zip(nz, inv))


# sixteen right operands from E6^4: the five the lazy QM31 product's unit counts are tight at, and eleven mixed ones
QM31_RIGHT = [(P - 1,) * 4, (0, P - 1, 0, P - 1), (P - 1, 0, P - 1, 0), (2**30,) * 4, (1, 0, 0, 0),
              (0, 0, 0, 0), (0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (2**30 - 1,) * 4, (P - 2,) * 4,
              (P - 1, P - 1, 2**30, 2**30), (2**30, 2**30, P - 1, P - 1), (0, 0, P - 1, P - 1), (P - 1, 2**30 - 1, P - 2, 2**30),
              (1, P - 1, 0, P - 1)]


def test_qm31_mul_edges(oracle):
    assert len(QM31_RIGHT) == 16 and len(set(QM31_RIGHT)) == 16 and all(w in E6 for t in QM31_RIGHT for w in t)
    left = fe.e6_tuples(with_zero=True)
    assert len(left) == 6**4
    for y in QM31_RIGHT:
        got = oracle.qm31_mul(_words(left), _words([y] * len(left))).reshape(-1, 4)
        want = [fe.q_mul(x, y) for x in left]
        assert got.tolist() == [list(w) for w in want], y


def test_qm31_inv_edges(oracle):
    xs = fe.e6_tuples()
    assert len(xs) == 1295
    # a field's only non-invertible element is 0: the GPU test's exclusion list is exactly {(0, 0, 0, 0)}
    assert all(fe.q_invertible(x) for x in xs) and not fe.q_invertible((0, 0, 0, 0))
    got = oracle.qm31_inv(_words(xs)).reshape(-1, 4)
    want = [fe.q_inv(x) for x in xs]
    assert got.tolist() == [list(w) for w in want]
    assert all(fe.q_mul(x, w) == (1, 0, 0, 0) for x, w in zip(xs, want))


def component_shapes(L, oracle, view):
    """(log, interaction columns, constraints) per component, from the host-side ABI and the oracle's traces."""
    out = []
    for cid in range(N_COMPONENTS):
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        assert L.cm_component_info(C.c_int32(cid), C.byref(a), C.byref(b), C.byref(c)) == 0
        log = int(np.log2(oracle.component_trace(view, cid).shape[1]))
        out.append((log, b.value, c.value))
    return out


@pytest.fixture(scope="module")
def fib37(oracle):
    inp = synth_fibonacci(37)
    yield inp, component_shapes(load_library(), oracle, inp.view)
    inp.free()


@pytest.mark.parametrize("name,rel", fe.relation_settings(), ids=[s[0] for s in fe.relation_settings()])
def test_steered_relations_through_the_oracle_alone(oracle, fib37, name, rel):
    """Same inputs, seeds and components as test_gpu_field_edges.test_logup_and_constraints_under_steered_relations: no
    denominator of a kept setting is zero (orc::M31::inverse asserts), and the claimed sums are field elements."""
    inp, shapes = fib37
    for cid, (log, n_it, n_cons) in enumerate(shapes):
        cols, cs = oracle.component_interaction(inp.view, cid, rel, n_it, log)
        assert cols.shape == (n_it, 1 << log) and int(cols.max(initial=0)) < P and int(cs.max()) < P
        if cid == C_RET and name.startswith("z_only"):   # the Python reference pins the oracle's first and fifth batch of row 0
            b0, b4 = fe.ret_row0_reference(tuple(int(w) for w in rel[:4]), int(oracle.component_trace(inp.view, cid)[0][0]))
            assert tuple(int(w) for w in cols[0:4, 0]) == b0 and tuple(int(w) for w in cols[16:20, 0]) == b4
        if log <= 12:
            for kind in ("pm1", "edge"):
                acc = oracle.component_constraints(inp.view, cid, rel, fe.constraint_coeffs(kind, n_cons, cid), log)
                assert acc.shape == (4, 2 << log) and int(acc.max()) < P


def test_every_kind_of_setting_survives():
    names = [s[0] for s in fe.relation_settings()]
    assert any(n.startswith("z_only") for n in names) and "all_pm1" in names and "edge_mix" in names
