"""The host twins of the prelude ops, without a GPU: cm_public_logup_sum_host (the host verifier's initial_logup_sum) against the
pure-Python restatement of PublicData::initial_logup_sum in tests/verify_prelude_ref.py at every shape the GPU test uses, and
cm_point_eval_host (the host verifier's point_eval): deterministic, and refusing wrong counts for all 34 components."""
import time

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, load_library, point_eval_host, point_eval_job, public_logup_sum_host, public_sum_job
from tests.field_edges import P, q_inv, q_sub
from tests.verify_prelude_ref import (B, N_COMPONENTS, REL_MEMORY, REL_MERKLE, TREE_HEIGHT, combine, count_zero_denominators,
                                      eval_job_words, initial_logup_sum, sum_cases)


@pytest.fixture(scope="module")
def cases():
    return sum_cases()


def test_the_shapes_are_the_ones_promised(cases):
    totals = sorted({int(c[2][:, 0].sum() + c[3][:, 0].sum() + c[4][:, 0].sum()) for c in cases if " present, " in c[0]})
    assert totals == [0, 1, B - 1, B, B + 1, 3 * B + 1]
    names = [c[0] for c in cases]
    assert "%d present, output only" % (3 * B + 1) in names and "%d present, spread" % (B + 1) in names
    by_name = {c[0]: c for c in cases}
    # absent entries sit first and last in a workgroup's chunk
    prog = by_name["%d present, program only" % (B + 1)][2]
    assert prog.shape[0] > B and prog[0, 0] == 0 and prog[B - 1, 0] == 0 and prog[1, 0] == 1
    # the steered cases have exactly one vanishing denominator, every other case none
    for c in cases:
        assert count_zero_denominators(c) == (1 if c[0].startswith("zero ") else 0), c[0]


def test_the_python_reference_is_quick(cases):
    """the largest case (3B + 1 present entries, about 3.8e3 inverses) takes well under a second"""
    big = next(c for c in cases if c[0] == "%d present, spread" % (3 * B + 1))
    t0 = time.perf_counter()
    initial_logup_sum(*big[1:])
    dt = time.perf_counter() - t0
    print("reference, %s: %.3f s" % (big[0], dt))
    assert dt < 1.0


def test_public_logup_sum_host_equals_the_reference(cases):
    L = load_library()
    for name, head, program, inp, output, rel in cases:
        got = public_logup_sum_host(public_sum_job(head, program, inp, output, rel), L)
        assert got == initial_logup_sum(head, program, inp, output, rel), name


def test_a_zero_denominator_contributes_nothing(cases):
    """taking the entry with the vanishing denominator's term out by hand: the sum moves by the other four inverses only"""
    L = load_library()
    c = next(c for c in cases if c[0] == "zero memory denominator")
    _, head, program, inp, output, rel = c
    got = public_logup_sum_host(public_sum_job(head, program, inp, output, rel), L)
    row = [int(w) for w in inp[B + 3]]
    assert not any(combine(rel, REL_MEMORY, (row[1], row[6], row[2], row[3], row[4], row[5])))
    without = inp.copy()
    without[B + 3, 0] = 0
    want = public_logup_sum_host(public_sum_job(head, program, without, output, rel), L)
    for k in range(4):      # the entry's four leaves, consumed under the initial root
        want = q_sub(want, q_inv(combine(rel, REL_MERKLE, ((4 * row[1] + k) % P, TREE_HEIGHT, row[2 + k], int(head[5])))))
    assert got == want


@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
def test_point_eval_host_is_deterministic(edge):
    L = load_library()
    rng = np.random.default_rng(77 + edge)
    seen = set()
    for cid in range(N_COMPONENTS):
        job = point_eval_job(cid, *eval_job_words(L, cid, rng, edge))
        a, b = point_eval_host(job, L), point_eval_host(job, L)
        assert a == b and all(w < 2**31 - 1 for w in a), cid
        seen.add(a)
    assert len(seen) > N_COMPONENTS // 2        # not one constant for every component


def test_point_eval_host_refuses_wrong_counts_for_every_component():
    L = load_library()
    rng = np.random.default_rng(3)
    for cid in range(N_COMPONENTS):
        words = eval_job_words(L, cid, rng, False)
        for field in ("n_tr_words", "n_it_words", "n_coeff_words"):
            for delta in (-4, 4):
                job = point_eval_job(cid, *words)
                setattr(job[0], field, getattr(job[0], field) + delta)
                with pytest.raises(CmError, match=field):
                    point_eval_host(job, L)
        # the next component's counts are wrong for this one wherever the two differ
        other = eval_job_words(L, (cid + 1) % N_COMPONENTS, rng, False)
        if [len(x) for x in other] != [len(x) for x in words]:
            job = point_eval_job(cid, *other)
            with pytest.raises(CmError, match="does not match"):
                point_eval_host(job, L)
