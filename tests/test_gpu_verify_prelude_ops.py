"""The prelude kernels one at a time, on steered words (cm_public_logup_sum_op, cm_point_eval_op).

Public sum: k_verify_public_sum + k_verify_prelude_fin against the pure-Python restatement of PublicData::initial_logup_sum
(tests/verify_prelude_ref.py), which decides; the host twin must agree.  Shapes: present totals 0, 1, B - 1, B, B + 1, 3B + 1
(B = 256 entries per workgroup), spread over the three lists and with empty lists, the output list alone (sign, final root),
absent entries first and last in a workgroup's chunk, edge words, one vanishing memory denominator, one vanishing Merkle leaf,
and all of them as jobs of ONE call.

Point evaluation: k_verify_oods against cm_point_eval_host word for word, every component, uniform waves (1, 63, 64, 65 jobs of
one component) and divergent ones (34 x 3 jobs interleaved), random and edge words in every slot, a non-zero shift."""
import numpy as np
import pytest

from cairo_m_amd.lib import point_eval_job, public_sum_job
from tests.verify_prelude_ref import N_COMPONENTS, count_zero_denominators, eval_job_words, initial_logup_sum, sum_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """[(case, the reference's sum)] — computed once"""
    return [(c, initial_logup_sum(*c[1:])) for c in sum_cases()]


def test_public_sum_every_shape_alone(backend, cases):
    for (name, head, program, inp, output, rel), want in cases:
        job = public_sum_job(head, program, inp, output, rel)
        got = backend.public_logup_sum([job])
        print(name, got[0])
        assert got == [want], name
        assert backend.public_logup_sum_host(job) == want, name


def test_public_sum_all_shapes_as_jobs_of_one_call(backend, cases):
    jobs = [public_sum_job(*c[1:]) for c, _ in cases]
    assert len({j[0].n_program + j[0].n_input + j[0].n_output for j in jobs}) > 6       # jobs of different sizes
    assert backend.public_logup_sum(jobs) == [want for _, want in cases]
    # the other order: a job's chunks do not depend on where it sits
    assert backend.public_logup_sum(jobs[::-1]) == [want for _, want in cases][::-1]


def test_public_sum_steered_zero_denominators(backend, cases):
    for (name, head, program, inp, output, rel), want in cases:
        if not name.startswith("zero "):
            continue
        got = backend.public_logup_sum([public_sum_job(head, program, inp, output, rel)])[0]
        assert count_zero_denominators((name, head, program, inp, output, rel)) == 1
        assert got == want and any(got), name


def _eval_jobs(L, plan, seed, edge):
    rng = np.random.default_rng(seed)
    return [point_eval_job(cid, *eval_job_words(L, cid, rng, edge)) for cid in plan]


def _check(backend, jobs):
    got = backend.point_eval(jobs)
    want = [backend.point_eval_host(j) for j in jobs]
    assert len(got) == len(jobs)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, jobs[k][0].component, g, w)
    return got


@pytest.mark.parametrize("edge", [False, True], ids=["random", "edge"])
def test_point_eval_every_component(backend, edge):
    jobs = _eval_jobs(backend.L, list(range(N_COMPONENTS)), 11 + edge, edge)
    assert all(any(j[0].shift) for j in jobs)
    got = _check(backend, jobs)
    assert len(set(got)) > N_COMPONENTS // 2


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_point_eval_uniform_waves(backend, n):
    """n jobs of ONE component: full and partial waves that hold a single arm of the switch"""
    for cid in (0, 14, 29):      # a small opcode, the widest u32 opcode (U32StoreDivFpImm), Poseidon2
        _check(backend, _eval_jobs(backend.L, [cid] * n, 100 * cid + n, edge=(n == 64)))


def test_point_eval_divergent_waves(backend):
    """34 x 3 jobs interleaved by component: every wave holds many arms of the switch"""
    plan = [cid for _ in range(3) for cid in range(N_COMPONENTS)]
    jobs = _eval_jobs(backend.L, plan, 5, False)
    edge_jobs = _eval_jobs(backend.L, plan, 6, True)
    mixed = [a if k % 2 else b for k, (a, b) in enumerate(zip(jobs, edge_jobs))]
    _check(backend, mixed)
