"""Composed transitions on the GPU (cm_compose_transitions, device == 1) against tests/mem_compose_ref.py: every chain equals the
two set openings of the union under the first and the last tree and the host path's bytes, the GPU verifier folds the result to
both roots, every buffer goes back to the pool, every refusal has the host path's status and message.  Parts built from real
handles (uploaded tree pairs opened with cm_input_open_transition) and the two-segment heap run through run_transition."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemTransition, MemTransitionViewC, Run, compose_transitions, prover_input_arrays, run_transition,
                             verify_transition, verify_transition_host)
from tests.mem_compose_ref import CHAINS, REFUSALS, assert_equals, chain, parts_of, refusals, same_bytes
from tests.mem_open_ref import image_cells
from tests.test_gpu_mem_open import _heap_run
from tests.test_gpu_transition import _upload
from tests.test_mem_compose_cpu import raw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CHAINS)
def test_gpu_composition_equals_the_reference_and_the_host_path(backend, name):
    c = chain(name)
    L = backend.L
    t = compose_transitions(parts_of(name), L, device=True)
    live = backend.mem_stats().live_bytes
    assert_equals(t, c["ref"])
    assert same_bytes(t, compose_transitions(parts_of(name), L, device=False))
    assert same_bytes(t, backend.compose_transitions(parts_of(name)))            # the same call, the same bytes
    assert verify_transition(t, L, with_roots=True) == (True, (c["trees"][0].root, c["trees"][-1].root))
    assert verify_transition_host(t, L) == (0, "")
    assert backend.mem_stats().live_bytes == live                                # every buffer of the calls went back to the pool


def test_one_part_and_empty_parts(backend):
    L = backend.L
    (p,) = parts_of("one")
    assert same_bytes(compose_transitions([p], L), p)
    assert same_bytes(compose_transitions(parts_of("empties"), L), compose_transitions(parts_of("no_empties"), L))
    t = compose_transitions(parts_of("all_empty"), L)
    assert t.addresses.size == 0 and t.siblings.size == 0 and t.root_before == t.root_after
    assert verify_transition(t, L) and verify_transition_host(t, L) == (0, "")
    ps = parts_of("far")
    ps[0].n_zero_only, ps[1].n_zero_only = 2, 5
    assert compose_transitions(ps, L).n_zero_only == 7


@pytest.mark.parametrize("what", REFUSALS)
def test_each_broken_chain_is_refused_as_the_host_path_refuses_it(backend, what):
    """refusals of well-defined input, decided before a word is read"""
    parts, status, needle = refusals()[what]
    L = backend.L
    live = backend.mem_stats().live_bytes
    host, gpu = raw(L, parts, device=0), raw(L, parts, device=1)
    assert gpu == host and gpu[0] == status and needle in gpu[1] and gpu[2] is None, (what, host, gpu)
    with pytest.raises(CmError) as e:
        backend.compose_transitions(parts)
    assert e.value.status == status and needle in e.value.message
    assert backend.mem_stats().live_bytes == live


def test_status_1_refusals_are_the_host_paths(backend):
    L = backend.L
    ps = parts_of("far")

    def short(v):
        v[1].struct_size = C.sizeof(MemTransitionViewC) - 8

    def no_new(v):
        v[0].new_values = None

    for kw in (dict(views=False), dict(out=False), dict(n_parts=0), dict(n_parts=(1 << 16) + 1), dict(edit=short), dict(edit=no_new)):
        host, gpu = raw(L, ps, device=0, **kw), raw(L, ps, device=1, **kw)
        assert gpu == host and gpu[0] == 1, (kw, host, gpu)
    n = (1 << 19) + 1
    zeros = np.zeros((n, 4), dtype=np.uint32)
    big = [MemTransition(np.arange(n, dtype=np.uint32), zeros, zeros, [], 1, 2), MemTransition(np.arange(n - 1, dtype=np.uint32), zeros[:-1], zeros[:-1], [], 2, 3)]
    host, gpu = raw(L, big, device=0), raw(L, big, device=1)
    assert gpu == host and gpu[0] == 1 and "compose in groups" in gpu[1]


def test_composition_is_associative_on_the_gpu(backend):
    ps = parts_of("wide")
    comp = backend.compose_transitions
    flat = comp(ps)
    for cut in range(1, len(ps) - 1):
        p1, p2, p3 = ps[:cut], ps[cut:cut + 1], ps[cut + 1:]
        assert same_bytes(comp([comp(p1 + p2)] + p3), flat)
        assert same_bytes(comp(p1 + [comp(p2 + p3)]), flat)


def test_parts_opened_from_real_handles(backend):
    """three consecutive trees of the wide chain as two uploaded inputs: the opener's own transitions, composed"""
    c = chain("wide")
    trees, parts = c["trees"][:3], c["parts"][:2]
    moves = []
    for i in range(2):
        dev, _ = _upload(backend, trees[i], trees[i + 1])
        moves.append(backend.open_transition(dev, parts[i]["a"]))
        backend.free_input(dev)
        assert_equals(moves[i], parts[i])
    t = backend.compose_transitions(moves)
    u = sorted(set(parts[0]["a"]) | set(parts[1]["a"]))
    from tests.mem_set_ref import ref_set
    words, old, _ = ref_set(trees[0], u)
    words_after, new, _ = ref_set(trees[2], u)
    assert words == words_after
    assert_equals(t, {"a": u, "old": old, "new": new, "words": words, "root0": trees[0].root, "root1": trees[2].root})
    assert verify_transition(t, backend.L, with_roots=True) == (True, (trees[0].root, trees[2].root))


def test_the_transition_of_a_whole_run(backend):
    """the two-segment heap run: one transition from proof 0's initial_root to the last proof's final_root; its updates applied to
    the starting image (as test_a_followed_run_rebuilds_the_final_image builds it) give the run's final image"""
    hss = _heap_run()
    first = Run.from_segment(backend, hss[0])
    dev0 = first.adapt_next(hss[0])
    hi0 = backend.download_input(dev0)
    rows = prover_input_arrays(hi0.view)
    image = {int(r[0]): tuple(int(x) for x in r[1:5]) for r in rows["initial_memory"]}
    backend.free_input(dev0)
    hi0.free()
    first.free()
    run = Run.from_segment(backend, hss[0])
    proofs, moves = run.prove(hss, transitions=True)
    assert len(proofs) == len(moves) == 2 and all(m is not None for m in moves)
    for device in (True, False):
        t = run_transition(proofs, moves, backend.L, device=device)
        assert (t.root_before, t.root_after) == (proofs[0].public_data()["initial_root"], proofs[-1].public_data()["final_root"])
        assert t.addresses.tolist() == sorted(set(moves[0].addresses.tolist()) | set(moves[1].addresses.tolist()))
        assert t.n_zero_only == moves[0].n_zero_only + moves[1].n_zero_only
    for a, v in t.updates():
        image[a] = v
    lo, hp = run.memory()
    final = {c[0]: tuple(c[1:]) for c in image_cells(lo, hp)}
    zero = (0, 0, 0, 0)
    assert all(image.get(a, zero) == final.get(a, zero) for a in set(image) | set(final))
    with pytest.raises(CmError) as e:
        run_transition(proofs, moves[::-1], backend.L)
    assert "part 1 starts at root" in str(e.value), str(e.value)
    bent = MemTransition(moves[1].addresses, moves[1].old_values, moves[1].new_values + np.uint32(1), moves[1].siblings,
                         moves[1].root_before, moves[1].root_after)
    with pytest.raises(CmError) as e:
        run_transition(proofs, [moves[0], bent], backend.L)
    assert "does not verify" in str(e.value), str(e.value)
    for p in proofs:
        p.free()
    run.free()
    for hs in hss:
        hs.free()
