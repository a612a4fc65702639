"""The batched verifiers on the GPU (cm_verify_memory_transitions, cm_verify_memory_sets) against tests/mem_transition_ref.py and
tests/mem_set_ref.py — references in pure Python, never the code under test — and, part for part, against the single-record GPU
calls and the host verifiers.  tests/test_mem_batch_cpu.py shows in numbers which kernel paths the batches used here reach.  The
tamper tests fail on any implementation that leaks a flag, a word offset or a root across a part boundary."""
import functools

import numpy as np
import pytest

from cairo_m_amd.lib import (CmError, MemImage, MemSetOpening, MemTransition, Run, follow_run, follow_run_image, prover_input_arrays, verify_set,
                             verify_set_host, verify_sets, verify_transition, verify_transition_host, verify_transitions)
from tests import mem_set_ref
from tests.mem_batch_cases import BATCHES, small_parts
from tests.mem_set_ref import SETS, ref_set
from tests.mem_transition_ref import first_tree, reference, tampers

pytestmark = pytest.mark.gpu
N = len(SETS)
PLACES = (0, 8, N - 1)                                                            # first, a middle (the widest part) and last
# the keys of mem_transition_ref.tampers and of mem_set_ref.tampers (spelled out so that collecting this file builds no tree;
# test_the_tamper_lists_are_the_references holds them to the references)
TAMPERS = ["an old word + 1", "a new word + 1", "a sibling + 1", "roots swapped", "root after + 1", "an old word = P", "a new word = P",
           "a sibling = P", "one word appended", "one word dropped", "two addresses swapped"]
SET_TAMPERS = ["value of the first cell", "value of a middle cell", "value of the last cell", "the first sibling", "a middle sibling",
               "the last sibling", "one word appended", "one word dropped", "a sibling = P", "a value = P", "two addresses swapped",
               "an address repeated", "an address + 1", "root + 1"]


def transition_of(r):
    return MemTransition(r["a"], r["old"], r["new"], r["words"], r["root0"], r["root1"])


@functools.lru_cache(maxsize=None)
def tampers_of(i):
    return tampers(reference(i))


@functools.lru_cache(maxsize=None)
def set_tampers_of(i):
    r = reference(i)
    return mem_set_ref.tampers(r["a"], r["old"], r["words"], r["root0"])


def tampered(i, name):
    """(the tampered MemTransition of SETS[i], which sides still fold) or None where the record has no such tamper"""
    t = tampers_of(i).get(name)
    return None if t is None else (MemTransition(t[0], t[1], t[2], t[3], t[4], t[5]), t[7])


def test_the_tamper_lists_are_the_references():
    assert set(TAMPERS) == set().union(*(tampers_of(i) for i in PLACES))
    assert set(SET_TAMPERS) == set().union(*(set_tampers_of(i) for i in PLACES))


@functools.lru_cache(maxsize=None)
def valid():
    return [transition_of(reference(i)) for i in range(N)]


def roots_of(i):
    return (reference(i)["root0"], reference(i)["root1"])


def set_of(i):
    """(root, MemSetOpening) of SETS[i] under its first memory: the old plane of the reference transition"""
    r = reference(i)
    return r["root0"], MemSetOpening(r["a"], r["old"], r["words"])


@pytest.mark.parametrize("name", list(BATCHES))
def test_valid_batches_fold_to_the_reference_roots(backend, name):
    order = BATCHES[name]
    got = verify_transitions([valid()[i] for i in order], backend.L, with_roots=True)
    assert got == [(True, roots_of(i)) for i in order]
    sets = [set_of(i) for i in order]
    got = verify_sets([r for r, _ in sets], [o for _, o in sets], backend.L, with_roots=True)
    assert got == [(True, reference(i)["root0"]) for i in order]


@pytest.mark.parametrize("name", TAMPERS)
def test_one_tampered_transition_among_valid_ones(backend, name):
    for place in PLACES:
        bad = tampered(place, name)
        if bad is None:                                                           # (a one-cell record has no two addresses to swap)
            continue
        t, sides = bad
        single = verify_transition(t, backend.L, with_roots=True)
        host, why = verify_transition_host(t, backend.L)
        assert single[0] is False and host == 11
        batch = valid()[:place] + [t] + valid()[place + 1:]
        got = verify_transitions(batch, backend.L, with_roots=True)
        assert got[place] == single, (name, place)
        if "hash to root" not in why:
            assert sides is None and single[1] == (0, 0)                          # malformed: zeros
        else:
            assert 0 not in single[1]                                             # well formed: the roots it does fold to
        for i in range(N):
            if i != place:
                assert got[i] == (True, roots_of(i)), (name, place, i)


def test_every_part_carries_a_different_tamper(backend):
    batch, single, chosen = [], [], []
    for i in range(N):
        names = [n for n in TAMPERS if n in tampers_of(i)]
        chosen.append(names[i % len(names)])
        t, _ = tampered(i, chosen[-1])
        batch.append(t)
        single.append(verify_transition(t, backend.L, with_roots=True))
        assert (verify_transition_host(t, backend.L)[0] == 0) == single[-1][0]
    assert len(set(chosen)) >= 8, chosen
    got = verify_transitions(batch, backend.L, with_roots=True)
    assert got == single and not any(ok for ok, _ in got)
    # and between valid ones, alternating
    mixed = [batch[i] if i % 2 else valid()[i] for i in range(N)]
    assert verify_transitions(mixed, backend.L, with_roots=True) == [single[i] if i % 2 else (True, roots_of(i)) for i in range(N)]


def _set_tampered(i, name):
    t = set_tampers_of(i).get(name)
    return None if t is None else (t[3], MemSetOpening(t[0], t[1], t[2]))


@pytest.mark.parametrize("name", SET_TAMPERS)
def test_one_tampered_set_among_valid_ones(backend, name):
    good = [set_of(i) for i in range(N)]
    for place in PLACES:
        bad = _set_tampered(place, name)
        if bad is None:
            continue
        single = verify_set(bad[0], bad[1], backend.L, with_root=True)
        assert single[0] is False and verify_set_host(bad[0], bad[1], backend.L)[0] == 11
        batch = good[:place] + [bad] + good[place + 1:]
        got = verify_sets([r for r, _ in batch], [o for _, o in batch], backend.L, with_roots=True)
        assert got[place] == single, (name, place)
        for i in range(N):
            if i != place:
                assert got[i] == (True, good[i][0]), (name, place, i)


def test_every_set_carries_a_different_tamper(backend):
    batch = []
    for i in range(N):
        names = [n for n in SET_TAMPERS if _set_tampered(i, n) is not None]
        batch.append(_set_tampered(i, names[(3 * i) % len(names)]))
    single = [verify_set(r, o, backend.L, with_root=True) for r, o in batch]
    assert not any(ok for ok, _ in single)
    assert verify_sets([r for r, _ in batch], [o for _, o in batch], backend.L, with_roots=True) == single


def test_three_hundred_small_parts(backend):
    """a tail-only batch with more parts than a block has lanes, and one with more than the tail's workgroup has"""
    parts = small_parts()
    ts = [transition_of(r) for r in parts]
    want = [(True, (r["root0"], r["root1"])) for r in parts]
    assert verify_transitions(ts, backend.L, with_roots=True) == want
    assert verify_transitions(ts[:130], backend.L, with_roots=True) == want[:130]
    assert verify_sets([r["root1"] for r in parts], [MemSetOpening(r["a"], r["new"], r["words"]) for r in parts], backend.L) == [True] * 300
    # one part in front, one past the first block's lanes and the last: each with the roots of its neighbour
    for j in (0, 257, 299):
        bent = list(ts)
        other = parts[j - 1]
        bent[j] = MemTransition(parts[j]["a"], parts[j]["old"], parts[j]["new"], parts[j]["words"], other["root0"], other["root1"])
        got = verify_transitions(bent, backend.L, with_roots=True)
        assert got[j] == (False, want[j][1]) and got[:j] + got[j + 1:] == want[:j] + want[j + 1:]


def test_a_batch_of_one_part_equals_the_single_call(backend):
    for i in (0, 4, 8, 10, 11):
        assert verify_transitions([valid()[i]], backend.L, with_roots=True) == [verify_transition(valid()[i], backend.L, with_roots=True)]
        root, o = set_of(i)
        assert verify_sets([root], [o], backend.L, with_roots=True) == [verify_set(root, o, backend.L, with_root=True)]
        for name in TAMPERS:
            bad = tampered(i, name)
            if bad is not None:
                assert verify_transitions([bad[0]], backend.L, with_roots=True) == [verify_transition(bad[0], backend.L, with_roots=True)], (i, name)


def test_parts_without_cells(backend):
    still = MemTransition([], [], [], [], 5, 5)                                   # accepted: nothing changes and the roots agree
    moved = MemTransition([], [], [], [], 5, 6)
    wordy = MemTransition([], [], [], [1], 5, 5)
    empties = [still, moved, wordy]
    want = [(True, (5, 5)), (False, (5, 5)), (False, (0, 0))]
    assert [verify_transition(t, backend.L, with_roots=True) for t in empties] == want
    assert verify_transitions(empties, backend.L, with_roots=True) == want        # a batch of only such parts launches nothing
    batch = [still, valid()[6], moved, valid()[8], wordy, valid()[1], still]
    assert verify_transitions(batch, backend.L, with_roots=True) == [want[0], (True, roots_of(6)), want[1], (True, roots_of(8)), want[2],
                                                                     (True, roots_of(1)), want[0]]
    none = MemSetOpening([], [], [])
    root, o = set_of(6)
    assert verify_set(7, none, backend.L, with_root=True) == (False, 0)
    assert verify_sets([7, root, 7], [none, o, none], backend.L, with_roots=True) == [(False, 0), (True, root), (False, 0)]


def test_a_part_that_fails_the_host_checks_sits_between_valid_ones(backend):
    r = reference(9)
    swapped = tampered(9, "two addresses swapped")[0]
    short = tampered(9, "one word dropped")[0]
    long = tampered(9, "one word appended")[0]
    beyond = MemTransition(r["a"][:-1] + [1 << 28], r["old"], r["new"], r["words"], r["root0"], r["root1"])
    batch = [valid()[8], swapped, valid()[9], short, long, valid()[10], beyond, valid()[0]]
    got = verify_transitions(batch, backend.L, with_roots=True)
    assert got == [(True, roots_of(8)), (False, (0, 0)), (True, roots_of(9)), (False, (0, 0)), (False, (0, 0)), (True, roots_of(10)), (False, (0, 0)),
                   (True, roots_of(0))]
    assert got == [verify_transition(t, backend.L, with_roots=True) for t in batch]
    only_bad = verify_transitions([swapped, short], backend.L, with_roots=True)   # no part reaches the device
    assert only_bad == [(False, (0, 0))] * 2


def test_a_followed_run_batched(backend):
    """the run of test_a_followed_run_rebuilds_the_final_image (tests/test_gpu_transition.py): batched=True gives the updates and
    the final image of the unbatched calls, and names the same segment in the same words"""
    from tests.test_gpu_mem_open import _heap_run
    hss = _heap_run()
    first = Run.from_segment(backend, hss[0])
    dev0 = first.adapt_next(hss[0])
    hi0 = backend.download_input(dev0)
    rows = prover_input_arrays(hi0.view)
    cells = [(int(r[0]),) + tuple(int(x) for x in r[1:5]) for r in rows["initial_memory"]]
    backend.free_input(dev0)
    hi0.free()
    first.free()
    run = Run.from_segment(backend, hss[0])
    proofs, moves = run.prove(hss, transitions=True)
    images = [MemImage.from_cells(cells, backend.L) for _ in range(4)]
    try:
        assert follow_run(proofs, moves, backend.L, batched=True) == follow_run(proofs, moves, backend.L)
        final = proofs[-1].public_data()["final_root"]
        assert follow_run_image(proofs, moves, images[0], batched=True) == follow_run_image(proofs, moves, images[1]) == final
        assert images[0].cells()[0].tobytes() == images[1].cells()[0].tobytes() and images[0].cells()[1].tobytes() == images[1].cells()[1].tobytes()
        bent = MemTransition(moves[1].addresses, moves[1].old_values, moves[1].new_values + np.uint32(1), moves[1].siblings, moves[1].root_before,
                             moves[1].root_after)
        said = []
        for kw in ({}, {"batched": True}):
            with pytest.raises(CmError) as e:
                follow_run(proofs, [moves[0], bent], backend.L, **kw)
            said.append(str(e.value))
            with pytest.raises(CmError) as e:
                follow_run(proofs, moves[::-1], backend.L, **kw)
            said.append(str(e.value))
        assert said[:2] == said[2:] and "segment 1" in said[0] and "segment 0" in said[1], said
        said = []
        for image, kw in ((images[2], {}), (images[3], {"batched": True})):
            with pytest.raises(CmError) as e:
                follow_run_image(proofs, [moves[0], bent], image, **kw)
            said.append(str(e.value))
            assert image.root == proofs[0].public_data()["final_root"]           # the image stays at the last good segment
        assert said[0] == said[1] and "segment 1" in said[0], said
    finally:
        for image in images:
            image.free()
        for p in proofs:
            p.free()
        run.free()
        for hs in hss:
            hs.free()
