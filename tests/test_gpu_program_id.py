"""GPU: cm_program_ids / cm_proofs_program_ids (k_pid_cells, k_pid_tree) against the host fold, which tests/test_program_id_cpu.py
holds to the reference's tree; proofs' ids against the id of the instruction words the test itself assembled; the statement of a
run in host code and on the device."""
import numpy as np
import pytest

from cairo_m_amd.lib import (mem_stats, partial_merkle_tree, program_entries, program_id, run_statement, synth_fibonacci,
                             synth_fibonacci_segment, verify_run)
from tests.casm_fixtures import load, run_case
from tests.mem_open_ref import P
from tests.program_id_util import casm_programs, cells_of, field_values, image_values, shapes

pytestmark = pytest.mark.gpu

# fibonacci_loop as the synthetic VM runs it: the words the test compares the proofs' program with
FIB = [[9, 0, 0], [9, 1, 1], [9, 0, 2], [4, P - 4, 0, 3], [1, 2, 3, 5], [14, 5, 3], [9, 0, 5], [13, 2], [9, 1, 5], [14, 5, 2], [13, 7],
       [0, 0, 1, 6], [4, 1, 0, 0], [4, 6, 0, 1], [4, 2, 1, 7], [4, 7, 0, 2], [13, P - 12], [4, 0, 0, P - 3], [11]]


def _tree_id(program):
    """through the host restatement of build_partial_merkle_tree, never through the new code"""
    return partial_merkle_tree(cells_of(0, image_values(program)), initial=True, ranges=(0,) * 6)[1]


@pytest.fixture(scope="module")
def batch():
    """every shape of the CPU file, n = 4097 and the 122 compiler-emitted programs, sizes shuffled, two bad items in the middle"""
    items = [(name, program_entries(start, values)) for name, start, values, _ in shapes()]
    items.append(("n 4097", program_entries(777, field_values(4097, 9))))
    items += [(name, program_entries(0, values)) for name, values in casm_programs()]
    order = np.random.default_rng(12).permutation(len(items))
    items = [items[i] for i in order]
    absent = program_entries(40, field_values(9, 10))
    absent[4] = 0
    big_word = program_entries(1 << 20, field_values(1500, 11))
    big_word[1234, 3] = P
    mid = len(items) // 2
    items[mid:mid] = [("absent entry", absent), ("word = P", big_word)]
    return items, {mid: "item %d: entry 4 (address 44) is absent" % mid,
                   mid + 1: "item %d: value word 1 of entry 1234 (address %d) is not below P" % (mid + 1, (1 << 20) + 1234)}


def test_one_batch_of_every_shape(backend, batch):
    items, bad = batch
    before = mem_stats(backend.L).live_bytes
    ids, status, msg = backend.program_ids([e for _, e in items], with_status=True)
    assert status == [1 if i in bad else 0 for i in range(len(items))]
    assert msg == bad[min(bad)]
    for i, (name, e) in enumerate(items):
        if i in bad:
            assert ids[i] == 0, name
        else:
            assert ids[i] == program_id(e, backend.L), name
    again = backend.program_ids([e for _, e in items], with_status=True)
    assert again[0].tobytes() == ids.tobytes() and again[1:] == (status, msg)
    assert mem_stats(backend.L).live_bytes == before                            # the call keeps nothing
    # the other bad item alone, and a batch of good ones through the raising form
    only = backend.program_ids([items[max(bad)][1]], with_status=True)
    assert only[1] == [1] and only[2] == bad[max(bad)].replace("item %d" % max(bad), "item 0")
    good = [e for i, (_, e) in enumerate(items) if i not in bad][:5]
    assert backend.program_ids(good).tolist() == [program_id(e, backend.L) for e in good]


@pytest.fixture(scope="module")
def two_proofs(backend):
    fx = next(f for f in load() if f["provable"])
    inp_fib = synth_fibonacci(7)
    inp_casm, _ = run_case(fx, fx["cases"][-1], backend.L)
    proofs = [backend.prove(inp_fib), backend.prove(inp_casm)]
    inp_fib.free()
    inp_casm.free()
    yield proofs, [FIB, fx["instructions"] + fx.get("data", [])]
    for p in proofs:
        p.free()


def test_proofs_name_their_programs(backend, two_proofs):
    proofs, programs = two_proofs
    want = [_tree_id(prog) for prog in programs]
    assert want[0] != want[1]
    assert [p.program_id() for p in proofs] == want
    assert backend.program_ids(proofs).tolist() == want
    assert backend.program_ids([proofs[1]]).tolist() == want[1:]
    assert backend.program_ids([p.public_data()["program"] for p in proofs]).tolist() == want


def test_run_statement_on_host_and_device(backend):
    segs = [synth_fibonacci_segment(300, max_steps=1100, segment=s) for s in range(3)]
    got = backend.prove_run(segs, inflight=2)
    try:
        assert len(got) == 3
        host = run_statement(got)
        dev = backend.run_statement(got, device=True)
        assert host[:2] == (0, "") == dev[:2]
        st = host[2]
        assert st.keys() == dev[2].keys()
        for k in st:
            assert np.array_equal(st[k], dev[2][k]), k
        first, last = got[0].public_data(), got[-1].public_data()
        assert st["n_segments"] == 3 and (st["program_start"], st["n_program"]) == (0, len(FIB))
        assert [st[k] for k in ("initial_pc", "initial_fp", "initial_root", "n_input")] == \
            [first["initial_pc"], first["initial_fp"], first["initial_root"], first["input"].shape[0]]
        assert [st[k] for k in ("final_pc", "final_fp", "final_root", "n_output")] == \
            [last["final_pc"], last["final_fp"], last["final_root"], last["output"].shape[0]]
        assert np.array_equal(st["input"], first["input"]) and np.array_equal(st["output"], last["output"])
        assert [p.program_id() for p in got] == [st["program_id"]] * 3 == [_tree_id(FIB)] * 3
        wrong = st["program_id"] ^ 1
        want = (11, "run: program_id 0x%08x != expected 0x%08x" % (st["program_id"], wrong), None)
        assert run_statement(got, program_id=wrong) == want == backend.run_statement(got, program_id=wrong, device=True)
        assert backend.run_statement(got, program_id=st["program_id"], device=True)[0] == 0
        swapped = [got[0], got[2], got[1]]
        words = verify_run(swapped)
        assert words[0] == 11 and " initial_" in words[1]
        assert run_statement(swapped)[:2] == words == backend.run_statement(swapped, device=True)[:2]
    finally:
        for p in got:
            p.free()
        for s in segs:
            s.free()
