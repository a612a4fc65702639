"""cm_program_id_entries / cm_proof_program_id / cm_run_statement_of in host code: the id of a program is the root of the partial
memory tree that holds only its cells (Proof::program_id, crates/prover/src/lib.rs:75-97).  Held to two roots that owe nothing to
the new code: lib.partial_merkle_tree, the host restatement of merkle.rs:183-295, and for the small shapes a plain-Python tree
(RefTree's node records hashed once more in Python — its map ends at depth 1 — and a sparse tree built from the leaves).  CPU only."""
import ctypes as C

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, Proof, load_library, program_entries, program_id, run_statement, verify_run, vm_run
from tests.mem_open_ref import P, SPACE, RefTree, default_hashes, poseidon2_hash
from tests.program_id_util import casm_programs, cells_of, image_values, python_root, shapes, tree_root

SHAPES = shapes()


@pytest.mark.parametrize("name,start,values,small", SHAPES, ids=[s[0] for s in SHAPES])
def test_id_is_the_root_of_the_partial_tree(name, start, values, small):
    got = program_id(program_entries(start, values))
    print(name, hex(got))
    assert got == tree_root(start, values)
    if small:
        cells = cells_of(start, values)
        ref = RefTree(cells)
        assert got == poseidon2_hash(ref.node(1, 0), ref.node(1, 1)) == python_root(cells)


def test_casm_programs_have_distinct_ids():
    """all 122 compiler-emitted programs laid out from address 0: the C yardstick's root, and one id per distinct image"""
    progs = casm_programs()
    assert len(progs) == 122
    by_words = {}
    for name, values in progs:
        got = program_id(program_entries(0, values))
        assert got == tree_root(0, values), name
        by_words.setdefault(values.tobytes(), set()).add(got)
    assert all(len(ids) == 1 for ids in by_words.values())
    ids = [next(iter(s)) for s in by_words.values()]
    assert len(set(ids)) == len(ids) > 100


def test_zero_cell_is_the_default():
    """a present all-zero cell hashes as an absent one: a property of the tree, stated in DESIGN"""
    v = np.array([[7, 1, 2, 3], [0, 0, 0, 0], [9, 0, 0, 4]], dtype=np.uint32)
    got = program_id(program_entries(6, v))
    assert got == partial_root([(6, 7, 1, 2, 3), (8, 9, 0, 0, 4)]) == tree_root(6, v)
    assert program_id(program_entries(123, [[0, 0, 0, 0]])) == default_hashes()[0]


def partial_root(cells):
    ref = RefTree(cells)
    return poseidon2_hash(ref.node(1, 0), ref.node(1, 1))


def test_clocks_do_not_enter_and_values_do():
    e = program_entries(3, SHAPES[3][2])
    base = program_id(e)
    other = e.copy()
    other[:, 6] = [5, 0, P - 1, 77]
    assert program_id(other) == base
    for row, word in ((0, 2), (3, 5), (1, 3)):
        other = e.copy()
        other[row, word] = (int(other[row, word]) + 1) % P
        assert program_id(other) != base


def _refused(entries, n=None, lib=None):
    L = lib or load_library()
    e = np.ascontiguousarray(entries, dtype=np.uint32)
    got = C.c_uint32(0xdead)
    rc = L.cm_program_id_entries(e.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(e.shape[0] if n is None else n), C.byref(got))
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    assert got.value == 0xdead or rc == 0                                       # nothing written by a refusal
    return rc, buf.value.decode()


def test_refusals():
    good = program_entries(10, [[1, 2, 3, 4]] * 4)
    assert _refused(good)[0] == 0
    assert _refused(good, n=0) == (1, "cm_program_id_entries: no entries: a program of no cells has no id")
    e = good.copy()
    e[2, 0] = 0
    assert _refused(e) == (1, "cm_program_id_entries: entry 2 (address 12) is absent")
    e = good.copy()
    e[0] = 0                                                                    # the all-zero record of an absent cell
    assert _refused(e) == (1, "cm_program_id_entries: entry 0 (address 0) is absent")
    e = good.copy()
    e[3, 1] = 14
    assert _refused(e) == (1, "cm_program_id_entries: entry 3 has address 14, not 13")
    e = good.copy()
    e[1, 1] = 10                                                                # a repeated address
    assert _refused(e) == (1, "cm_program_id_entries: entry 1 has address 10, not 11")
    for word, value in ((0, P), (3, 0xffffffff)):
        e = good.copy()
        e[2, 2 + word] = value
        assert _refused(e) == (1, f"cm_program_id_entries: value word {word} of entry 2 (address 12) is not below P")
    e = program_entries(SPACE - 3, [[1, 2, 3, 4]] * 4)
    assert _refused(e) == (1, f"cm_program_id_entries: the range [{SPACE - 3}, {SPACE + 1}) ends beyond the address space of 2^28 cells")
    e = program_entries(SPACE, [[1, 2, 3, 4]])
    assert _refused(e)[0] == 1 and "ends beyond the address space" in _refused(e)[1]
    assert _refused(good, n=(1 << 24) + 1) == (1, f"cm_program_id_entries: more than 2^24 entries ({(1 << 24) + 1})")
    with pytest.raises(CmError, match="entry 2 .address 12. is absent"):
        e = good.copy()
        e[2, 0] = 0
        program_id(e)
    with pytest.raises(CmError, match="no entries"):
        program_id(np.zeros((0, 7), dtype=np.uint32))


def test_program_entries_helper():
    e = program_entries(5, [[1, 2, 3, 4], [9], [7, 8]])
    assert e.dtype == np.uint32 and e.tolist() == [[1, 5, 1, 2, 3, 4, 0], [1, 6, 9, 0, 0, 0, 0], [1, 7, 7, 8, 0, 0, 0]]


# ---- proofs without a GPU: the oracle's, parsed by cm_proof_from_words ---------------------------------------------------------
@pytest.fixture(scope="module")
def chain(oracle):
    from tests.test_oracle_air import CHAIN_PROG
    L = load_library()
    proofs, inputs = [], []
    for s in range(4):
        hi = vm_run(CHAIN_PROG, max_steps=2, segment=s)
        words, _ = oracle.prove(hi.view)
        w = np.ascontiguousarray(words, dtype=np.uint32)
        h = C.c_void_p()
        assert L.cm_proof_from_words(w.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(w.size), C.byref(h)) == 0
        proofs.append(Proof(L, h))
        inputs.append(hi)
    yield CHAIN_PROG, proofs
    for p in proofs:
        p.free()
    for hi in inputs:
        hi.free()


def test_proof_program_id_is_the_id_of_its_instruction_words(chain):
    prog, proofs = chain
    rows = image_values(prog)
    want = tree_root(0, rows)
    for p in proofs:
        pd = p.public_data()
        assert np.array_equal(pd["program"][:, 2:6], rows) and pd["program"][:, 0].all()
        assert p.program_id() == want == program_id(pd["program"])


def test_run_statement_in_host_code(chain):
    prog, proofs = chain
    rc, msg, st = run_statement(proofs)
    assert (rc, msg) == (0, "")
    first, last = proofs[0].public_data(), proofs[-1].public_data()
    assert st["n_segments"] == 4 and st["program_id"] == proofs[0].program_id()
    assert (st["program_start"], st["n_program"]) == (int(first["program"][0, 1]), first["program"].shape[0])
    assert [st[k] for k in ("initial_pc", "initial_fp", "initial_root")] == [first[k] for k in ("initial_pc", "initial_fp", "initial_root")]
    assert [st[k] for k in ("final_pc", "final_fp", "final_root")] == [last[k] for k in ("final_pc", "final_fp", "final_root")]
    assert (st["n_input"], st["n_output"]) == (first["input"].shape[0], last["output"].shape[0])
    assert np.array_equal(st["input"], first["input"]) and np.array_equal(st["output"], last["output"])
    assert run_statement(proofs, program_id=st["program_id"])[0] == 0
    wrong = st["program_id"] ^ 1
    assert run_statement(proofs, program_id=wrong)[:2] == (11, "run: program_id 0x%08x != expected 0x%08x" % (st["program_id"], wrong))
    # the chain check comes first and keeps its own words
    swapped = [proofs[0], proofs[2], proofs[1], proofs[3]]
    assert run_statement(swapped, program_id=wrong)[:2] == verify_run(swapped) == (11, "run: segment 1 initial_pc != segment 0 final_pc")
    assert run_statement(proofs, cfg=(16, 1, 0, 79))[:2] == verify_run(proofs, cfg=(16, 1, 0, 79))
    assert run_statement(proofs[1:2])[2]["n_segments"] == 1
