"""Host side of the memory transitions against tests/mem_transition_ref.py: the premise of the statement on the reference alone
(the sibling words of a set are the same under two trees that differ only inside it), cm_verify_memory_transition_host on the
reference and on every tamper, the view struct against the header and the no-GPU statuses of the device calls.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cairo_m_amd.lib import (MemSetOpening, MemTransition, MemTransitionViewC, load_library, set_root, verify_set_host,
                             verify_transition_host)
from tests.mem_set_ref import SET_IDS, SETS, check_set
from tests.mem_transition_ref import P, ZERO, reference, second_memory, tampers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_input_write_set", "cm_input_open_transition", "cm_mem_transition_get", "cm_mem_transition_free", "cm_verify_memory_transition",
       "cm_verify_memory_transition_host", "cm_prove_run_transitions"]


def _transition(a, old, new, words, r0, r1):
    return MemTransition(a, old, new, words, r0, r1)


def test_the_second_memories_hold_the_edge_cells_the_statement_names():
    zeroed = [second_memory(i)[1] for i in range(len(SETS))]
    created = [second_memory(i)[2] for i in range(len(SETS))]
    top = [second_memory(i)[3] for i in range(len(SETS))]
    assert any(z is not None for z in zeroed) and any(created) and any(t is not None for t in top)
    for i, (_, a) in enumerate(SETS):
        r = reference(i)
        assert not any(tuple(o) == tuple(n) for o, n in zip(r["old"].tolist(), r["new"].tolist()))   # every cell of the set changes
        if zeroed[i] is not None:
            assert tuple(r["new"][a.index(zeroed[i])]) == ZERO and tuple(r["old"][a.index(zeroed[i])]) != ZERO
        for x in created[i]:
            assert tuple(r["old"][a.index(x)]) == ZERO and tuple(r["new"][a.index(x)]) != ZERO
        if top[i] is not None:
            assert r["new"][a.index(top[i])][3] == P - 1


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_the_words_under_both_trees_are_identical(i):
    """the premise, on the reference alone: two trees that differ only in cells of the set give the set the same sibling words"""
    r = reference(i)
    assert r["words"] == r["words_after"] and len(r["words"]) == sum(r["counts"])
    assert r["root0"] != r["root1"]
    assert check_set(r["root0"], r["a"], r["old"], r["words"]) and check_set(r["root1"], r["a"], r["new"], r["words"])
    assert not check_set(r["root1"], r["a"], r["old"], r["words"])


@pytest.mark.parametrize("i", range(len(SETS)), ids=SET_IDS)
def test_host_verifier_accepts_the_reference_and_names_every_tamper(i):
    r = reference(i)
    t = _transition(r["a"], r["old"], r["new"], r["words"], r["root0"], r["root1"])
    assert verify_transition_host(t) == (0, "")
    assert t.nbytes == 36 * len(r["a"]) + 4 * len(r["words"])
    cases = tampers(r)
    assert len(cases) == (11 if len(r["a"]) > 1 else 10)
    for what, (a, old, new, w, r0, r1, needle, still) in cases.items():
        rc, msg = verify_transition_host(_transition(a, old, new, w, r0, r1))
        assert rc == 11 and msg.startswith(f"memory transition of {len(a)} cells: ") and needle in msg, (what, rc, msg)
        if still in ("old", "both"):                                              # only the named side is wrong: the other still folds
            assert verify_set_host(r["root0"], MemSetOpening(a, old, w)) == (0, ""), what
        if still in ("new", "both"):
            assert verify_set_host(r["root1"], MemSetOpening(a, new, w)) == (0, ""), what
        if still == "new":
            assert set_root(MemSetOpening(a, old, w)) != r["root0"], what
        if still == "old":
            assert set_root(MemSetOpening(a, new, w)) != r["root1"], what


def test_no_cells_is_accepted_exactly_when_the_roots_are_equal():
    none = np.zeros((0, 4), dtype=np.uint32)
    assert verify_transition_host(MemTransition([], none, none, [], 7, 7)) == (0, "")
    rc, msg = verify_transition_host(MemTransition([], none, none, [], 7, 8))
    assert rc == 11 and msg == "memory transition of 0 cells: no cell changes, and root 7 is not root 8"
    rc, msg = verify_transition_host(MemTransition([], none, none, [1], 7, 7))
    assert rc == 11 and "1 sibling words where the addresses need 0" in msg


def test_a_superset_of_the_write_set_is_a_valid_transition():
    """cells with old == new ride along: the set of SETS[11] under a second memory that differs only in SETS[11]'s first ten cells"""
    from tests.mem_set_ref import RefTree, range_memories, ref_set
    name, a = SETS[11]
    cells = {c[0]: tuple(c[1:]) for c in range_memories()[name]}
    before = RefTree([(x,) + v for x, v in cells.items()])
    for j, x in enumerate(a[:10]):
        cells[x] = (j + 1, 0, P - 1, 5)
    after = RefTree([(x,) + v for x, v in cells.items()])
    words, old, _ = ref_set(before, a)
    words_after, new, _ = ref_set(after, a)
    assert words == words_after and np.array_equal(old[10:], new[10:]) and not np.array_equal(old[:10], new[:10])
    assert verify_transition_host(MemTransition(a, old, new, words, before.root, after.root)) == (0, "")


def test_status_1_is_for_null_arguments_and_oversized_sets_only():
    L = load_library()
    one, words = (C.c_uint32 * 4)(), (C.c_uint32 * 28)()

    def call(addresses=one, n=1, old=one, new=one, sib=words):
        rc = L.cm_verify_memory_transition_host(C.c_uint32(0), C.c_uint32(0), addresses, C.c_uint64(n), old, new, sib, C.c_uint32(28))
        buf = C.create_string_buffer(512)
        L.cm_last_error(buf, C.c_size_t(512))
        return rc, buf.value.decode()

    for kw in (dict(addresses=None), dict(old=None), dict(new=None), dict(sib=None)):
        rc, msg = call(**kw)
        assert rc == 1 and "null argument" in msg, (kw, rc, msg)
    rc, msg = call(n=(1 << 20) + 1)
    assert rc == 1 and "split the set" in msg
    rc, msg = call()                                                              # a well-formed record of zeros that folds elsewhere
    assert rc == 11 and "the old values hash to root" in msg


def test_symbols_and_the_view_struct_match_the_header():
    L = load_library()
    for name in NEW:
        assert hasattr(L, name), name
        assert re.search(r"\b" + name + r"\(", HDR), name
    body = re.search(r"typedef struct \{([^}]*)\} cm_mem_transition_view;\s*/\* sizeof = (\d+) \*/", HDR)
    fields = re.findall(r"(const uint32_t\*|uint32_t)\s+(\w+);", body.group(1))
    assert [f[1] for f in fields] == [n for n, _ in MemTransitionViewC._fields_]
    for (ty, name), (_, ct) in zip(fields, MemTransitionViewC._fields_):
        assert (ct is C.c_uint32) == (ty == "uint32_t"), name
    assert C.sizeof(MemTransitionViewC) == int(body.group(2)) == 56
    assert "typedef struct cm_mem_transition cm_mem_transition;" in HDR


def test_device_calls_without_a_device_are_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the host verifier and the handle
    calls still answer"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library
L = load_library()
one, words = (C.c_uint32 * 4)(), (C.c_uint32 * 28)()
ok, n, z, h = C.c_uint8(7), C.c_uint64(7), C.c_uint64(7), C.c_void_p()
rcs = [L.cm_verify_memory_transition(C.c_uint32(0), C.c_uint32(0), one, C.c_uint64(1), one, one, words, C.c_uint32(28), C.byref(ok), None, C.c_uint64(0)),
       L.cm_input_write_set(None, None, C.c_uint64(0), C.byref(n), C.byref(z)),
       L.cm_input_open_transition(None, None, C.c_uint64(0), C.byref(h))]
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
host = L.cm_verify_memory_transition_host(C.c_uint32(0), C.c_uint32(0), one, C.c_uint64(1), one, one, words, C.c_uint32(28))
print(*rcs, host, L.cm_mem_transition_get(None, None), L.cm_mem_transition_free(None), ok.value, n.value, int(bool(h.value)), buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    a, b, c, host, get, free, ok, n, h, msg = p.stdout.strip().split(" ", 9)
    assert (int(a), int(b), int(c)) == (3, 3, 3) and "no HIP device" in msg, p.stdout
    assert (int(host), int(get), int(free)) == (11, 1, 0) and (int(ok), int(n), int(h)) == (7, 7, 0)   # verdicts; nothing written
