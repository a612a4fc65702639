"""Host side of the composed transitions (cm_compose_transitions, device == 0) against tests/mem_compose_ref.py: every chain equals
the two set openings of the union under the first and the last tree, word for word; the host verifier accepts the result; the
operation is associative byte for byte; every refusal has its status and names its cause; the symbol is in the header and the
library.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from cairo_m_amd import lib as cm_lib
from cairo_m_amd.lib import (Backend, CmError, MemTransition, MemTransitionViewC, compose_transitions, load_library, run_transition,
                             verify_transition_host)
from tests.mem_compose_ref import CHAINS, REFUSALS, assert_equals, chain, parts_of, refusals, same_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()


def _last_error(L):
    buf = C.create_string_buffer(1024)
    L.cm_last_error(buf, C.c_size_t(1024))
    return buf.value.decode()


def _views(ts):
    views, keep = (MemTransitionViewC * max(len(ts), 1))(), []
    for i, t in enumerate(ts):
        views[i], k = cm_lib._transition_view(t)
        keep.append(k)
    return views, keep


def raw(L, ts, device=0, views=True, n_parts=None, out=True, edit=None):
    """the C call itself -> (status, message, the out handle's value)"""
    v, keep = _views(ts)
    if edit:
        edit(v)
    h = C.c_void_p(0xdead)
    rc = L.cm_compose_transitions(v if views else None, C.c_uint32(len(ts) if n_parts is None else n_parts), C.c_uint32(device),
                                  C.byref(h) if out else None)
    return rc, _last_error(L) if rc else "", h.value


@pytest.mark.parametrize("name", CHAINS)
def test_host_composition_equals_the_two_set_openings_of_the_union(name):
    c = chain(name)
    t = compose_transitions(parts_of(name), device=False)
    assert_equals(t, c["ref"])
    assert t.n_zero_only == 0
    assert verify_transition_host(t) == (0, "")
    assert same_bytes(t, compose_transitions(parts_of(name), device=False))      # the same call, the same bytes


def test_one_part_composes_to_itself():
    (p,) = parts_of("one")
    q = MemTransition(p.addresses, p.old_values, p.new_values, p.siblings, p.root_before, p.root_after, n_zero_only=3)
    t = compose_transitions([q], device=False)
    assert same_bytes(t, q) and t.n_zero_only == 3


def test_the_stale_word_of_the_buddies_is_not_used():
    c = chain("buddies")
    t = compose_transitions(parts_of("buddies"), device=False)
    assert t.siblings.size == 27 and c["parts"][1]["words"][0] not in t.siblings.tolist()


def test_empty_parts_add_nothing():
    with_e, without = compose_transitions(parts_of("empties"), device=False), compose_transitions(parts_of("no_empties"), device=False)
    assert same_bytes(with_e, without)
    t = compose_transitions(parts_of("all_empty"), device=False)
    assert t.addresses.size == 0 and t.siblings.size == 0 and t.root_before == t.root_after == chain("all_empty")["trees"][0].root
    assert verify_transition_host(t) == (0, "")


def test_n_zero_only_is_the_sum_of_the_parts():
    ps = parts_of("far")
    ps[0].n_zero_only, ps[1].n_zero_only = 2, 5
    assert compose_transitions(ps, device=False).n_zero_only == 7


@pytest.mark.parametrize("name", ["gap_and_restore", "wide"])
def test_composition_is_associative_byte_for_byte(name):
    ps = parts_of(name)
    comp = lambda x: compose_transitions(x, device=False)
    for cut in range(1, len(ps) - 1):
        p1, p2, p3 = ps[:cut], ps[cut:cut + 1], ps[cut + 1:]
        flat = comp(ps)
        assert same_bytes(comp([comp(p1 + p2)] + p3), flat)
        assert same_bytes(comp(p1 + [comp(p2 + p3)]), flat)


@pytest.mark.parametrize("what", REFUSALS)
def test_each_broken_chain_is_refused_with_its_cause(what):
    parts, status, needle = refusals()[what]
    with pytest.raises(CmError) as e:
        compose_transitions(parts, device=False)
    assert e.value.status == status and needle in e.value.message, (what, str(e.value))
    rc, msg, h = raw(load_library(), parts)
    assert (rc, h) == (status, None) and needle in msg                          # the out handle is NULL after a refusal


def test_status_1_refusals():
    L = load_library()
    ps = parts_of("far")

    def short(v):
        v[1].struct_size = C.sizeof(MemTransitionViewC) - 8

    def no_old(v):
        v[0].old_values = None

    def no_words(v):
        v[1].siblings = None

    for kw, needle in ((dict(views=False), "null argument"), (dict(out=False), "null argument"), (dict(n_parts=0), "no parts"),
                       (dict(n_parts=(1 << 16) + 1), "2^16"), (dict(device=2), "`device`"), (dict(edit=short), "part 1: struct_size"),
                       (dict(edit=no_old), "part 0: null array"), (dict(edit=no_words), "part 1: null array")):
        rc, msg, h = raw(L, ps, **kw)
        assert rc == 1 and needle in msg and (h is None or "out" in kw), (kw, rc, msg, h)
    assert raw(L, ps)[0] == 0


def test_more_than_2_pow_20_cells_in_all_is_refused_on_the_count():
    """two parts of arange addresses and zero values, no words at all: the count is refused before anything else is looked at"""
    n = (1 << 19) + 1
    zeros = np.zeros((n, 4), dtype=np.uint32)
    big = [MemTransition(np.arange(n, dtype=np.uint32), zeros, zeros, [], 1, 2), MemTransition(np.arange(n - 1, dtype=np.uint32), zeros[:-1], zeros[:-1], [], 2, 3)]
    assert sum(t.addresses.size for t in big) == (1 << 20) + 1
    rc, msg, h = raw(load_library(), big)
    assert (rc, h) == (1, None) and "compose in groups" in msg and str((1 << 20) + 1) in msg


def test_run_transition_says_what_failed():
    class FakeProof:
        def __init__(self, r0, r1):
            self.L, self.d = load_library(), {"initial_root": r0, "final_root": r1}

        def public_data(self):
            return self.d

    ps, ref = parts_of("gap_and_restore"), chain("gap_and_restore")["ref"]
    proofs = [FakeProof(p.root_before, p.root_after) for p in ps]
    assert_equals(run_transition(proofs, ps, device=False), ref)
    with pytest.raises(CmError) as e:
        run_transition(proofs, ps[::-1], device=False)
    assert "do not compose" in str(e.value) and "starts at root" in str(e.value)
    with pytest.raises(CmError) as e:
        run_transition([FakeProof(ps[0].root_before ^ 1, 0)] + proofs[1:], ps, device=False)
    assert "root before" in str(e.value) and "initial_root" in str(e.value)
    with pytest.raises(CmError) as e:
        run_transition(proofs[:-1] + [FakeProof(0, ps[-1].root_after ^ 1)], ps, device=False)
    assert "root after" in str(e.value) and "final_root" in str(e.value)
    bent = MemTransition(ps[2].addresses, ps[2].old_values, ps[2].new_values + np.uint32(1), ps[2].siblings, ps[2].root_before, ps[2].root_after)
    with pytest.raises(CmError) as e:
        run_transition(proofs, ps[:2] + [bent], device=False)
    assert "the new values hash to root" in str(e.value)


def test_the_symbol_is_declared_exported_and_bound_and_the_revision_stays():
    L = load_library()
    assert hasattr(L, "cm_compose_transitions")
    assert re.search(r"int32_t cm_compose_transitions\(const cm_mem_transition_view\* parts, uint32_t n_parts, uint32_t device, cm_mem_transition\*\* out\);", HDR)
    assert re.search(r"#define CM_ABI_REVISION 10\b", HDR)
    assert callable(compose_transitions) and callable(run_transition) and callable(Backend.compose_transitions)
    assert "cm_compose_transitions" in open(cm_lib.__file__).read()


def test_device_1_on_a_machine_without_a_gpu_is_status_3():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(CmError) as e:
        compose_transitions(parts_of("far"), device=True)
    assert e.value.status == 3 and "no HIP device" in e.value.message


def test_the_gpu_path_without_a_device_is_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the host path still answers"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library
L = load_library()
h = C.c_void_p(5)
rc = L.cm_compose_transitions(None, C.c_uint32(0), C.c_uint32(1), C.byref(h))
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
print(rc, L.cm_compose_transitions(None, C.c_uint32(0), C.c_uint32(0), C.byref(h)), h.value, buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    gpu, host, h, msg = p.stdout.strip().split(" ", 3)
    assert (int(gpu), int(host), h) == (3, 1, "None") and "no HIP device" in msg, p.stdout
