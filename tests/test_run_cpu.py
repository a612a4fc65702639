"""Host side of the run layer (header revision 10): the ABI revision, the new symbols and struct sizes against lib.py, cm_verify_run
and cm_proof_public_data on oracle-made proofs (no GPU: the proofs travel as words through cm_proof_from_words)."""
import ctypes as C
import json
import os
import re

import numpy as np

from cairo_m_amd.lib import Proof, PublicDataC, RunSegmentC, load_library, prover_input_arrays, verify_run, vm_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_run_begin", "cm_run_adapt_next", "cm_run_memory", "cm_run_free", "cm_prove_run", "cm_proof_public_data",
       "cm_proof_public_entries", "cm_verify_run", "cm_host_segment_end_lengths"]


def test_abi_revision_is_10():
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name


def _c_struct_bytes(name):
    """size of a header struct made of uint32_t / uint64_t / pointer fields (natural alignment)"""
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, hdr, re.S).group(1)
    off = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = re.match(r"((?:const )?\w+\*?)\s+(.*)", decl, re.S).groups()
        size = 8 if ty.endswith("*") or "uint64_t" in ty else 4
        for _ in names.split(","):
            off = (off + size - 1) // size * size + size
    return (off + 7) // 8 * 8 if "uint64_t" in body or "*" in body else off


def test_struct_sizes_match_lib_py():
    assert C.sizeof(RunSegmentC) == _c_struct_bytes("cm_run_segment") == 48
    assert C.sizeof(PublicDataC) == _c_struct_bytes("cm_public_data") == 48


def _chain_proofs(oracle):
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
    return L, proofs, inputs


def test_verify_run_on_oracle_proofs(oracle):
    L, proofs, inputs = _chain_proofs(oracle)
    assert verify_run(proofs) == (0, "")
    assert verify_run(proofs[2:3]) == (0, "")
    rc, msg = verify_run([proofs[0], proofs[2], proofs[1], proofs[3]])
    assert rc == 11 and msg == "run: segment 1 initial_pc != segment 0 final_pc", msg
    rc, msg = verify_run([proofs[0], proofs[1], proofs[3]])
    assert rc == 11 and msg == "run: segment 2 initial_pc != segment 1 final_pc", msg
    # a proof that does not verify is named before any link is looked at
    rc, msg = verify_run(proofs, cfg=(16, 1, 0, 79))
    assert rc == 11 and msg.startswith("run: segment 0: verification failed: "), msg
    assert L.cm_verify_run(None, C.c_uint32(0), None) == 1
    for p in proofs:
        p.free()
    for hi in inputs:
        hi.free()


def test_public_data_equals_the_proof_json(oracle):
    L, proofs, inputs = _chain_proofs(oracle)
    for p, hi in zip(proofs, inputs):
        pd, doc = p.public_data(), json.loads(p.json())["public_data"]
        assert {"pc": pd["initial_pc"], "fp": pd["initial_fp"]} == doc["initial_registers"]
        assert {"pc": pd["final_pc"], "fp": pd["final_fp"]} == doc["final_registers"]
        assert (pd["clock"], pd["initial_root"], pd["final_root"]) == (doc["clock"], doc["initial_root"], doc["final_root"])
        a = prover_input_arrays(hi.view)
        assert [pd["initial_root"], pd["final_root"]] == a["roots"]
        for name, lo, hi_ in (("program", a["ranges"][0], a["ranges"][1]), ("input", a["ranges"][2], a["ranges"][3]),
                              ("output", a["ranges"][4], a["ranges"][5])):
            ent, want = pd[name], doc["public_memory"][name]
            assert ent.shape == (max(hi_ - lo, 0), 7) and len(want) == ent.shape[0]
            for row, w in zip(ent, want):
                if w is None:
                    assert not row.any()
                else:
                    addr, value, clock = w
                    assert row.tolist() == [1, addr, value[0][0], value[0][1], value[1][0], value[1][1], clock]
    # struct_size is checked, a short capacity is refused with the count reported
    d = PublicDataC()
    assert L.cm_proof_public_data(proofs[0].h, C.byref(d)) == 1
    n = C.c_uint64(0)
    buf = (C.c_uint32 * 7)()
    assert L.cm_proof_public_entries(proofs[0].h, C.c_uint32(0), buf, C.c_uint64(1), C.byref(n)) == 1 and n.value == 7
    assert L.cm_proof_public_entries(proofs[0].h, C.c_uint32(3), None, C.c_uint64(0), C.byref(n)) == 1
    for p in proofs:
        p.free()
    for hi in inputs:
        hi.free()
