"""Host side of the batched device verifier (cm_verify_many, cm_verify_run_device): the symbols and the struct against the
header and lib.py, the order of the CM_VERIFY_* ids, the ABI revision (still 10: the change is additive), and the answer on a machine
without a GPU.  That the host verifier says what it said before its helpers moved into verifier_common.hpp is what
tests/test_verifier.py, tests/test_framing.py and tests/test_run_cpu.py check, unedited."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from cairo_m_amd.lib import CmError, VerifyResultC, load_library, synth_fibonacci, verify_many, verify_run
from tests.verify_many_util import hand_flips, host_verify_words, proof_from_words, proof_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_verify_many", "cm_verify_run_device", "cm_verify_many_timing", "cm_verify_plan_stats", "cm_verify_many_detail"]
# the host verifier's order (cairo_m_amd/csrc/verifier_common.hpp verify_prelude, then verifier.hip verify_proof)
ORDER = ["STRUCTURE", "POW_INTERACTION", "LOGUP_SUM", "OODS", "FRI_STRUCTURE", "POW", "MERKLE", "QUERIED_VALUES", "FRI_FIRST_EVALS",
         "FRI_FIRST_COMMITMENT", "FRI_INNER_EVALS", "FRI_INNER_COMMITMENT", "FRI_LAST_EVALS"]


def test_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name


def test_abi_revision_is_still_10_and_says_why():
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10
    comment = HDR[:HDR.index("#define CM_ABI_REVISION")]
    assert "cm_verify_many" in comment and "additive" in comment


def _header_struct_bytes(name):
    """size of a header struct of int32_t / uint32_t / char[n] fields"""
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    body = re.search(r"typedef struct %s \{([^}]*)\} %s;" % (name, name), hdr, re.S).group(1)
    size = 0
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, nm, arr = re.match(r"(\w+)\s+(\w+)(?:\[(\d+)\])?$", decl).groups()
        unit = {"int32_t": 4, "uint32_t": 4, "char": 1}[ty]
        size = (size + unit - 1) // unit * unit + unit * int(arr or 1)
    return (size + 3) // 4 * 4


def test_struct_size_matches_lib_py():
    assert C.sizeof(VerifyResultC) == _header_struct_bytes("cm_verify_result") == 168
    assert [f[0] for f in VerifyResultC._fields_] == ["status", "check", "message"]


def test_check_ids_follow_the_host_verifiers_order():
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define CM_VERIFY_(\w+) (\d+)", HDR)}
    assert sorted(ids) == sorted(ORDER)
    values = [ids[n] for n in ORDER]
    assert values[0] >= 1 and all(a < b for a, b in zip(values, values[1:])), values


def test_argument_errors_come_before_the_device():
    L = load_library()
    assert L.cm_verify_many(None, C.c_uint32(0), None, None, C.c_uint64(0)) == 1
    assert L.cm_verify_run_device(None, C.c_uint32(0), None) == 1
    null = (C.c_void_p * 1)(None)
    assert L.cm_verify_many(null, C.c_uint32(1), None, None, C.c_uint64(0)) == 1
    buf = C.create_string_buffer(256)
    L.cm_last_error(buf, C.c_size_t(256))
    assert buf.value == b"cm_verify_many: null proof"


def test_no_cpu_fallback_without_gpu(oracle):
    """cm_verify_many is a GPU entry point: without a device it answers cm_init's status, 3, for a proof the host verifier
    accepts — never 0.  (tests/test_abi.py::test_no_cpu_fallback_without_gpu is the pattern.)"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = load_library()
    inp = synth_fibonacci(5)
    words, _ = oracle.prove(inp.view)
    inp.free()
    p = proof_from_words(L, words)
    assert p.verify() == (0, "")
    hs = (C.c_void_p * 1)(p.h.value)
    res = (VerifyResultC * 1)()
    assert L.cm_verify_many(hs, C.c_uint32(1), None, res, C.c_uint64(0)) == 3
    assert L.cm_verify_run_device(hs, C.c_uint32(1), None) == 3
    with pytest.raises(CmError, match="no HIP device"):
        verify_many([p])
    rc, msg = verify_run([p], device=True)
    assert rc == 3 and "no HIP device" in msg
    assert verify_run([p]) == (0, "")          # the default stays the host path
    p.free()


def test_layout_helper_and_tamper_counts_of_the_gpu_test(oracle):
    """What tests/test_gpu_verify_many.py relies on, checked with the host verifier alone: the layout helper walks the whole
    stream, every hand-placed flip of synth_fibonacci(7) is rejected, and of the 64 flips of default_rng(1) at least 62 are
    rejected and at most 2 no longer parse (measured: 64 and 0)."""
    L = load_library()
    inp = synth_fibonacci(7)
    words, _ = oracle.prove(inp.view)
    inp.free()
    lay = proof_layout(words)
    assert len(lay["commitments"]) == 4 and len(lay["fri_inner"]) == 20 and lay["last_poly"][1] == 1
    for name, pos in hand_flips(words).items():
        bad = words.copy()
        bad[pos] ^= 1
        assert host_verify_words(L, bad)[0] == 11, name
    rejected = unparsed = 0
    for pos in np.random.default_rng(1).integers(8, words.size - 1, size=64):
        bad = words.copy()
        bad[pos] ^= 1
        p = proof_from_words(L, bad)
        if p is None:
            unparsed += 1
            continue
        rejected += p.verify()[0] == 11
        p.free()
    assert rejected + unparsed >= 62 and unparsed <= 2, (rejected, unparsed)
