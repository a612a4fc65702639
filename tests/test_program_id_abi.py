"""Host side of the program id and the run statement (cm_program_id_entries, cm_proof_program_id, cm_program_ids,
cm_proofs_program_ids, cm_run_statement_of): the symbols, the ctypes mirror against the header's struct, the no-GPU status of the
two batch calls, and the refusal of NULL arguments.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import RunStatementC, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_program_id_entries", "cm_proof_program_id", "cm_program_ids", "cm_proofs_program_ids", "cm_run_statement_of"]
FIELDS = ["struct_size", "n_segments", "program_id", "program_start", "n_program", "initial_pc", "initial_fp", "final_pc", "final_fp",
          "initial_root", "final_root", "n_input", "n_output", "reserved0"]


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirror_matches_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_run_statement;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"uint32_t\s+(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in RunStatementC._fields_] == FIELDS
    assert [getattr(RunStatementC, f).offset for f in fields] == [4 * i for i in range(14)]
    assert C.sizeof(RunStatementC) == int(m.group(2)) == 56


def test_batch_calls_without_a_device_are_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the host calls still answer"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, program_entries, program_id, RunStatementC
L = load_library()
buf = C.create_string_buffer(512)
rcs, msgs = [], []
for call in (lambda: L.cm_program_ids(None, None, C.c_uint32(0), None, None, C.c_uint64(0)),
             lambda: L.cm_proofs_program_ids(None, C.c_uint32(0), None, None, C.c_uint64(0))):
    rcs.append(call())
    L.cm_last_error(buf, C.c_size_t(512))
    msgs.append(buf.value.decode())
out = RunStatementC()
out.struct_size = C.sizeof(RunStatementC)
# the chain check's own status passes through: no proofs is refused before the device is looked for
rcs.append(L.cm_run_statement_of(None, C.c_uint32(0), None, None, C.c_uint32(1), C.byref(out)))
rcs.append(L.cm_verify_run_device(None, C.c_uint32(0), None))
print(*rcs, program_id(program_entries(5, [[1, 2, 3, 4]])), "|".join(msgs))
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    a, b, c, d, host_id, msg = p.stdout.strip().split(" ", 5)
    assert (int(a), int(b)) == (3, 3) and int(c) == int(d) == 1, p.stdout
    assert msg.count("no HIP device") == 2 and "cm_program_ids" in msg and "cm_proofs_program_ids" in msg
    assert int(host_id) == 0x47d99bfb                                           # the reference's test_single_element_tree shape


def test_host_calls_refuse_null_arguments():
    L = load_library()
    e, got = (C.c_uint32 * 7)(1, 5, 1, 2, 3, 4, 0), C.c_uint32(0)

    def refused(rc, word=b"null"):
        buf = C.create_string_buffer(256)
        L.cm_last_error(buf, C.c_size_t(256))
        return rc == 1 and word in buf.value

    assert refused(L.cm_program_id_entries(None, C.c_uint64(1), C.byref(got)))
    assert refused(L.cm_program_id_entries(e, C.c_uint64(1), None))
    assert L.cm_program_id_entries(e, C.c_uint64(1), C.byref(got)) == 0 and got.value == 0x47d99bfb
    assert refused(L.cm_proof_program_id(None, C.byref(got)))
    out = RunStatementC()
    assert refused(L.cm_run_statement_of(None, C.c_uint32(0), None, None, C.c_uint32(0), None))
    assert refused(L.cm_run_statement_of(None, C.c_uint32(0), None, None, C.c_uint32(0), C.byref(out)), b"struct_size")
    out.struct_size = C.sizeof(RunStatementC)
    assert refused(L.cm_run_statement_of(None, C.c_uint32(0), None, None, C.c_uint32(2), C.byref(out)), b"`device`")
    assert refused(L.cm_run_statement_of(None, C.c_uint32(0), None, None, C.c_uint32(0), C.byref(out)), b"cm_verify_run: no proofs")
