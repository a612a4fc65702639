"""Host side of the memory openings (cm_input_open_memory, cm_run_open_memory, cm_verify_memory_openings,
cm_verify_memory_opening): the symbols, the ctypes mirror against the header's struct, the no-GPU status of the three device
calls, and the refusal of NULL arguments.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import MemOpening, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_input_open_memory", "cm_run_open_memory", "cm_verify_memory_openings", "cm_verify_memory_opening"]


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirror_matches_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_opening;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, name, arr = re.match(r"(\w+)\s+(\w+)(?:\[(\d+)\])?$", decl).groups()
            assert ty == "uint32_t"
            fields.append((name, 4 * int(arr or 1)))
    assert [f[0] for f in MemOpening._fields_] == [f[0] for f in fields] == ["address", "present", "value", "siblings"]
    off = 0
    for (name, cty), (_, size) in zip(MemOpening._fields_, fields):
        assert C.sizeof(cty) == size and getattr(MemOpening, name).offset == off, name
        off += size
    assert C.sizeof(MemOpening) == off == int(m.group(2)) == 136


def test_device_calls_without_a_device_are_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the host verifier still answers"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library, MemOpening, verify_opening
L = load_library()
root, ok, o = C.c_uint32(0), (C.c_uint8 * 1)(), MemOpening()
rcs = [L.cm_input_open_memory(None, C.c_uint32(0), None, C.c_uint64(0), None, C.byref(root)),
       L.cm_run_open_memory(None, None, C.c_uint64(0), None, C.byref(root)),
       L.cm_verify_memory_openings(C.c_uint32(0), C.byref(o), C.c_uint64(1), ok, C.c_uint64(0))]
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
print(*rcs, verify_opening(1, o)[0], buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    a, b, c, host, msg = p.stdout.strip().split(" ", 4)
    assert (int(a), int(b), int(c)) == (3, 3, 3) and "no HIP device" in msg, p.stdout
    assert int(host) == 11                                                        # a verdict, not a missing device


def test_host_verifier_refuses_a_null_opening():
    L = load_library()
    assert L.cm_verify_memory_opening(C.c_uint32(0), None) == 1
    buf = C.create_string_buffer(256)
    L.cm_last_error(buf, C.c_size_t(256))
    assert b"null" in buf.value
