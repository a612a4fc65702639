"""Host side of the range openings (cm_input_open_memory_range, cm_run_open_memory_range, cm_verify_memory_range,
cm_verify_memory_range_host, cm_mem_range_plan): the symbols, the ctypes mirrors against the header's structs, the no-GPU status of
the three device calls, and the refusal of NULL arguments.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import MemRangeOpening, MemRangeStep, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_input_open_memory_range", "cm_run_open_memory_range", "cm_verify_memory_range", "cm_verify_memory_range_host", "cm_mem_range_plan"]


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def _header_fields(struct):
    m = re.search(r"typedef struct \{([^{}]*?)\} %s;\s*/\* sizeof = (\d+) \*/" % struct, HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ty, names = re.match(r"(\w+)\s+(.*)$", decl, re.S).groups()
            assert ty == "uint32_t"
            for nm in names.split(","):
                name, arr = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm).groups()
                fields.append((name, 4 * int(arr or 1)))
    return fields, int(m.group(2))


def _mirror_matches(cls, struct, names, size):
    fields, stated = _header_fields(struct)
    assert [f[0] for f in cls._fields_] == [f[0] for f in fields] == names
    off = 0
    for (name, cty), (_, nbytes) in zip(cls._fields_, fields):
        assert C.sizeof(cty) == nbytes and getattr(cls, name).offset == off, name
        off += nbytes
    assert C.sizeof(cls) == off == stated == size


def test_ctypes_mirrors_match_the_header():
    _mirror_matches(MemRangeOpening, "cm_mem_range_opening", ["start", "n_cells", "left", "right"], 232)
    _mirror_matches(MemRangeStep, "cm_mem_range_step", ["depth", "lo", "hi", "kernel", "uses_left", "uses_right"], 24)
    words = list(range(1, 59))
    assert MemRangeOpening.from_words(words).words() == words


def test_device_calls_without_a_device_are_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the host verifier and the plan
    still answer"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, MemRangeOpening, verify_range_host, mem_range_plan
L = load_library()
root, ok, o = C.c_uint32(0), C.c_uint8(0), MemRangeOpening(5, 1)
v = (C.c_uint32 * 4)()
rcs = [L.cm_input_open_memory_range(None, C.c_uint32(0), C.c_uint32(0), C.c_uint32(1), None, None, C.byref(root)),
       L.cm_run_open_memory_range(None, C.c_uint32(0), C.c_uint32(1), None, None, C.byref(root)),
       L.cm_verify_memory_range(C.c_uint32(0), C.byref(o), v, C.byref(ok), C.c_uint64(0))]
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
print(*rcs, verify_range_host(1, o, np.zeros(4, dtype=np.uint32))[0], len(mem_range_plan(5, 1)), buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    a, b, c, host, steps, msg = p.stdout.strip().split(" ", 5)
    assert (int(a), int(b), int(c)) == (3, 3, 3) and "no HIP device" in msg, p.stdout
    assert int(host) == 11 and int(steps) == 29                                  # verdicts, not a missing device


def test_host_verifier_refuses_null_arguments():
    L = load_library()
    o, v = MemRangeOpening(5, 1), (C.c_uint32 * 4)()
    for opening, values in ((None, v), (C.byref(o), None), (None, None)):
        assert L.cm_verify_memory_range_host(C.c_uint32(0), opening, values) == 1
        buf = C.create_string_buffer(256)
        L.cm_last_error(buf, C.c_size_t(256))
        assert b"null" in buf.value
