"""Host side of the set openings (cm_mem_set_plan, cm_input_open_memory_set, cm_run_open_memory_set, cm_verify_memory_set,
cm_memory_set_root_host, cm_verify_memory_set_host): the symbols, the ctypes mirror against the header's struct, the no-GPU status
of the three device calls, and the refusal of NULL arguments.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import MemSetStep, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_mem_set_plan", "cm_input_open_memory_set", "cm_run_open_memory_set", "cm_verify_memory_set", "cm_memory_set_root_host",
       "cm_verify_memory_set_host"]


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_ctypes_mirror_matches_the_header():
    m = re.search(r"typedef struct \{([^{}]*?)\} cm_mem_set_step;\s*/\* sizeof = (\d+) \*/", HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.match(r"uint32_t\s+(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in MemSetStep._fields_] == ["depth", "n_nodes", "n_siblings", "kernel"]
    assert [getattr(MemSetStep, f).offset for f in fields] == [0, 4, 8, 12]
    assert C.sizeof(MemSetStep) == int(m.group(2)) == 16


def test_device_calls_without_a_device_are_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; the plan and the host calls
    still answer"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, MemSetOpening, verify_set_host, mem_set_plan
L = load_library()
root, ok, need = C.c_uint32(0), C.c_uint8(0), C.c_uint32(0)
a, v, s = (C.c_uint32 * 1)(5), (C.c_uint32 * 4)(), (C.c_uint32 * 28)()
rcs = [L.cm_input_open_memory_set(None, C.c_uint32(0), a, C.c_uint64(1), v, s, C.c_uint32(28), C.byref(need), C.byref(root)),
       L.cm_run_open_memory_set(None, a, C.c_uint64(1), v, s, C.c_uint32(28), C.byref(need), C.byref(root)),
       L.cm_verify_memory_set(C.c_uint32(0), a, C.c_uint64(1), v, s, C.c_uint32(28), C.byref(ok), None, C.c_uint64(0))]
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
o = MemSetOpening([5], np.zeros((1, 4), dtype=np.uint32), np.zeros(28, dtype=np.uint32))
got = C.c_uint32(0)
host_root = L.cm_memory_set_root_host(a, C.c_uint64(1), v, s, C.c_uint32(28), C.byref(got))
print(*rcs, verify_set_host(1, o)[0], host_root, len(mem_set_plan([5])[0]), mem_set_plan([5])[1], buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    a, b, c, host, host_root, steps, words, msg = p.stdout.strip().split(" ", 7)
    assert (int(a), int(b), int(c)) == (3, 3, 3) and "no HIP device" in msg, p.stdout
    assert int(host) == 11 and int(host_root) == 0 and int(steps) == 29 and int(words) == 28   # verdicts, not a missing device


def test_host_calls_refuse_null_arguments():
    L = load_library()
    a, v, s, got, k, m = (C.c_uint32 * 1)(5), (C.c_uint32 * 4)(), (C.c_uint32 * 28)(), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    steps = (MemSetStep * 29)()

    def refused(rc):
        buf = C.create_string_buffer(256)
        L.cm_last_error(buf, C.c_size_t(256))
        return rc == 1 and b"null" in buf.value

    for aa, vv, ss in ((None, v, s), (a, None, s), (a, v, None)):
        assert refused(L.cm_verify_memory_set_host(C.c_uint32(0), aa, C.c_uint64(1), vv, ss, C.c_uint32(28)))
        assert refused(L.cm_memory_set_root_host(aa, C.c_uint64(1), vv, ss, C.c_uint32(28), C.byref(got)))
    assert refused(L.cm_memory_set_root_host(a, C.c_uint64(1), v, s, C.c_uint32(28), None))
    for args in ((None, C.c_uint64(1), steps, C.c_uint32(29), C.byref(k), C.byref(m)), (a, C.c_uint64(1), None, C.c_uint32(29), C.byref(k), C.byref(m)),
                 (a, C.c_uint64(1), steps, C.c_uint32(29), None, C.byref(m)), (a, C.c_uint64(1), steps, C.c_uint32(29), C.byref(k), None)):
        assert refused(L.cm_mem_set_plan(*args))
    assert L.cm_mem_set_plan(a, C.c_uint64(1), steps, C.c_uint32(28), C.byref(k), C.byref(m)) == 1       # cap < 29
    assert L.cm_mem_set_plan(a, C.c_uint64(1), steps, C.c_uint32(29), C.byref(k), C.byref(m)) == 0 and (k.value, m.value) == (29, 28)
