"""ABI of the memory accounting (cm_mem_stats, cm_proof_mem, cm_mem_estimate): the ctypes mirrors and the Rust #[repr(C)] twins
follow the header field by field with no implicit padding, the counters read zero in a process that sees no GPU, the budget
round-trips, and a proof rebuilt from words reports no memory.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
FFI = open(os.path.join(ROOT, "integration", "prover-hip", "src", "ffi.rs")).read()
WIDTH = {"uint32_t": 4, "uint64_t": 8}
STRUCTS = {"cm_mem_stats": ("MemStats", 72), "cm_proof_mem": ("ProofMem", 8 + 5 * 8 + 32 * 8), "cm_mem_estimate": ("MemEstimate", 32)}


def header_fields(name):
    """[(field, C type, array length or 1)] of a typedef struct of the header"""
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*?)\} %s;" % name, hdr, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = re.match(r"(\w+)\s+(.*)", decl, re.S).groups()
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", nm)
            out.append((m.group(1), ty, int(m.group(2) or 1)))
    return out


@pytest.mark.parametrize("name", sorted(STRUCTS))
def test_ctypes_and_rust_structs_match_the_header(name):
    import cairo_m_amd.lib as lib
    cls = getattr(lib, STRUCTS[name][0])
    hdr = header_fields(name)
    assert hdr[0][0] == "struct_size" and hdr[0][1] == "uint32_t"
    off = 0
    for (fname, ty, n), (cname, cty) in zip(hdr, cls._fields_):
        assert fname == cname
        assert off % WIDTH[ty] == 0, (name, fname, off)          # natural alignment everywhere: no implicit padding
        assert getattr(cls, cname).offset == off and C.sizeof(cty) == WIDTH[ty] * n, (name, fname)
        off += WIDTH[ty] * n
    assert len(hdr) == len(cls._fields_) and off % 8 == 0
    assert C.sizeof(cls) == off == STRUCTS[name][1]
    body = re.search(r"pub struct %s \{(.*?)\n\}" % name, FFI, re.S).group(1)
    rs = [(n, re.sub(r"\s+", "", t)) for n, t in re.findall(r"pub (\w+): ([^,\n]+),", body)]
    assert [f[0] for f in rs] == [f[0] for f in hdr]
    for (rn, rt), (_, ty, n) in zip(rs, hdr):
        want = {"uint32_t": "u32", "uint64_t": "u64"}[ty]
        assert rt == (want if n == 1 else f"[{want};{n}]"), (name, rn, rt)
    assert "#[repr(C)]\n#[derive(Clone, Copy)]\npub struct %s" % name in FFI


def test_abi_revision_names_the_memory_calls():
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) >= 9


def test_budget_round_trips_through_the_stats():
    from cairo_m_amd.lib import load_library, mem_stats, set_memory_budget
    L = load_library()
    assert mem_stats(L).budget_bytes == 0
    try:
        set_memory_budget(123456789012, L)
        assert mem_stats(L).budget_bytes == 123456789012
    finally:
        set_memory_budget(0, L)
    assert mem_stats(L).budget_bytes == 0
    L.cm_mem_reset_peak()
    assert L.cm_mem_stats_get(None) == 1


def test_stats_work_without_a_gpu_and_report_zeros():
    """in a child process that sees no GPU, before cm_init: every counter is zero; CM_MEMORY_BUDGET gives the initial budget"""
    code = r"""
import sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library, mem_stats
L = load_library()
d = mem_stats(L).as_dict()
assert d.pop("budget_bytes") == 4096, d
assert all(v == 0 for v in d.values()), d
assert L.cm_mem_reset_peak() == 0
print("ok")
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1", CM_MEMORY_BUDGET="4096")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", p.stderr


def test_a_proof_rebuilt_from_words_reports_no_memory():
    import numpy as np
    from cairo_m_amd.lib import Proof, load_library, synth_fibonacci
    from tests.oracle_binding import Oracle
    L = load_library()
    inp = synth_fibonacci(5, lib=L)
    words, _ = Oracle(os.path.join(ROOT, "oracle", "liboracle.so")).prove(inp.view)     # the CPU oracle's proof of the same input
    words = np.ascontiguousarray(words.astype(np.uint32))
    h = C.c_void_p()
    assert L.cm_proof_from_words(words.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint64(words.size), C.byref(h)) == 0
    pr = Proof(L, h)
    m = pr.memory()
    assert (m.n_phases, m.peak_live_bytes, m.start_live_bytes, m.driver_allocs, m.input_bytes) == (0, 0, 0, 0, 0)
    st = pr.stats()
    assert set(st) >= {"cells", "steps", "phase_ms", "memory"} and st["memory"]["peak_live_bytes"] == 0
    pr.free()
    inp.free()
