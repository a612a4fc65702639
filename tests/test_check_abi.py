"""ABI of the PCS-free AIR check (cm_check_report, cm_check_constraints): the ctypes CheckReport and the Rust #[repr(C)] twin
mirror the header field by field, the layout is plain words, and without a GPU the entry point reports an error instead of
crashing.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
FFI = open(os.path.join(ROOT, "integration", "prover-hip", "src", "ffi.rs")).read()
CONSTS = {"CM_N_COMPONENTS": 34, "CM_N_RELATIONS": 8}
WIDTH = {"int32_t": 4, "uint32_t": 4, "uint64_t": 8, "char": 1, "cm_relations": 4 * (8 * 4 + 8 * 16 * 4)}


def header_report_fields():
    """[(name, C type, dims)] of cm_check_report"""
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*?)\} cm_check_report;", hdr, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = re.match(r"(\w+)\s+(.*)", decl, re.S).groups()
        for nm in names.split(","):
            m = re.match(r"\s*(\w+)((?:\[\w+\])*)", nm)
            dims = [CONSTS.get(d) or int(d) for d in re.findall(r"\[(\w+)\]", m.group(2))]
            out.append((m.group(1), ty, dims))
    return out


def rust_report_fields():
    body = re.search(r"pub struct cm_check_report \{(.*?)\n\}", FFI, re.S).group(1)
    return [(n, re.sub(r"\s+", "", t)) for n, t in re.findall(r"pub (\w+): ([^,\n]+),", body)]


def rust_type(ty, dims):
    base = {"int32_t": "i32", "uint32_t": "u32", "uint64_t": "u64", "char": "c_char", "cm_relations": "cm_relations"}[ty]
    names = {34: "CM_N_COMPONENTS", 8: "CM_N_RELATIONS"}
    for d in reversed(dims):
        base = f"[{base};{names.get(d, d)}]"
    return base


def test_report_layout_is_plain_words():
    fields = header_report_fields()
    off = 0
    for name, ty, dims in fields:
        w = WIDTH[ty]
        assert off % min(w, 8) == 0, (name, off)      # every field starts at its natural alignment: no implicit padding
        n = 1
        for d in dims:
            n *= d
        off += w * n
    assert off % 8 == 0
    from cairo_m_amd.lib import CheckReport
    assert C.sizeof(CheckReport) == off == 8176


def test_ctypes_report_matches_the_header():
    from cairo_m_amd.lib import CheckReport
    hdr = header_report_fields()
    cf = CheckReport._fields_
    assert [f[0] for f in cf] == [f[0] for f in hdr]
    for (name, cty), (_, ty, dims) in zip(cf, hdr):
        n = 1
        for d in dims:
            n *= d
        assert C.sizeof(cty) == WIDTH[ty] * n, name
        assert getattr(CheckReport.__bases__[0], name).offset == sum(
            C.sizeof(t) for nm, t in cf[:[f[0] for f in cf].index(name)]), name


def test_rust_report_matches_the_header():
    rs, hdr = rust_report_fields(), header_report_fields()
    assert [f[0] for f in rs] == [f[0] for f in hdr]
    for (rn, rt), (_, ty, dims) in zip(rs, hdr):
        assert rt == rust_type(ty, dims), (rn, rt)
    assert "#[repr(C)]\n#[derive(Clone, Copy)]\npub struct cm_check_report" in FFI


def test_check_without_gpu_reports_an_error():
    """in a child process that sees no GPU: cm_check_constraints returns non-zero with a message, and does not crash"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library, CheckReport, synth_fibonacci
L = load_library()
inp = synth_fibonacci(5, lib=L)
dev = C.c_void_p()
rc = L.cm_input_upload(inp.view, C.byref(dev))
if rc == 0:
    rep = CheckReport()
    rc = L.cm_check_constraints(dev, None, C.byref(rep))
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
print(rc, buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rc, _, msg = p.stdout.strip().partition(" ")
    assert int(rc) != 0 and msg


def test_null_arguments_are_refused():
    from cairo_m_amd.lib import load_library, CheckReport
    L = load_library()
    rep = CheckReport()
    assert L.cm_check_constraints(None, None, C.byref(rep)) != 0
    buf = C.create_string_buffer(256)
    L.cm_last_error(buf, C.c_size_t(256))
    assert b"null" in buf.value
