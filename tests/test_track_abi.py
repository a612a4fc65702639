"""ABI of the relation tracker (cm_relation_entry, cm_track_relations, cm_relation_entries): the ctypes RelationEntry and the Rust
#[repr(C)] twin mirror the header field by field, the layout is plain words, cm_check_report keeps its size, NULL arguments are
refused, and without a GPU both entry points report an error instead of crashing.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
FFI = open(os.path.join(ROOT, "integration", "prover-hip", "src", "ffi.rs")).read()
CONSTS = {"CM_MAX_RELATION_SIZE": 16}
WIDTH = {"uint32_t": 4, "uint64_t": 8}


def header_entry_fields():
    """[(name, C type, dims)] of cm_relation_entry"""
    hdr = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
    body = re.search(r"typedef struct \{([^{}]*?)\} cm_relation_entry;", hdr, re.S).group(1)
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


def count(dims):
    n = 1
    for d in dims:
        n *= d
    return n


def test_entry_layout_is_plain_words():
    off = 0
    for name, ty, dims in header_entry_fields():
        assert off % WIDTH[ty] == 0, (name, off)      # every field starts at its natural alignment: no implicit padding
        off += WIDTH[ty] * count(dims)
    assert off % 8 == 0
    from cairo_m_amd.lib import CheckReport, RelationEntry
    assert C.sizeof(RelationEntry) == off == 96
    assert C.sizeof(CheckReport) == 8176


def test_ctypes_entry_matches_the_header():
    from cairo_m_amd.lib import RelationEntry
    hdr = header_entry_fields()
    cf = RelationEntry._fields_
    assert [f[0] for f in cf] == [f[0] for f in hdr]
    off = 0
    for (name, cty), (_, ty, dims) in zip(cf, hdr):
        assert C.sizeof(cty) == WIDTH[ty] * count(dims), name
        assert getattr(RelationEntry, name).offset == off, name
        off += C.sizeof(cty)


def test_rust_entry_matches_the_header():
    body = re.search(r"pub struct cm_relation_entry \{(.*?)\n\}", FFI, re.S).group(1)
    rs = [(n, re.sub(r"\s+", "", t)) for n, t in re.findall(r"pub (\w+): ([^,\n]+),", body)]
    hdr = header_entry_fields()
    assert [f[0] for f in rs] == [f[0] for f in hdr]
    for (rn, rt), (_, ty, dims) in zip(rs, hdr):
        want = {"uint32_t": "u32", "uint64_t": "u64"}[ty]
        for d in reversed(dims):
            want = f"[{want};{ {16: 'CM_MAX_RELATION_SIZE'}.get(d, d) }]"
        assert rt == want, (rn, rt)
    assert "#[repr(C)]\n#[derive(Clone, Copy)]\npub struct cm_relation_entry" in FFI


def test_abi_revision_names_the_tracker():
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) >= 8


def last_error(L):
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return buf.value


def test_null_arguments_are_refused():
    from cairo_m_amd.lib import load_library, RelationEntry
    L = load_library()
    n = C.c_uint64(0)
    buf = (RelationEntry * 4)()
    assert L.cm_track_relations(None, None, C.c_uint32(0), None, buf, C.c_uint64(4), C.byref(n)) != 0
    assert b"null" in last_error(L)
    rel = (C.c_uint32 * (4 * (8 + 8 * 16)))()
    cols = (C.c_uint64 * 512)()
    assert L.cm_relation_entries(C.c_int32(0), cols, cols, C.c_uint32(4), None, C.c_uint32(0), buf, C.c_uint64(4), C.byref(n), C.c_uint64(0)) != 0
    assert b"null" in last_error(L)
    assert L.cm_relation_entries(C.c_int32(0), cols, cols, C.c_uint32(4), rel, C.c_uint32(0), buf, C.c_uint64(4), None, C.c_uint64(0)) != 0
    assert b"null" in last_error(L)
    assert L.cm_relation_entries(C.c_int32(0), cols, cols, C.c_uint32(4), rel, C.c_uint32(0), None, C.c_uint64(4), C.byref(n), C.c_uint64(0)) != 0
    assert b"null" in last_error(L)
    assert L.cm_relation_entries(C.c_int32(0), cols, cols, C.c_uint32(4), rel, C.c_uint32(0x100), buf, C.c_uint64(4), C.byref(n), C.c_uint64(0)) != 0
    assert b"relation_mask" in last_error(L)


def test_tracker_without_gpu_reports_an_error():
    """in a child process that sees no GPU: both entry points return non-zero with a message, and do not crash"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library, CheckReport, RelationEntry, synth_fibonacci
L = load_library()
def err():
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return buf.value.decode().replace("\n", " ")
inp = synth_fibonacci(5, lib=L)
dev = C.c_void_p()
buf = (RelationEntry * 4)()
n = C.c_uint64(0)
rc = L.cm_input_upload(inp.view, C.byref(dev))
if rc == 0:
    rep = CheckReport()
    rc = L.cm_track_relations(dev, None, C.c_uint32(0), C.byref(rep), buf, C.c_uint64(4), C.byref(n))
print(rc, err())
rel = (C.c_uint32 * (4 * (8 + 8 * 16)))(*([1] * (4 * (8 + 8 * 16))))
cols = (C.c_uint64 * 512)(*([4096] * 512))
rc = L.cm_relation_entries(C.c_int32(0), cols, cols, C.c_uint32(4), rel, C.c_uint32(0), buf, C.c_uint64(4), C.byref(n), C.c_uint64(0))
print(rc, err())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 2
    for ln in lines:
        rc, _, msg = ln.partition(" ")
        assert int(rc) != 0 and msg
