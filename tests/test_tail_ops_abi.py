"""Host side of the tail's op-level entry points (cm_tail_grind_op, cm_tail_tables_op, cm_tail_tab_words, cm_tail_last_op): the
symbols, the ctypes mirrors against the header's structs, and every refusal — each comes back as status 1 with the entry's own
message, before any device call.  CPU only: the calls run in a child process that sees no GPU, so an argument set that slipped
through the checks would end as a device-initialisation status (2 or 3), never as a launch on made-up handles."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import TailPiece, TailTablesOut, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_tail_grind_op", "cm_tail_tables_op", "cm_tail_last_op"]


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    getattr(L, "cm_tail_tab_words")
    assert re.search(r"uint64_t\s+cm_tail_tab_words\(", HDR)
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive
    note = HDR[:HDR.index("#define CM_ABI_REVISION")]
    for name in NEW + ["cm_tail_tab_words", "cm_tail_piece", "cm_tail_tables_out"]:
        assert name in note, name


def test_ctypes_mirrors_match_the_header():
    m = re.search(r"typedef struct cm_tail_piece \{(.*?)\} cm_tail_piece;", HDR, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == "uint32_t kind, k, width, reserved; const cm_handle* cols;"
    assert [f[0] for f in TailPiece._fields_] == ["kind", "k", "width", "reserved", "cols"]
    assert [getattr(TailPiece, f[0]).offset for f in TailPiece._fields_] == [0, 4, 8, 12, 16] and C.sizeof(TailPiece) == 24
    m = re.search(r"typedef struct cm_tail_tables_out \{(.*?)\} cm_tail_tables_out;", HDR, re.S)
    names = re.findall(r"(\w+)[;,]", m.group(1))
    assert names == [f[0] for f in TailTablesOut._fields_] == ["struct_size", "reserved", "hdr", "positions", "tab", "offsets", "words",
                                                               "words_cap"]
    assert [getattr(TailTablesOut, n).offset for n in names] == [0, 4, 8, 16, 24, 32, 40, 48] and C.sizeof(TailTablesOut) == 56


def test_tab_words_is_the_documented_layout():
    L = load_library()
    L.cm_tail_tab_words.restype = C.c_uint64
    for nq_pad in (1, 64, 1024):
        assert L.cm_tail_tab_words(C.c_uint32(nq_pad)) == 3 * 32 + 32 * nq_pad * 6


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, TailPiece, TailTablesOut
L = load_library()
u32p = C.POINTER(C.c_uint32)
dig = (C.c_uint32 * 8)(*range(8))
FAKE = 0x1000          # a non-null handle: never dereferenced, every case below is refused before the first device call
res = {}

def note(name, rc):
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    res[name] = [rc, buf.value.decode(errors="replace")]

# ---- cm_tail_grind_op
nonce = C.c_uint64(0)
note("grind_null_digest", L.cm_tail_grind_op(None, C.c_uint32(4), C.byref(nonce), C.c_uint64(0)))
note("grind_null_out", L.cm_tail_grind_op(dig, C.c_uint32(4), None, C.c_uint64(0)))
note("grind_bits_27", L.cm_tail_grind_op(dig, C.c_uint32(27), C.byref(nonce), C.c_uint64(0)))

# ---- cm_tail_tables_op
bufs = [np.zeros(n, dtype=np.uint32) for n in (16, 1024, 3 * 32 + 32 * 1024 * 6, 8, 1 << 16)]
def tables(digest=dig, nq=8, nq_pad=8, L0=4, pieces=((0, 1, 1), (3, 0, 2)), n_small=1, out="ok", null_cols=None, zero_handle=None,
           words_cap=1 << 16, null_pieces=False, struct_size=None):
    arr = (TailPiece * max(len(pieces), 1))()
    keep = []
    for i, (kind, k, nh) in enumerate(pieces):
        hs = (C.c_uint64 * max(nh, 1))(*([FAKE] * max(nh, 1)))
        if zero_handle == i:
            hs[nh - 1] = 0
        keep.append(hs)
        arr[i].kind, arr[i].k, arr[i].width = kind, k, nh
        arr[i].cols = None if null_cols == i else C.cast(hs, C.POINTER(C.c_uint64))
    p = [b.ctypes.data_as(u32p) for b in bufs]
    o = TailTablesOut(C.sizeof(TailTablesOut) if struct_size is None else struct_size, 0, *p, words_cap)
    if out in ("hdr", "positions", "tab", "offsets", "words"):
        setattr(o, out, None)
    return L.cm_tail_tables_op(digest, C.c_uint64(5), C.c_uint32(nq), C.c_uint32(nq_pad), C.c_uint32(L0), C.c_uint32(0),
                               None if null_pieces else arr, C.c_uint32(len(pieces)), C.c_uint32(n_small),
                               None if out is None else C.byref(o), C.c_uint64(0))
note("tables_null_digest", tables(digest=None))
note("tables_null_out", tables(out=None))
note("tables_null_pieces", tables(null_pieces=True))
note("tables_struct_size", tables(struct_size=48))
for f in ("hdr", "positions", "tab", "offsets", "words"):
    note("tables_null_" + f, tables(out=f))
note("tables_nq_0", tables(nq=0))
note("tables_nq_1025", tables(nq=1025, nq_pad=2048))
note("tables_pad_not_pow2", tables(nq=8, nq_pad=12))
note("tables_pad_below_nq", tables(nq=9, nq_pad=8))
note("tables_pad_2048", tables(nq=8, nq_pad=2048))
note("tables_log_domain_32", tables(L0=32))
note("tables_k_above_domain", tables(pieces=((0, 5, 1), (3, 0, 2))))
note("tables_n_small_above", tables(n_small=3))
note("tables_row_before_small", tables(pieces=((3, 0, 2), (3, 0, 2)), n_small=1))
note("tables_small_after_small", tables(pieces=((0, 1, 1), (2, 1, 4)), n_small=1))
note("tables_bad_kind", tables(pieces=((4, 1, 1), (3, 0, 2))))
note("tables_f_at_k0", tables(pieces=((1, 0, 1), (3, 0, 2))))
note("tables_row_width_0", tables(pieces=((0, 1, 1), (3, 0, 0))))
note("tables_null_cols", tables(null_cols=1))
note("tables_zero_handle", tables(zero_handle=1))
note("tables_zero_coord_handle", tables(pieces=((2, 1, 4), (3, 0, 2)), zero_handle=0))
note("tables_words_cap", tables(words_cap=8 * 8 + 2 * 8 - 1))

# ---- cm_tail_last_op
last = (C.c_uint64 * 4)(FAKE, FAKE, FAKE, FAKE)
ar = np.zeros(400, dtype=np.uint32)
outs = dict(dout=(C.c_uint32 * 8)(), flag=C.c_uint32(0), last_out=(C.c_uint32 * 256)(), ar_out=(C.c_uint32 * 400)(), cell=C.c_uint64(0))
def lastop(digest=dig, last=last, log_n=3, log_keep=1, ar=ar, n_ar=12, null=None):
    o = {k: (None if k == null else (v if k in ("dout", "last_out", "ar_out") else C.byref(v))) for k, v in outs.items()}
    return L.cm_tail_last_op(digest, last, C.c_uint32(log_n), C.c_uint32(log_keep), None if ar is None else ar.ctypes.data_as(u32p),
                             C.c_uint32(n_ar), o["dout"], o["flag"], o["last_out"], o["ar_out"], o["cell"], C.c_uint64(0))
note("last_null_digest", lastop(digest=None))
note("last_null_last", lastop(last=None))
note("last_zero_handle", lastop(last=(C.c_uint64 * 4)(FAKE, FAKE, 0, FAKE)))
for k in outs:
    note("last_null_" + k, lastop(null=k))
note("last_null_ar", lastop(ar=None))
note("last_log_n_7", lastop(log_n=7, log_keep=1))
note("last_keep_above_n", lastop(log_n=2, log_keep=3))
note("last_ar_385", lastop(n_ar=385))
print(json.dumps(res))
"""


def test_every_refusal_is_status_1_with_the_entrys_message():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert len(res) == 3 + 26 + 12
    want = {"grind_bits_27": "TAIL_MAX_POW_BITS", "tables_nq_0": "n_queries", "tables_nq_1025": "n_queries",
            "tables_pad_not_pow2": "nq_pad", "tables_pad_below_nq": "nq_pad", "tables_pad_2048": "nq_pad",
            "tables_log_domain_32": "log_domain", "tables_k_above_domain": "above log_domain", "tables_n_small_above": "n_small",
            "tables_row_before_small": "row piece in front of n_small", "tables_small_after_small": "behind n_small",
            "tables_bad_kind": "kind", "tables_f_at_k0": "k >= 1", "tables_row_width_0": "width", "tables_null_cols": "column handles",
            "tables_zero_handle": "null column handle", "tables_zero_coord_handle": "null column handle", "tables_words_cap": "words_cap",
            "tables_struct_size": "struct_size", "last_zero_handle": "null column handle", "last_log_n_7": "log_n above 6",
            "last_keep_above_n": "log_keep above log_n", "last_ar_385": "384"}
    for name, (rc, msg) in res.items():
        entry = {"grind": "cm_tail_grind_op:", "tables": "cm_tail_tables_op:", "last": "cm_tail_last_op:"}[name.split("_")[0]]
        assert rc == 1 and msg.startswith(entry), (name, rc, msg)
        assert want.get(name, "null") in msg, (name, msg)
