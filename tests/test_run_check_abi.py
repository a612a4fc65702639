"""Host side of the whole-run check (cm_link_diff, cm_check_chain, cm_check_run): the symbols, the ctypes mirrors against the
header's structs, the no-GPU status, and the rule the link diff is built on — on the host adapter's own rows and roots, the
numpy reference lists a cell exactly when the two roots of a link differ.  CPU only."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

from cairo_m_amd.lib import (CheckReport, LinkCell, LinkReport, RunCheckC, load_library, prover_input_arrays, synth_fibonacci,
                             synth_fibonacci_segment, vm_run, vm_segment)
from tests.link_diff_ref import link_diff_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_link_diff", "cm_check_chain", "cm_check_run"]
WIDTH = {"uint32_t": 4, "uint64_t": 8, "char": 1, "cm_check_report": 8176, "cm_link_report": 240}


def test_new_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive: new symbols and structs only


def header_struct(name):
    """([(field, bytes)], sizeof the header states in the comment behind the struct) of a struct of plain words"""
    m = re.search(r"typedef struct \{([^{}]*?)\} %s;\s*/\* sizeof = (?:[^*]*= )?(\d+) \*/" % name, HDR, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        ty, names = re.match(r"(\w+)\s+(.*)", decl, re.S).groups()
        for nm in names.split(","):
            f = re.match(r"\s*(\w+)(?:\[(\d+)\])?", nm)
            fields.append((f.group(1), WIDTH[ty] * int(f.group(2) or 1), min(WIDTH[ty], 8)))
    return fields, int(m.group(2))


@pytest.mark.parametrize("name,cls", [("cm_link_cell", LinkCell), ("cm_link_report", LinkReport), ("cm_run_check", RunCheckC)])
def test_ctypes_mirrors_match_the_header(name, cls):
    fields, stated = header_struct(name)
    assert [f[0] for f in cls._fields_] == [f[0] for f in fields]
    off = 0
    owner = next(k for k in cls.__mro__ if "_fields_" in vars(k))     # (LinkReport overrides `message` with a str property)
    for (fname, cty), (_, size, align) in zip(cls._fields_, fields):
        assert off % align == 0, (fname, off)                     # plain words: no implicit padding
        assert C.sizeof(cty) == size and getattr(owner, fname).offset == off, fname
        off += size
    assert C.sizeof(cls) == off == stated
    assert C.sizeof(CheckReport) == WIDTH["cm_check_report"]


def test_struct_sizes():
    assert (C.sizeof(LinkCell), C.sizeof(LinkReport), C.sizeof(RunCheckC)) == (44, 240, 8432)


def test_link_diff_without_a_device_is_status_3():
    """in a child process that sees no GPU: cm_init's status, before any argument is looked at; cm_check_chain likewise"""
    code = r"""
import ctypes as C, sys
sys.path.insert(0, sys.argv[1])
from cairo_m_amd.lib import load_library, LinkReport
L = load_library()
rep = LinkReport()
rep.struct_size = C.sizeof(LinkReport)
n = C.c_uint64(0)
rc = L.cm_link_diff(None, None, C.byref(rep), None, C.c_uint64(0), C.byref(n))
buf = C.create_string_buffer(512)
L.cm_last_error(buf, C.c_size_t(512))
print(rc, L.cm_check_chain(None, C.c_uint32(0), None, None, C.c_uint64(0)), buf.value.decode())
"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", code, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    rc, rc_chain, msg = p.stdout.strip().split(" ", 2)
    assert (int(rc), int(rc_chain)) == (3, 3) and "no HIP device" in msg, p.stdout


def test_check_run_refuses_null_arguments():
    L = load_library()
    assert L.cm_check_run(None, None, C.c_uint32(0), None, None, None, C.c_uint64(0)) == 1
    buf = C.create_string_buffer(256)
    L.cm_last_error(buf, C.c_size_t(256))
    assert b"null" in buf.value


# ---- the rule: a cell is listed <=> it changes the root --------------------------------------------------------------------
def _cuts():
    """name -> (host adapter input of segment s, runner segment s, max_steps, segments)"""
    from tests.test_gpu_adapter import scatter_store_program
    from tests.test_gpu_run import _cut, _runs
    runs = _runs()
    small = scatter_store_program(300)
    fib_steps = 10 * 200 + 12

    def vm(prog):
        return (lambda s, ms: vm_run(prog, max_steps=ms, segment=s)), (lambda s, ms: vm_segment(prog, max_steps=ms, segment=s))
    return {
        "fibonacci4": ((lambda s, ms: synth_fibonacci(200, max_steps=ms, segment=s)),
                       (lambda s, ms: synth_fibonacci_segment(200, max_steps=ms, segment=s)), -(-fib_steps // 4), 4),
        "chain": runs["chain"],
        "high": runs["high"],
        "scatter300": vm(small) + (_cut(small, 3), 3),
    }


CUT_NAMES = ["fibonacci4", "chain", "high", "scatter300"]
BROKEN = {"scatter300"}     # every link: each segment first-writes cells beyond the memory it was handed
ZERO_ONLY = {"high"}        # the case that decides the rule: a link with cells present on one side only, all zero, and EQUAL roots


@pytest.mark.parametrize("name", CUT_NAMES)
def test_reference_lists_a_cell_exactly_when_the_roots_differ(name):
    mk_input, mk_segment, max_steps, n = _cuts()[name]
    first = mk_segment(0, max_steps)
    assert (getattr(first, "n_segments", None) or n) == n
    first.free()
    arrays = []
    for s in range(n):
        hi = mk_input(s, max_steps)
        arrays.append(prover_input_arrays(hi.view))
        hi.free()
    broken = zero_only_with_equal_roots = 0
    for i in range(1, n):
        prev, nxt = arrays[i - 1], arrays[i]
        cells, totals = link_diff_ref(prev["final_memory"], nxt["initial_memory"])
        roots_equal = prev["roots"][1] == nxt["roots"][0]
        print(name, "link", i, "roots_equal", roots_equal, "cells", len(cells), totals)
        assert roots_equal == (len(cells) == 0), (name, i, totals)
        assert len(cells) == totals["n_changed"] + totals["n_only_next"] + totals["n_only_prev"]
        broken += not roots_equal
        zero_only_with_equal_roots += roots_equal and totals["n_zero_only"] > 0
    assert broken == ((n - 1) if name in BROKEN else 0), (name, broken)
    assert not (name in ZERO_ONLY) or zero_only_with_equal_roots > 0, name
