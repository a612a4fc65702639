"""Host side of cm_eval_at_points_op: the symbol, the ctypes mirror against the header's struct, and every refusal — each comes
back as status 1 with the entry's own message, before any device call.  CPU only: the calls run in a child process that sees no
GPU, so an argument set that slipped through the checks would end as a device-initialisation status, never as a launch on
made-up handles."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import EVAL_GUARD, EVAL_GUARD_WORDS, EVAL_MAX_JOBS, EvalJob, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()


def test_the_symbol_is_exported_and_declared():
    getattr(load_library(), "cm_eval_at_points_op")
    assert re.search(r"int32_t\s+cm_eval_at_points_op\(", HDR)
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive
    note = HDR[:HDR.index("#define CM_ABI_REVISION")]
    assert "cm_eval_at_points_op" in note and "cm_eval_job" in note


def test_ctypes_mirror_and_constants_match_the_header():
    m = re.search(r"typedef struct cm_eval_job \{(.*?)\} cm_eval_job;", HDR, re.S)
    assert re.sub(r"\s+", " ", m.group(1)).strip() == ("uint32_t log_n, n_cols; const cm_handle* coeffs; uint32_t point[8]; "
                                                        "uint32_t has_shift, shift_x, shift_y, reserved;")
    names = [f[0] for f in EvalJob._fields_]
    assert names == ["log_n", "n_cols", "coeffs", "point", "has_shift", "shift_x", "shift_y", "reserved"]
    assert [getattr(EvalJob, n).offset for n in names] == [0, 4, 8, 16, 48, 52, 56, 60] and C.sizeof(EvalJob) == 64
    m = re.search(r"enum \{ CM_EVAL_MAX_JOBS = (\d+), CM_EVAL_GUARD_WORDS = (\d+) \};\s*#define CM_EVAL_GUARD (0x[0-9A-Fa-f]+)u", HDR)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3), 16)) == (EVAL_MAX_JOBS, EVAL_GUARD_WORDS, EVAL_GUARD)
    assert EVAL_GUARD >= 2**31 - 1 and EVAL_GUARD_WORDS % 4 == 0       # no M31 word; slices stay 16-byte aligned


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, EvalJob
L = load_library()
u32p = C.POINTER(C.c_uint32)
P = 2**31 - 1
FAKE = 0x1000          # a non-null handle: never dereferenced, every case below is refused before the first device call
res = {}
out = np.zeros(4096, dtype=np.uint32)
land = np.zeros(4096, dtype=np.uint32)
t_ok = np.zeros(4, dtype=np.uint32)

def call(n_jobs=2, null_jobs=False, null_out=False, landing=0, null_landing=True, t=None, n_cols=2, log_n=5, null_coeffs=None,
         zero_handle=None, shift=(0, 0), has_shift=0, point_word=None, bad=1):
    arr = (EvalJob * max(n_jobs, 1))()
    keep = []
    for i in range(min(n_jobs, len(arr))):
        worse = i == bad                      # the second job carries the fault: the checks walk every job
        nc = n_cols if worse else 2
        hs = (C.c_uint64 * max(nc, 1))(*([FAKE] * max(nc, 1)))
        if worse and zero_handle is not None:
            hs[zero_handle] = 0
        keep.append(hs)
        arr[i].log_n, arr[i].n_cols = (log_n if worse else 5), nc
        arr[i].coeffs = None if (worse and null_coeffs) else C.cast(hs, C.POINTER(C.c_uint64))
        if worse:
            arr[i].has_shift, arr[i].shift_x, arr[i].shift_y = has_shift, shift[0], shift[1]
            if point_word is not None:
                arr[i].point[point_word] = P
    rc = L.cm_eval_at_points_op(None if null_jobs else arr, C.c_uint32(n_jobs), None if t is None else t.ctypes.data_as(u32p),
                                C.c_uint32(landing), None if null_out else out.ctypes.data_as(u32p),
                                None if null_landing else land.ctypes.data_as(u32p), C.c_uint64(0))
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return [rc, buf.value.decode(errors="replace")]

res["null_jobs"] = call(null_jobs=True)
res["null_out"] = call(null_out=True)
res["null_landing"] = call(landing=1, null_landing=True)
res["null_coeffs"] = call(null_coeffs=True)
res["zero_handle_first"] = call(zero_handle=0)
res["zero_handle_last"] = call(n_cols=3, zero_handle=2)
res["n_jobs_0"] = call(n_jobs=0)
res["n_jobs_65"] = call(n_jobs=65)
res["n_cols_0"] = call(n_cols=0)
res["n_cols_65537"] = call(n_cols=65537)
res["log_n_27"] = call(log_n=27)
res["log_n_32"] = call(log_n=32)
res["shift_x_p"] = call(shift=(P, 0), has_shift=1, t=t_ok)
res["shift_y_p"] = call(shift=(0, P), has_shift=1, t=t_ok)
res["shift_y_max_unused"] = call(shift=(0, 0xFFFFFFFF), has_shift=0)
res["felt_word_p"] = call(t=np.array([0, 0, P, 0], dtype=np.uint32))
res["point_word_p"] = call(point_word=7)
res["fault_in_job_64_of_64"] = call(n_jobs=64, n_cols=0, bad=63)
print(json.dumps(res))
"""


def test_every_refusal_is_status_1_with_the_entrys_message():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    want = {"null_jobs": "null argument", "null_out": "null argument", "null_landing": "null argument",
            "null_coeffs": "without column handles", "zero_handle_first": "null column handle", "zero_handle_last": "null column handle",
            "n_jobs_0": "n_jobs is 0", "n_jobs_65": "more than 64 jobs", "n_cols_0": "n_cols 0", "n_cols_65537": "65536",
            "log_n_27": "log_n above 26", "log_n_32": "log_n above 26", "shift_x_p": "shift word", "shift_y_p": "shift word",
            "shift_y_max_unused": "shift word", "felt_word_p": "felt word", "point_word_p": "point word",
            "fault_in_job_64_of_64": "n_cols 0"}
    assert sorted(res) == sorted(want)
    for name, text in want.items():
        rc, msg = res[name]
        assert rc == 1 and msg.startswith("cm_eval_at_points_op:") and text in msg, (name, rc, msg)
