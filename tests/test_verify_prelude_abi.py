"""Host side of the verifier prelude on the GPU (CM_VERIFY_ARITH_ON_DEVICE, cm_verify_many_ex and its siblings, the two op-level
entries and their host twins): symbols, the ctypes mirrors against the header's structs, the revision note, and every refusal —
status 1 with the entry's own message, before any device call.  CPU only: the calls run in a child process that sees no GPU, so an
argument set that slipped through the checks would end as status 3 (no device), never as a launch on made-up buffers."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import (RELATIONS_WORDS, VERIFY_ARITH_ON_DEVICE, VERIFY_PUBLIC_SUM_ENTRIES, PointEvalJobC, PublicSumJobC,
                             load_library)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
NEW = ["cm_verify_many_ex", "cm_verify_many_detail_ex", "cm_verify_run_device_ex", "cm_public_logup_sum_op", "cm_public_logup_sum_host",
       "cm_point_eval_op", "cm_point_eval_host"]


def test_symbols_are_exported_and_declared():
    L = load_library()
    for name in NEW:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name


def test_revision_is_still_10_and_the_note_names_the_additions():
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10
    note = HDR[:HDR.index("#define CM_ABI_REVISION")]
    last = note[note.rindex("Still 10"):]
    assert "additive" in last
    for name in NEW + ["CM_VERIFY_ARITH_ON_DEVICE", "cm_public_sum_job", "cm_point_eval_job"]:
        assert name in last, name


def test_constants_match_lib_py():
    assert int(re.search(r"#define CM_VERIFY_ARITH_ON_DEVICE\s+(\d+)u", HDR).group(1)) == VERIFY_ARITH_ON_DEVICE == 1
    assert int(re.search(r"#define CM_PUBLIC_SUM_ENTRIES (\d+)u", HDR).group(1)) == VERIFY_PUBLIC_SUM_ENTRIES
    assert re.search(r"#define CM_RELATIONS_WORDS \(4u \* CM_N_RELATIONS \* \(1u \+ CM_MAX_RELATION_SIZE\)\)", HDR)
    n_rel = int(re.search(r"#define CM_N_RELATIONS (\d+)", HDR).group(1))
    max_size = int(re.search(r"#define CM_MAX_RELATION_SIZE (\d+)", HDR).group(1))
    assert 4 * n_rel * (1 + max_size) == RELATIONS_WORDS == 544


def _body(name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HDR, re.S)
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)).strip()


def test_ctypes_mirrors_match_the_header():
    assert _body("cm_public_sum_job") == ("uint32_t head[7]; uint32_t n_program, n_input, n_output; const uint32_t* entries; "
                                          "const uint32_t* rel_words;")
    names = [f[0] for f in PublicSumJobC._fields_]
    assert names == ["head", "n_program", "n_input", "n_output", "entries", "rel_words"]
    assert [getattr(PublicSumJobC, n).offset for n in names] == [0, 28, 32, 36, 40, 48] and C.sizeof(PublicSumJobC) == 56
    assert _body("cm_point_eval_job") == ("uint32_t component, n_tr_words, n_it_words, n_coeff_words; "
                                          "const uint32_t *tr, *it, *pp, *rel_words, *coeff; uint32_t shift[4];")
    names = [f[0] for f in PointEvalJobC._fields_]
    assert names == ["component", "n_tr_words", "n_it_words", "n_coeff_words", "tr", "it", "pp", "rel_words", "coeff", "shift"]
    assert [getattr(PointEvalJobC, n).offset for n in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56] and C.sizeof(PointEvalJobC) == 72


CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import (PointEvalJobC, PublicSumJobC, VerifyResultC, load_library, point_eval_job, public_sum_job, synth_fibonacci)
from tests.oracle_binding import Oracle
from tests.verify_many_util import proof_from_words
from tests.verify_prelude_ref import component_counts, entries, random_rel
L = load_library()
P = 2**31 - 1
res = {}
out = (C.c_uint32 * 64)()

def err(rc):
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return [rc, buf.value.decode(errors="replace")]

# ---- the verifier entries: flags, and no device
inp = synth_fibonacci(5)
words, _ = Oracle(os.path.join(sys.argv[1], "oracle", "liboracle.so")).prove(inp.view)
p = proof_from_words(L, words)
assert p.verify() == (0, "")
hs = (C.c_void_p * 1)(p.h.value)
r1 = (VerifyResultC * 1)()
first = (C.c_uint32 * 2)()
for flags in (0, 1):
    res["many_ex_flags_%d" % flags] = err(L.cm_verify_many_ex(hs, C.c_uint32(1), None, C.c_uint32(flags), r1, C.c_uint64(0)))
    res["detail_ex_flags_%d" % flags] = err(L.cm_verify_many_detail_ex(hs, C.c_uint32(1), None, C.c_uint32(flags), r1, None, C.c_uint32(0),
                                                                          first, C.c_uint64(0)))
    res["run_ex_flags_%d" % flags] = err(L.cm_verify_run_device_ex(hs, C.c_uint32(1), None, C.c_uint32(flags)))
for flags in (2, 3, 0x80000000):
    res["many_ex_unknown_%x" % flags] = err(L.cm_verify_many_ex(hs, C.c_uint32(1), None, C.c_uint32(flags), r1, C.c_uint64(0)))
    res["detail_ex_unknown_%x" % flags] = err(L.cm_verify_many_detail_ex(hs, C.c_uint32(1), None, C.c_uint32(flags), r1, None, C.c_uint32(0),
                                                                            first, C.c_uint64(0)))
    res["run_ex_unknown_%x" % flags] = err(L.cm_verify_run_device_ex(hs, C.c_uint32(1), None, C.c_uint32(flags)))
res["many_ex_no_proofs"] = err(L.cm_verify_many_ex(None, C.c_uint32(0), None, C.c_uint32(1), None, C.c_uint64(0)))

# ---- cm_public_logup_sum_op / _host
rng = np.random.default_rng(5)
def sum_call(host=False, null_jobs=False, null_out=False, n_jobs=2, **bad):
    jobs = []
    for i in range(2):
        worse = i == 1                      # the second job carries the fault: the checks walk every job
        head = [1, 2, 3, 4, 5, 6, 7]
        lists = [entries(rng, 3), entries(rng, 2), entries(rng, 4)]
        rel = random_rel(rng)
        if worse:
            if "head_word" in bad: head[bad["head_word"]] = P
            if "entry_word" in bad: lists[bad["list"]][bad["row"], bad["entry_word"]] = bad.get("value", P)
            if "rel_word" in bad: rel[bad["rel_word"]] = P
        j = public_sum_job(head, lists[0], lists[1], lists[2], rel)
        if worse:
            if bad.get("null_entries"): j[0].entries = None
            if bad.get("null_rel"): j[0].rel_words = None
            if "n_program" in bad: j[0].n_program = bad["n_program"]
        jobs.append(j)
    arr = (PublicSumJobC * 2)(jobs[0][0], jobs[1][0])
    if host:
        return err(L.cm_public_logup_sum_host(None if null_jobs else C.byref(arr[1]), None if null_out else out))
    return err(L.cm_public_logup_sum_op(None if null_jobs else arr, C.c_uint32(n_jobs), C.c_uint64(0), None if null_out else out))

for host in (False, True):
    tag = "sum_host_" if host else "sum_op_"
    res[tag + "null_jobs"] = sum_call(host, null_jobs=True)
    res[tag + "null_out"] = sum_call(host, null_out=True)
    res[tag + "null_entries"] = sum_call(host, null_entries=True)
    res[tag + "null_rel"] = sum_call(host, null_rel=True)
    res[tag + "head_word_p"] = sum_call(host, head_word=6)
    res[tag + "addr_p"] = sum_call(host, list=0, row=0, entry_word=1)
    res[tag + "value_p"] = sum_call(host, list=1, row=1, entry_word=5)
    res[tag + "clock_max"] = sum_call(host, list=2, row=3, entry_word=6, value=0xFFFFFFFF)
    res[tag + "present_2"] = sum_call(host, list=2, row=0, entry_word=0, value=2)
    res[tag + "rel_word_p"] = sum_call(host, rel_word=543)
    res[tag + "list_too_long"] = sum_call(host, n_program=(1 << 24) + 1)
res["sum_op_n_jobs_0"] = sum_call(n_jobs=0)
res["sum_op_n_jobs_65537"] = sum_call(n_jobs=65537)
res["sum_op_valid_no_device"] = sum_call()
res["sum_host_valid"] = sum_call(host=True)

# ---- cm_point_eval_op / _host
def eval_call(host=False, null_jobs=False, null_out=False, n_jobs=2, cid=3, **bad):
    jobs = []
    for i in range(2):
        worse = i == 1
        c = cid if worse else 0
        n_tr, n_it, n_co = component_counts(L, min(c, 33))
        arrs = [rng.integers(0, P, size=n, dtype=np.uint32) for n in (n_tr, n_it, 28, 544, n_co)]
        shift = [1, 2, 3, 4]
        if worse:
            if "word" in bad: arrs[bad["array"]][bad["word"]] = P
            if "shift_word" in bad: shift[bad["shift_word"]] = P
        j = point_eval_job(min(c, 33), *arrs, shift)
        if worse:
            j[0].component = c
            for name in ("tr", "it", "pp", "rel_words", "coeff"):
                if bad.get("null") == name: setattr(j[0], name, None)
            for name in ("n_tr_words", "n_it_words", "n_coeff_words"):
                if name in bad: setattr(j[0], name, getattr(j[0], name) + bad[name])
        jobs.append(j)
    arr = (PointEvalJobC * 2)(jobs[0][0], jobs[1][0])
    if host:
        return err(L.cm_point_eval_host(None if null_jobs else C.byref(arr[1]), None if null_out else out))
    return err(L.cm_point_eval_op(None if null_jobs else arr, C.c_uint32(n_jobs), C.c_uint64(0), None if null_out else out))

for host in (False, True):
    tag = "eval_host_" if host else "eval_op_"
    res[tag + "null_jobs"] = eval_call(host, null_jobs=True)
    res[tag + "null_out"] = eval_call(host, null_out=True)
    for name in ("tr", "it", "pp", "rel_words", "coeff"):
        res[tag + "null_" + name] = eval_call(host, null=name)
    res[tag + "component_34"] = eval_call(host, cid=34)
    res[tag + "component_max"] = eval_call(host, cid=0xFFFFFFFF)
    res[tag + "tr_short"] = eval_call(host, n_tr_words=-4)
    res[tag + "tr_long"] = eval_call(host, n_tr_words=4)
    res[tag + "it_short"] = eval_call(host, n_it_words=-4)
    res[tag + "it_long"] = eval_call(host, n_it_words=1)
    res[tag + "coeff_short"] = eval_call(host, n_coeff_words=-4)
    res[tag + "coeff_long"] = eval_call(host, n_coeff_words=4)
    for k, name in enumerate(("tr", "it", "pp", "rel", "coeff")):
        res[tag + name + "_word_p"] = eval_call(host, array=k, word=3)
    res[tag + "shift_word_p"] = eval_call(host, shift_word=2)
res["eval_op_n_jobs_0"] = eval_call(n_jobs=0)
res["eval_op_n_jobs_65537"] = eval_call(n_jobs=65537)
res["eval_op_valid_no_device"] = eval_call()
res["eval_host_valid"] = eval_call(host=True)
print(json.dumps(res))
"""


def _child():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    return json.loads(p.stdout.strip().splitlines()[-1])


_RES = {}


def _results():
    if not _RES:
        _RES.update(_child())
    return _RES


def test_flags_unknown_bits_are_status_1_and_no_device_is_status_3():
    res = _results()
    for entry in ("many_ex", "detail_ex", "run_ex"):
        for flags in (0, 1):
            rc, msg = res["%s_flags_%d" % (entry, flags)]
            assert rc == 3 and "no HIP device" in msg, (entry, flags, rc, msg)
        for flags in ("2", "3", "80000000"):
            rc, msg = res["%s_unknown_%s" % (entry, flags)]
            assert rc == 1 and "unknown flag bit" in msg, (entry, flags, rc, msg)
    assert res["many_ex_no_proofs"][0] == 1


def _check(res, tag, who, want):
    seen = {k[len(tag):] for k in res if k.startswith(tag)}
    assert seen == set(want) | {"valid_no_device" if tag.endswith("_op_") else "valid"}, sorted(seen ^ set(want))
    for name, text in want.items():
        rc, msg = res[tag + name]
        assert rc == 1 and msg.startswith(who + ":") and text in msg, (tag + name, rc, msg)


def test_every_refusal_of_the_public_sum_entries():
    res = _results()
    want = {"null_jobs": "null argument", "null_out": "null argument", "null_entries": "without entries", "null_rel": "without rel_words",
            "head_word_p": "head word", "addr_p": "entry word", "value_p": "entry word", "clock_max": "entry word",
            "present_2": "present word", "rel_word_p": "relation word", "list_too_long": "2^24"}
    _check(res, "sum_host_", "cm_public_logup_sum_host", want)
    _check(res, "sum_op_", "cm_public_logup_sum_op", dict(want, n_jobs_0="n_jobs outside", n_jobs_65537="n_jobs outside"))
    rc, msg = res["sum_op_valid_no_device"]
    assert rc == 3 and "no HIP device" in msg          # a valid call gets as far as the device, and only a valid one
    assert res["sum_host_valid"][0] == 0


def test_every_refusal_of_the_point_eval_entries():
    res = _results()
    want = {"null_jobs": "null argument", "null_out": "null argument", "component_34": "component id", "component_max": "component id",
            "tr_short": "n_tr_words", "tr_long": "n_tr_words", "it_short": "n_it_words", "it_long": "n_it_words",
            "coeff_short": "n_coeff_words", "coeff_long": "n_coeff_words", "tr_word_p": "mask word", "it_word_p": "mask word",
            "pp_word_p": "mask word", "rel_word_p": "relation word", "coeff_word_p": "coefficient word", "shift_word_p": "shift word"}
    want.update({"null_" + n: "null argument" for n in ("tr", "it", "pp", "rel_words", "coeff")})
    _check(res, "eval_host_", "cm_point_eval_host", want)
    _check(res, "eval_op_", "cm_point_eval_op", dict(want, n_jobs_0="n_jobs outside", n_jobs_65537="n_jobs outside"))
    rc, msg = res["eval_op_valid_no_device"]
    assert rc == 3 and "no HIP device" in msg
    assert res["eval_host_valid"][0] == 0
