"""Host side of the op-level entries of shard_ops.hip (cm_fri_fold_rows_op, cm_fri_fold_leaves_rows_op,
cm_accumulate_quotients_rows_op, cm_pack_parity_op, cm_halo_build_op, cm_sum_copies_op, cm_copy_segments_op): the symbols, the
header's constants against the Python and Rust mirrors, and every refusal — each comes back as status 1 with the entry's own
message, before any device call.  CPU only: the calls run in a child process that sees no GPU, so an argument set that slipped
through the checks would end as a device-initialisation status, never as a launch on made-up handles.  The twiddle handle is a
host struct whose first word is R, the only thing the checks read of it: the child builds one of its own."""
import json
import os
import re
import subprocess
import sys

from cairo_m_amd.lib import FOLD_ACCUMULATE, FOLD_ALPHA_ON_DEVICE, FOLD_CIRCLE, QUOT_PATHS, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "cairom_hip.h")).read()
FFI = open(os.path.join(ROOT, "integration", "prover-hip", "src", "ffi.rs")).read()
ENTRIES = ["cm_fri_fold_rows_op", "cm_fri_fold_leaves_rows_op", "cm_accumulate_quotients_rows_op", "cm_pack_parity_op",
           "cm_halo_build_op", "cm_sum_copies_op", "cm_copy_segments_op"]


def test_the_symbols_are_exported_and_declared():
    L = load_library()
    note = HDR[:HDR.index("#define CM_ABI_REVISION")]
    for name in ENTRIES:
        getattr(L, name)
        assert re.search(r"int32_t\s+%s\(" % name, HDR), name
        assert re.search(r"pub fn %s\(" % name, FFI), name
        assert name in note, name
    assert int(re.search(r"#define CM_ABI_REVISION (\d+)", HDR).group(1)) == 10      # additive


def test_constants_match_the_header_and_the_rust_mirror():
    def hdr(name):
        return int(re.search(r"#define %s (\d+)u" % name, HDR).group(1))

    def ffi(name):
        return int(re.search(r"pub const %s: u32 = (\d+);" % name, FFI).group(1))
    want = {"CM_FOLD_CIRCLE": FOLD_CIRCLE, "CM_FOLD_ACCUMULATE": FOLD_ACCUMULATE, "CM_FOLD_ALPHA_ON_DEVICE": FOLD_ALPHA_ON_DEVICE}
    for word, name in QUOT_PATHS.items():
        want["CM_QUOT_PATH_" + name.upper().replace("-", "_")] = word
    assert len(want) == 9 and sorted(QUOT_PATHS) == [1, 2, 3, 4, 5, 6]
    for name, value in want.items():
        assert hdr(name) == value and ffi(name) == value, name


CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from cairo_m_amd.lib import load_library, SampleBatches
L = load_library()
u32p = C.POINTER(C.c_uint32)
P = 2**31 - 1
FAKE = 0x1000          # a non-null handle: never dereferenced, every case below is refused before the first device call
R = 12
tw_host = (C.c_uint64 * 8)(R)        # cm::Twiddles: uint32 R, then table pointers the checks never follow
TW = C.addressof(tw_host)
res = {}

def done(rc):
    buf = C.create_string_buffer(512)
    L.cm_last_error(buf, C.c_size_t(512))
    return [rc, buf.value.decode(errors="replace")]

def h4(zero=None):
    a = (C.c_uint64 * 4)(*([FAKE] * 4))
    if zero is not None:
        a[zero] = 0
    return a

def w4(bad=None):
    a = np.array([1, 2, 3, 4], dtype=np.uint32)
    if bad is not None:
        a[bad] = P
    return a

def ptr(a):
    return None if a is None else a.ctypes.data_as(u32p)

def fold(out=True, src=True, alpha=True, tw=TW, zero_out=None, zero_src=None, bad_alpha=None, log_n=8, i0=0, n_out=64, flags=0):
    a = w4(bad_alpha)
    return done(L.cm_fri_fold_rows_op(h4(zero_out) if out else None, h4(zero_src) if src else None, ptr(a) if alpha else None,
                                      C.c_uint32(log_n), C.c_uint64(tw), C.c_uint32(i0), C.c_uint32(n_out), C.c_uint32(flags), C.c_uint64(0)))

res["fold.null_out"] = fold(out=False)
res["fold.null_src"] = fold(src=False)
res["fold.null_alpha"] = fold(alpha=False)
res["fold.null_tw"] = fold(tw=0)
res["fold.zero_out_handle"] = fold(zero_out=3)
res["fold.zero_src_handle"] = fold(zero_src=0)
res["fold.unknown_flag"] = fold(flags=8)
res["fold.line_accumulate"] = fold(flags=2)
res["fold.alpha_word_p"] = fold(bad_alpha=2)
res["fold.line_log_0"] = fold(log_n=0, n_out=1)
res["fold.line_log_R"] = fold(log_n=R)
res["fold.circle_log_1"] = fold(log_n=1, n_out=1, flags=1)
res["fold.circle_log_R_plus_1"] = fold(log_n=R + 1, flags=1)
res["fold.n_out_0"] = fold(n_out=0)
res["fold.range_one_past"] = fold(i0=65, n_out=64)
res["fold.range_wraps_u32"] = fold(i0=0xFFFFFFFF, n_out=2)
res["fold.circle_range_one_past"] = fold(i0=1, n_out=128, flags=1 | 2 | 4)

def leaves(line=True, circle=False, alpha=True, alpha_c=False, tw=TW, out=True, hashes=FAKE, fused=True, zero_out=None, zero_in=None,
           zero_circle=None, bad_alpha=None, bad_alpha_c=None, log_n=8, row0=0, n_rows=64):
    a, ac, f = w4(bad_alpha), w4(bad_alpha_c), C.c_uint32(7)
    return done(L.cm_fri_fold_leaves_rows_op(h4(zero_in) if line else None, h4(zero_circle) if circle else None, ptr(a) if alpha else None,
                                             ptr(ac) if alpha_c else None, C.c_uint32(log_n), C.c_uint64(tw), C.c_uint32(row0),
                                             C.c_uint32(n_rows), h4(zero_out) if out else None, C.c_uint64(hashes),
                                             C.byref(f) if fused else None, C.c_uint64(0)))

res["leaves.null_tw"] = leaves(tw=0)
res["leaves.null_out"] = leaves(out=False)
res["leaves.null_hashes"] = leaves(hashes=0)
res["leaves.null_fused"] = leaves(fused=False)
res["leaves.no_source"] = leaves(line=False, alpha=False)
res["leaves.line_without_challenge"] = leaves(alpha=False)
res["leaves.challenge_without_circle"] = leaves(alpha_c=True)
res["leaves.zero_out_handle"] = leaves(zero_out=1)
res["leaves.zero_in_handle"] = leaves(zero_in=2)
res["leaves.zero_circle_handle"] = leaves(circle=True, alpha_c=True, zero_circle=3)
res["leaves.alpha_word_p"] = leaves(bad_alpha=0)
res["leaves.alpha_circle_word_p"] = leaves(circle=True, alpha_c=True, bad_alpha_c=3)
res["leaves.log_1"] = leaves(log_n=1, n_rows=1)
res["leaves.line_log_R"] = leaves(log_n=R)
res["leaves.circle_log_R_plus_1"] = leaves(line=False, alpha=False, circle=True, alpha_c=True, log_n=R + 1)
res["leaves.n_rows_0"] = leaves(n_rows=0)
res["leaves.n_rows_not_a_power_of_two"] = leaves(n_rows=96)
res["leaves.range_one_past"] = leaves(row0=65, n_rows=64)
res["leaves.range_wraps_u32"] = leaves(row0=0xFFFFFFFF, n_rows=1)

def quot(tw=TW, cols=True, b=True, coeff=True, out=True, path=True, null_field=None, n_cols=3, n_batches=2, zero_col=None, zero_out=None,
         bad_coeff=None, off=(0, 3, 5), bad_point=None, ci=(0, 1, 2, 0, 2), dev=0, si=(0, 1, 2, 3, 4), null_si=False, n_samples=5,
         bad_value=None, log_size=6, row0=0, n_rows=0, leaf=0, null_cc=False):
    hs = (C.c_uint64 * max(n_cols, 1))(*([FAKE] * max(n_cols, 1)))
    if zero_col is not None:
        hs[zero_col] = 0
    pts = np.arange(1, 8 * max(n_batches, 1) + 1, dtype=np.uint32)
    if bad_point is not None:
        pts[bad_point] = P
    offs, cis, sis = np.array(off, dtype=np.uint32), np.array(ci, dtype=np.uint32), np.array(si, dtype=np.uint32)
    vals = np.arange(1, 4 * 8 + 1, dtype=np.uint32)
    if bad_value is not None:
        vals[bad_value] = P
    f = [pts.ctypes.data, offs.ctypes.data, cis.ctypes.data, vals.ctypes.data]
    if null_field is not None:
        f[null_field] = None
    sb = SampleBatches(n_batches, *f)
    co, p = w4(bad_coeff), C.c_uint32(0)
    cc, sums = np.zeros(4 * 8, dtype=np.uint32), np.zeros(12 * 4, dtype=np.uint32)
    return done(L.cm_accumulate_quotients_rows_op(
        C.c_uint32(log_size), hs if cols else None, C.c_uint32(n_cols), C.byref(sb) if b else None, ptr(co) if coeff else None,
        h4(zero_out) if out else None, C.c_uint64(tw), C.c_uint32(row0), C.c_uint32(n_rows), C.c_uint64(leaf), C.c_uint32(dev),
        None if null_si else ptr(sis), C.c_uint32(n_samples), C.byref(p) if path else None, None if null_cc else ptr(cc), ptr(sums), C.c_uint64(0)))

res["quot.null_tw"] = quot(tw=0)
res["quot.null_cols"] = quot(cols=False)
res["quot.null_batches"] = quot(b=False)
res["quot.null_coeff"] = quot(coeff=False)
res["quot.null_out"] = quot(out=False)
res["quot.null_path"] = quot(path=False)
for k, name in enumerate(["points", "batch_off", "col_index", "values"]):
    res["quot.null_" + name] = quot(null_field=k)
res["quot.n_cols_0"] = quot(n_cols=0)
res["quot.n_batches_0"] = quot(n_batches=0)
res["quot.zero_col_handle"] = quot(zero_col=2)
res["quot.zero_out_handle"] = quot(zero_out=0)
res["quot.coeff_word_p"] = quot(bad_coeff=1)
res["quot.batch_off_start"] = quot(off=(1, 3, 5))
res["quot.empty_batch"] = quot(off=(0, 3, 3))
res["quot.point_word_p"] = quot(bad_point=15)
res["quot.col_index_out_of_range"] = quot(ci=(0, 1, 2, 0, 3))
res["quot.device_without_sample_idx"] = quot(dev=1, null_si=True)
res["quot.device_without_coef_c_out"] = quot(dev=1, null_cc=True)
res["quot.n_samples_0"] = quot(dev=1, n_samples=0)
res["quot.sample_idx_out_of_range"] = quot(dev=1, si=(0, 1, 2, 3, 5))
res["quot.value_word_p"] = quot(bad_value=19)
res["quot.device_value_word_p"] = quot(dev=1, bad_value=19)
res["quot.log_size_0"] = quot(log_size=0)
res["quot.log_size_R_plus_1"] = quot(log_size=R + 1)
res["quot.whole_domain_with_row0"] = quot(row0=8, n_rows=0)
res["quot.range_one_past"] = quot(row0=33, n_rows=32)
res["quot.range_wraps_u32"] = quot(row0=0xFFFFFFFF, n_rows=1)
# the LEAF launch: what quotient_leaf_serves refuses.  The predicate is host code; "merkle_multi_top" is at its lower bound
assert L.cm_set_tuning(b"merkle_multi_top", C.c_int32(17)) == 0
tw20 = (C.c_uint64 * 8)(20)
TW20 = C.addressof(tw20)
res["quot.leaf_three_batches"] = quot(tw=TW20, log_size=17, leaf=FAKE, n_batches=3, off=(0, 2, 4, 5))
res["quot.leaf_below_multi_top"] = quot(tw=TW20, log_size=17, leaf=FAKE, n_rows=1 << 16)
res["quot.leaf_whole_below_multi_top"] = quot(tw=TW20, log_size=16, leaf=FAKE)
res["quot.leaf_row0_not_a_multiple"] = quot(tw=TW20, log_size=19, leaf=FAKE, row0=1 << 16, n_rows=1 << 17)
res["quot.leaf_not_a_power_of_two"] = quot(tw=TW20, log_size=19, leaf=FAKE, n_rows=3 << 16)
assert L.cm_set_tuning(b"quot_rows", C.c_int32(4)) == 0
res["quot.leaf_quot_rows_4"] = quot(tw=TW20, log_size=17, leaf=FAKE)
assert L.cm_set_tuning(b"quot_rows", C.c_int32(2)) == 0

def pack(src=FAKE, dst=FAKE, half_len=8, parity=0):
    return done(L.cm_pack_parity_op(C.c_uint64(src), C.c_uint64(dst), C.c_uint32(half_len), C.c_uint32(parity), C.c_uint64(0)))

res["pack.null_src"] = pack(src=0)
res["pack.null_dst"] = pack(dst=0)
res["pack.half_len_0"] = pack(half_len=0)
res["pack.half_len_huge"] = pack(half_len=(1 << 30) + 1)
res["pack.parity_2"] = pack(parity=2)

def halo(even=FAKE, odd=FAKE, out=FAKE, err=True, even_src=1, odd_src=3, row0=0, length=64, n=9, trace_log=8, log_ranks=2):
    e = C.c_uint32(7)
    return done(L.cm_halo_build_op(C.c_uint64(even), C.c_uint64(odd), C.c_uint32(even_src), C.c_uint32(odd_src), C.c_uint32(row0),
                                   C.c_uint32(length), C.c_uint32(n), C.c_uint32(trace_log), C.c_uint32(log_ranks), C.c_uint64(out),
                                   C.byref(e) if err else None, C.c_uint64(0)))

res["halo.null_even"] = halo(even=0)
res["halo.null_odd"] = halo(odd=0)
res["halo.null_out"] = halo(out=0)
res["halo.null_err"] = halo(err=False)
res["halo.n_1"] = halo(n=1, trace_log=1, log_ranks=1, length=1)
res["halo.n_31"] = halo(n=31, trace_log=30)
res["halo.trace_log_0"] = halo(trace_log=0)
res["halo.trace_log_above_n"] = halo(trace_log=10)
res["halo.log_ranks_0"] = halo(log_ranks=0, even_src=0, odd_src=0)
res["halo.log_ranks_n"] = halo(log_ranks=9)
res["halo.even_src_out_of_range"] = halo(even_src=4)
res["halo.odd_src_out_of_range"] = halo(odd_src=4)
res["halo.len_0"] = halo(length=0)
res["halo.range_one_past"] = halo(row0=449, length=64)
res["halo.range_wraps_u32"] = halo(row0=0xFFFFFFFF, length=1)

def sums(src=FAKE, out=FAKE, n_copies=2, stride=16, words=16, modular=1):
    return done(L.cm_sum_copies_op(C.c_uint64(src), C.c_uint32(n_copies), C.c_uint64(stride), C.c_uint64(words), C.c_uint64(out),
                                   C.c_uint32(modular), C.c_uint64(0)))

res["sum.null_in"] = sums(src=0)
res["sum.null_out"] = sums(out=0)
res["sum.n_copies_0"] = sums(n_copies=0)
res["sum.n_copies_1025"] = sums(n_copies=1025)
res["sum.words_0"] = sums(words=0)
res["sum.words_huge"] = sums(words=(1 << 30) + 1, stride=(1 << 30) + 1)
res["sum.stride_below_words"] = sums(stride=15)
res["sum.stride_huge"] = sums(stride=(1 << 30) + 1)

def copy(n_segs=2, src=True, dst=True, words=(4, 4), null_words=False, zero_src=None, zero_dst=None):
    n = max(len(words), 1)
    s, d = (C.c_uint64 * n)(*([FAKE] * n)), (C.c_uint64 * n)(*([FAKE] * n))
    if zero_src is not None:
        s[zero_src] = 0
    if zero_dst is not None:
        d[zero_dst] = 0
    w = (C.c_uint64 * n)(*words)
    return done(L.cm_copy_segments_op(s if src else None, d if dst else None, None if null_words else w, C.c_uint32(n_segs), C.c_uint64(0)))

res["copy.null_src"] = copy(src=False)
res["copy.null_dst"] = copy(dst=False)
res["copy.null_words"] = copy(null_words=True)
res["copy.too_many_segments"] = copy(n_segs=65536)
res["copy.zero_src_handle"] = copy(zero_src=1)
res["copy.zero_dst_handle"] = copy(zero_dst=0)
res["copy.segment_huge"] = copy(words=(4, (1 << 30) + 1))
print(json.dumps(res))
"""

WANT = {
    "fold.null_out": "null argument", "fold.null_src": "null argument", "fold.null_alpha": "null argument", "fold.null_tw": "null twiddles",
    "fold.zero_out_handle": "null column handle", "fold.zero_src_handle": "null column handle", "fold.unknown_flag": "unknown flag",
    "fold.line_accumulate": "only the circle fold accumulates", "fold.alpha_word_p": "challenge word", "fold.line_log_0": "log_n outside",
    "fold.line_log_R": "log_n outside", "fold.circle_log_1": "log_n outside", "fold.circle_log_R_plus_1": "log_n outside",
    "fold.n_out_0": "n_out is 0", "fold.range_one_past": "i0 + n_out beyond", "fold.range_wraps_u32": "i0 + n_out beyond",
    "fold.circle_range_one_past": "i0 + n_out beyond",
    "leaves.null_tw": "null twiddles", "leaves.null_out": "null argument", "leaves.null_hashes": "null argument",
    "leaves.null_fused": "null argument", "leaves.no_source": "neither a line nor a circle source",
    "leaves.line_without_challenge": "every source comes with its challenge", "leaves.challenge_without_circle": "every source comes with its challenge",
    "leaves.zero_out_handle": "null column handle", "leaves.zero_in_handle": "null column handle", "leaves.zero_circle_handle": "null column handle",
    "leaves.alpha_word_p": "challenge word", "leaves.alpha_circle_word_p": "challenge word", "leaves.log_1": "log_n outside",
    "leaves.line_log_R": "log_n outside", "leaves.circle_log_R_plus_1": "log_n outside", "leaves.n_rows_0": "n_rows is 0",
    "leaves.n_rows_not_a_power_of_two": "not a power of two", "leaves.range_one_past": "row0 + n_rows beyond",
    "leaves.range_wraps_u32": "row0 + n_rows beyond",
    "quot.null_tw": "null twiddles", "quot.null_cols": "null argument", "quot.null_batches": "null argument", "quot.null_coeff": "null argument",
    "quot.null_out": "null argument", "quot.null_path": "null argument", "quot.null_points": "null argument", "quot.null_batch_off": "null argument",
    "quot.null_col_index": "null argument", "quot.null_values": "null argument", "quot.n_cols_0": "n_cols is 0", "quot.n_batches_0": "n_batches is 0",
    "quot.zero_col_handle": "null column handle", "quot.zero_out_handle": "null column handle", "quot.coeff_word_p": "coefficient word",
    "quot.batch_off_start": "does not start at 0", "quot.empty_batch": "a batch with no entry", "quot.point_word_p": "point word",
    "quot.col_index_out_of_range": "column index out of range", "quot.device_without_sample_idx": "device_coeffs without",
    "quot.device_without_coef_c_out": "device_coeffs without", "quot.n_samples_0": "n_samples is 0",
    "quot.sample_idx_out_of_range": "sample index out of range", "quot.value_word_p": "sampled-value word",
    "quot.device_value_word_p": "sampled-value word", "quot.log_size_0": "log_size outside", "quot.log_size_R_plus_1": "log_size outside",
    "quot.whole_domain_with_row0": "with a row0", "quot.range_one_past": "row0 + n_rows beyond", "quot.range_wraps_u32": "row0 + n_rows beyond",
    "quot.leaf_three_batches": "does not serve", "quot.leaf_below_multi_top": "does not serve", "quot.leaf_whole_below_multi_top": "does not serve",
    "quot.leaf_row0_not_a_multiple": "does not serve", "quot.leaf_not_a_power_of_two": "does not serve", "quot.leaf_quot_rows_4": "does not serve",
    "pack.null_src": "null column handle", "pack.null_dst": "null column handle", "pack.half_len_0": "half_len is 0",
    "pack.half_len_huge": "above 2^30", "pack.parity_2": "neither 0 nor 1",
    "halo.null_even": "null column handle", "halo.null_odd": "null column handle", "halo.null_out": "null column handle",
    "halo.null_err": "null argument", "halo.n_1": "n outside", "halo.n_31": "n outside", "halo.trace_log_0": "trace_log outside",
    "halo.trace_log_above_n": "trace_log outside", "halo.log_ranks_0": "log_ranks outside", "halo.log_ranks_n": "log_ranks outside",
    "halo.even_src_out_of_range": "source rank", "halo.odd_src_out_of_range": "source rank", "halo.len_0": "len is 0",
    "halo.range_one_past": "row0 + len beyond", "halo.range_wraps_u32": "row0 + len beyond",
    "sum.null_in": "null column handle", "sum.null_out": "null column handle", "sum.n_copies_0": "n_copies is 0",
    "sum.n_copies_1025": "more than 1024 copies", "sum.words_0": "words is 0", "sum.words_huge": "words above 2^30",
    "sum.stride_below_words": "stride below words", "sum.stride_huge": "stride below words",
    "copy.null_src": "null argument", "copy.null_dst": "null argument", "copy.null_words": "null argument",
    "copy.too_many_segments": "more than 65535 segments", "copy.zero_src_handle": "null column handle",
    "copy.zero_dst_handle": "null column handle", "copy.segment_huge": "above 2^30 words",
}
PREFIX = {"fold": "cm_fri_fold_rows_op:", "leaves": "cm_fri_fold_leaves_rows_op:", "quot": "cm_accumulate_quotients_rows_op:",
          "pack": "cm_pack_parity_op:", "halo": "cm_halo_build_op:", "sum": "cm_sum_copies_op:", "copy": "cm_copy_segments_op:"}


def test_every_refusal_is_status_1_with_the_entrys_message():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert sorted(res) == sorted(WANT)
    for name, text in WANT.items():
        rc, msg = res[name]
        assert rc == 1 and msg.startswith(PREFIX[name.split(".")[0]]) and text in msg, (name, rc, msg)
