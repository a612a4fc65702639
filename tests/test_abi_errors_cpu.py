"""The error contract of the C-ABI boundary on paths host code alone reaches (no GPU): a failing call returns its status and
leaves its message for cm_last_error(), one failing path per family of entry points (abi.hpp's guard, host_api.hip, capi.hip,
api_prove.hip, api_run.hip, api_proof.hip, api_verify.hip, api_air_ops.hip, the memory family, program_id.hip); a call that succeeds after
a failing one returns 0; the error string belongs to the calling thread."""
import ctypes as C
import threading

import pytest

from cairo_m_amd.lib import load_library


@pytest.fixture(scope="module")
def L():
    return load_library()


def last_error(L):
    buf = C.create_string_buffer(4096)
    L.cm_last_error(buf, C.c_size_t(len(buf)))
    return buf.value.decode()


u32, u64, i32 = C.c_uint32, C.c_uint64, C.c_int32


def synth_fibonacci_past_the_end(L):
    out = C.c_void_p()
    return L.cm_synth_fibonacci(u32(5), u64(1 << 20), u32(7), C.byref(out))


def host_segment_end_lengths_null(L):
    a, b = u64(), u64()
    return L.cm_host_segment_end_lengths(None, C.byref(a), C.byref(b))


def vm_run_invalid_opcode(L):
    out = C.c_void_p()
    return L.cm_vm_run((u32 * 1)(999), (u32 * 1)(1), u32(1), u32(0), None, u32(0), u32(0), u64(10), u32(0), C.byref(out), None)


def segment_from_artifacts_bad_length(L):
    out = C.c_void_p()
    return L.cm_segment_from_artifacts(None, u64(7), None, u64(0), i32(0), None, u64(0), None, C.byref(out))


def adapt_segment_host_null(L):
    return L.cm_adapt_segment_host(None, None)


def fft_plan_log_out_of_range(L):
    out, n = ((u32 * 4) * 8)(), u32()
    return L.cm_fft_plan(u32(29), out, C.byref(n))


def merkle_plan_capacity_too_small(L):
    logs, rec, n = (u32 * 3)(12, 12, 10), ((u32 * 26) * 1)(), u32()
    return L.cm_merkle_plan(logs, u32(3), rec, u32(0), C.byref(n))


def shard_plan_world_3(L):
    owner, words = (i32 * 64)(), u64()
    return L.cm_shard_plan(None, None, u32(3), owner, C.byref(words))


def estimate_memory_null(L):
    return L.cm_estimate_memory(None, None, u32(1), None)


def set_tuning_out_of_range(L):
    return L.cm_set_tuning(b"oods_split", i32(1001))


def set_framing_malformed(L):
    return L.cm_set_framing(b"no_such_switch=1")


def component_info_bad_id(L):
    return L.cm_component_info(i32(-1), None, None, None)


def tail_list_bad_domain(L):
    n = u32()
    return L.cm_tail_list(None, u32(0), u32(40), u32(0), u32(0), u32(0), None, u32(0), C.byref(n))


def prove_run_null(L):
    return L.cm_prove_run(None, None, u32(0), None, u32(1), None)


def prove_run_transitions_null(L):
    return L.cm_prove_run_transitions(None, None, u32(0), None, u32(1), None, None)


def run_begin_null_output(L):
    return L.cm_run_begin(None, u64(0), None, u64(0), None, None)


def check_run_null(L):
    return L.cm_check_run(None, None, u32(0), None, None, None, u64(0))


def proof_public_data_null(L):
    return L.cm_proof_public_data(None, None)


def proof_from_words_bad_magic(L):
    out = C.c_void_p()
    return L.cm_proof_from_words(None, u64(0), C.byref(out))


def verify_run_no_proofs(L):
    return L.cm_verify_run(None, u32(0), None)


def verify_many_detail_null_slot_first(L):
    return L.cm_verify_many_detail(None, u32(1), None, None, None, u32(0), None, u64(0))


def mem_batch_plan_null_part(L):
    ptrs, ns, steps, k = (C.POINTER(u32) * 1)(), (u32 * 1)(3), (u32 * (4 * 29))(), u32()
    return L.cm_mem_batch_plan(ptrs, ns, u32(1), steps, u32(29), C.byref(k))


def program_id_absent_entry(L):
    entries, got = (u32 * 14)(1, 0, 1, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0), u32()
    return L.cm_program_id_entries(entries, u64(2), C.byref(got))


def program_id_no_entries(L):
    entries, got = (u32 * 7)(), u32()
    return L.cm_program_id_entries(entries, u64(0), C.byref(got))


FAILING = [
    (synth_fibonacci_past_the_end, 1, "segment index out of range"),
    (host_segment_end_lengths_null, 1, "cm_host_segment_end_lengths: null argument"),
    (vm_run_invalid_opcode, 1, "vm: invalid opcode 999"),
    (segment_from_artifacts_bad_length, 1, "trace file: length is not a multiple of 8 bytes (fp, pc)"),
    (adapt_segment_host_null, 1, "cm_adapt_segment_host: null argument"),
    (fft_plan_log_out_of_range, 1, "cm_fft_plan: log size out of range (1..28)"),
    (merkle_plan_capacity_too_small, 1, "cm_merkle_plan: output buffer too small"),
    (shard_plan_world_3, 1, "cm_shard_plan: world must be 1, 2, 4 or 8"),
    (estimate_memory_null, 1, "cm_estimate_memory: null argument"),
    (set_tuning_out_of_range, 1, "cm_set_tuning: value out of the key's range"),
    (set_framing_malformed, 1, "framing: unknown switch 'no_such_switch' (mix_u64, hash_node, sample_batch, pcs_mix)"),
    (component_info_bad_id, 1, "bad component id"),
    (tail_list_bad_domain, 1, "cm_tail_list: bad arguments"),
    (prove_run_null, 1, "cm_prove_run: null argument"),
    (prove_run_transitions_null, 1, "cm_prove_run_transitions: null argument"),
    (run_begin_null_output, 1, "cm_run_begin: null output"),
    (check_run_null, 1, "cm_check_run: null argument"),
    (proof_public_data_null, 1, "cm_proof_public_data: null argument"),
    (proof_from_words_bad_magic, 11, "cm_proof_from_words: not a proof word stream (bad magic)"),
    (verify_run_no_proofs, 1, "cm_verify_run: no proofs"),
    (verify_many_detail_null_slot_first, 1, "cm_verify_many_detail: null output"),
    (mem_batch_plan_null_part, 1, "cm_mem_batch_plan: part 0: null array"),
    (program_id_absent_entry, 1, "cm_program_id_entries: entry 1 (address 1) is absent"),
    (program_id_no_entries, 1, "cm_program_id_entries: no entries: a program of no cells has no id"),
]


@pytest.mark.parametrize("call,status,message", FAILING, ids=[f[0].__name__ for f in FAILING])
def test_failing_path_reports_status_and_message(L, call, status, message):
    assert call(L) == status
    assert last_error(L) == message


def test_prove_many_of_nothing_succeeds(L):
    assert L.cm_prove_many(None, u32(0), None, u32(1), None) == 0


def test_success_after_failure_returns_zero(L):
    assert fft_plan_log_out_of_range(L) == 1
    out, n = ((u32 * 4) * 8)(), u32()
    assert L.cm_fft_plan(u32(10), out, C.byref(n)) == 0 and n.value >= 1
    assert component_info_bad_id(L) == 1
    cols = u32()
    assert L.cm_component_info(i32(0), C.byref(cols), None, None) == 0 and cols.value >= 1
    assert synth_fibonacci_past_the_end(L) == 1
    assert L.cm_prove_many(None, u32(0), None, u32(1), None) == 0


def test_error_string_is_per_thread(L):
    """two threads fail in different entry points at the same time; each reads back its own message, and a thread that never failed
    reads an empty one"""
    calls = [(shard_plan_world_3, "cm_shard_plan: world must be 1, 2, 4 or 8"), (component_info_bad_id, "bad component id")]
    both_failed = threading.Barrier(len(calls))
    seen = [None] * len(calls)

    def work(k):
        rc = calls[k][0](L)
        both_failed.wait(timeout=30)
        seen[k] = (rc, last_error(L))

    threads = [threading.Thread(target=work, args=(k,)) for k in range(len(calls))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert seen == [(1, calls[0][1]), (1, calls[1][1])]
    fresh = []
    t = threading.Thread(target=lambda: fresh.append(last_error(L)))
    t.start()
    t.join()
    assert fresh == [""]
