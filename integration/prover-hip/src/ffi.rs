//! Raw bindings of include/cairom_hip.h — EVERY exported function (tests/test_rust_shim.py fails on a header function without
//! an extern twin of the same arity; tools/gen_ffi_rs.py prints the block from the header).  Layouts are `#[repr(C)]` mirrors
//! of the C structs; every function returns a status (0 = OK) and leaves a message for `cm_last_error`.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_void};

pub type cm_handle = u64;
pub type cm_stream_t = u64;

pub const CM_N_OPCODE_COMPONENTS: usize = 26;

#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_bundle {
    pub pc: u32,
    pub fp: u32,
    pub clock: u32,
    pub inst_prev_clock: u32,
    pub inst: [u32; 6],
    pub span_start: u32,
    pub span_len: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_data_access {
    pub address: u32,
    pub prev_clock: u32,
    pub prev_value: u32,
    pub value: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_memory_cell {
    pub address: u32,
    pub value: [u32; 4],
    pub clock: u32,
    pub multiplicity: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_clock_update {
    pub address: u32,
    pub prev_clock: u32,
    pub value: [u32; 4],
}
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_merkle_node {
    pub index: u32,
    pub depth: u32,
    pub left_value: u32,
    pub right_value: u32,
    pub parent_value: u32,
    pub left_mult: u32,
    pub right_mult: u32,
    pub parent_mult: u32,
}
#[repr(C)]
pub struct cm_prover_input {
    pub initial_pc: u32,
    pub initial_fp: u32,
    pub final_pc: u32,
    pub final_fp: u32,
    pub bundles: [*const cm_bundle; CM_N_OPCODE_COMPONENTS],
    pub n_bundles: [u64; CM_N_OPCODE_COMPONENTS],
    pub data_accesses: *const cm_data_access,
    pub n_data_accesses: u64,
    pub initial_memory: *const cm_memory_cell,
    pub n_initial_memory: u64,
    pub final_memory: *const cm_memory_cell,
    pub n_final_memory: u64,
    pub clock_updates: *const cm_clock_update,
    pub n_clock_updates: u64,
    pub initial_tree: *const cm_merkle_node,
    pub n_initial_tree: u64,
    pub final_tree: *const cm_merkle_node,
    pub n_final_tree: u64,
    pub initial_root: u32,
    pub final_root: u32,
    pub program_range: [u32; 2],
    pub input_range: [u32; 2],
    pub output_range: [u32; 2],
}
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_pcs_config {
    pub pow_bits: u32,
    pub log_blowup_factor: u32,
    pub log_last_layer_degree_bound: u32,
    pub n_queries: u32,
}
#[repr(C)]
pub struct cm_proof {
    _private: [u8; 0],
}
#[repr(C)]
pub struct cm_device_input {
    _private: [u8; 0],
}
#[repr(C)]
pub struct cm_host_input {
    _private: [u8; 0],
}
#[repr(C)]
pub struct cm_host_segment {
    _private: [u8; 0],
}
/// Stwo `ColumnSampleBatch`es of one size group, flattened (QuotientOps::accumulate_quotients)
#[repr(C)]
pub struct cm_sample_batches {
    pub n_batches: u32,
    pub points: *const u32,
    pub batch_off: *const u32,
    pub col_index: *const u32,
    pub values: *const u32,
}
pub const CM_N_COMPONENTS: usize = 34;
pub const CM_N_RELATIONS: usize = 8;
pub const CM_MAX_RELATION_SIZE: usize = 16;
pub const CM_N_PREPROCESSED: usize = 7;
/// `Relations::draw` (components/mod.rs:311-323): z and alpha^0.. of every relation, QM31 as 4 words
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_relations {
    pub z: [[u32; 4]; CM_N_RELATIONS],
    pub alpha_pow: [[[u32; 4]; CM_MAX_RELATION_SIZE]; CM_N_RELATIONS],
}
/// Verdict of `cm_check_constraints` (the PCS-free AIR check, `debug_tools::assert_constraints`): status 0 ok, 1 a lookup value
/// out of range, 2 a constraint fails, 3 the LogUp sums do not cancel.  Plain words only (no implicit padding).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_check_report {
    pub status: i32,
    pub component: i32,
    pub constraint: i32,
    pub reserved: i32,
    pub row: u64,
    pub failing_rows: [u64; CM_N_COMPONENTS],
    pub first_constraint: [i32; CM_N_COMPONENTS],
    pub first_row: [u64; CM_N_COMPONENTS],
    pub claimed_sum: [[u32; 4]; CM_N_COMPONENTS],
    pub relation_sum: [[[u32; 4]; CM_N_RELATIONS]; CM_N_COMPONENTS],
    pub public_sum: [[u32; 4]; CM_N_RELATIONS],
    pub total: [u32; 4],
    pub relations: cm_relations,
    pub message: [c_char; 256],
}
/// Process-wide device-memory counters over all thread pools (`cm_mem_stats_get`); `struct_size` = `size_of::<cm_mem_stats>()`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_stats {
    pub struct_size: u32,
    pub proofs_in_flight: u32,
    pub peak_proofs_in_flight: u32,
    pub reserved0: u32,
    pub live_bytes: u64,
    pub reserved_bytes: u64,
    pub peak_live_bytes: u64,
    pub peak_reserved_bytes: u64,
    pub pinned_host_bytes: u64,
    pub driver_allocs: u64,
    pub budget_bytes: u64,
}
/// What one proof took from the proving thread's device pool (`cm_proof_memory`); phases as `cm_proof_stats`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_proof_mem {
    pub struct_size: u32,
    pub n_phases: u32,
    pub start_live_bytes: u64,
    pub peak_live_bytes: u64,
    pub peak_reserved_bytes: u64,
    pub input_bytes: u64,
    pub driver_allocs: u64,
    pub phase_peak_live_bytes: [u64; 32],
}
/// Host-side estimate of a proof's device memory (`cm_estimate_memory`): `working_bytes` is an upper bound.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_estimate {
    pub struct_size: u32,
    pub reserved0: u32,
    pub input_bytes: u64,
    pub working_bytes: u64,
    pub cached_bytes: u64,
}
/// One tuple of the relation tracker's summary (`cm_track_relations`, `cm_relation_entries`): net multiplicity (canonical M31,
/// never 0), the lowest (component, row) merged into it (`CM_N_COMPONENTS` = public data) and the number of entries merged.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_relation_entry {
    pub relation: u32,
    pub multiplicity: u32,
    pub n_values: u32,
    pub first_component: u32,
    pub first_row: u64,
    pub n_entries: u64,
    pub values: [u32; CM_MAX_RELATION_SIZE],
}
/// One runner segment (crates/common/src/execution.rs:10-15) as plain arrays
#[repr(C)]
pub struct cm_runner_segment {
    pub trace: *const u32,
    pub n_trace: u64,
    pub memory_trace: *const u32,
    pub n_memory_trace: u64,
    pub initial_memory: *const u32,
    pub n_initial_memory: u64,
    pub program_range: [u32; 2],
    pub input_range: [u32; 2],
    pub output_range: [u32; 2],
    /// (revision 6) heap cells at segment start: index i = the cell at MAX_ADDRESS - i (runner/src/vm/mod.rs:205-221)
    pub initial_heap: *const u32,
    pub n_initial_heap: u64,
}
/// Collectives of the sharded prover (cm_prove_sharded): two blocking calls over two device staging buffers
#[repr(C)]
pub struct cm_comm {
    /// `size_of::<cm_comm>()`: the library only reads the optional fields this size covers
    pub struct_size: u32,
    pub rank: u32,
    pub world: u32,
    pub ctx: *mut c_void,
    pub send_buf: *mut u32,
    pub recv_buf: *mut u32,
    pub buf_words: u64,
    pub all_to_all_v: Option<unsafe extern "C" fn(ctx: *mut c_void, send_words: *const u64, recv_words: *const u64) -> i32>,
    pub all_gather: Option<unsafe extern "C" fn(ctx: *mut c_void, words_per_rank: u64) -> i32>,
    /// CM_COMM_STREAM_ORDERED (1): the callbacks enqueue on the stream given through `set_stream` and do not block
    pub flags: u32,
    pub set_stream: Option<unsafe extern "C" fn(ctx: *mut c_void, stream: cm_stream_t) -> i32>,
    /// called when this rank fails inside cm_prove_sharded, so that the communicator can release the peers (None: its own timeout)
    pub abort: Option<unsafe extern "C" fn(ctx: *mut c_void)>,
}
pub const CM_COMM_STREAM_ORDERED: u32 = 1;
/// u32 words of one launch record of `cm_merkle_plan`
pub const CM_MERKLE_PLAN_WORDS: usize = 26;
#[repr(C)]
pub struct cm_rccl_comm {
    _private: [u8; 0],
}
/// (revision 10) a run: the program's memory kept on the device from segment to segment
#[repr(C)]
pub struct cm_run {
    _private: [u8; 0],
}
/// One segment of a run: trace and memory log as in `cm_runner_segment`, plus the lengths of the runner's two memory vectors
/// when the segment ends
#[repr(C)]
pub struct cm_run_segment {
    pub trace: *const u32,
    pub n_trace: u64,
    pub memory_trace: *const u32,
    pub n_memory_trace: u64,
    pub n_memory_end: u64,
    pub n_heap_end: u64,
}
/// One proof's verdict from `cm_verify_many`: the host verifier's status and words, and the CM_VERIFY_* id of the failed check
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_verify_result {
    pub status: i32,
    pub check: i32,
    pub message: [c_char; 160],
}
/// The shapes of the plan `cm_verify_many` would launch for one proof (`cm_verify_plan_stats`); set `struct_size` before the call
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_verify_stats {
    pub struct_size: u32,
    pub early_check: i32,
    pub n_answer_jobs: u32,
    pub max_batch_entries: u32,
    pub max_first_pairs: u32,
    pub max_inner_pairs: u32,
    pub max_level_nodes: u32,
    pub merkle_lds_bytes: u32,
    pub n_tree_jobs: u32,
    pub n_slots: u32,
    pub blob_words: u64,
    pub scratch_words: u64,
}
/// One check of one proof as `cm_verify_many_detail` left it
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_verify_slot {
    pub check: i32,
    pub on_device: u32,
    pub raised: u32,
    pub message: [c_char; 116],
}
/// A proof's public data (public_data.rs:192-227); set `struct_size` before the call
#[repr(C)]
pub struct cm_public_data {
    pub struct_size: u32,
    pub reserved0: u32,
    pub initial_pc: u32,
    pub initial_fp: u32,
    pub final_pc: u32,
    pub final_fp: u32,
    pub clock: u32,
    pub initial_root: u32,
    pub final_root: u32,
    pub n_program: u32,
    pub n_input: u32,
    pub n_output: u32,
}
/// A memory transition as the library hands it out (`cm_input_open_transition`); read through `cm_mem_transition_get`
#[repr(C)]
pub struct cm_mem_transition {
    _private: [u8; 0],
}
/// The arrays of a `cm_mem_transition`, valid until `cm_mem_transition_free`; set `struct_size` before `cm_mem_transition_get`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cm_mem_transition_view {
    pub struct_size: u32,
    pub root_before: u32,
    pub root_after: u32,
    pub n: u32,
    pub n_siblings: u32,
    pub n_zero_only: u32,
    pub addresses: *const u32,
    pub old_values: *const u32,
    pub new_values: *const u32,
    pub siblings: *const u32,
}
/// One set of a batch (`cm_verify_memory_sets`): a transition view without the second plane; set `struct_size`
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct cm_mem_set_view {
    pub struct_size: u32,
    pub root: u32,
    pub n: u32,
    pub n_siblings: u32,
    pub addresses: *const u32,
    pub values: *const u32,
    pub siblings: *const u32,
}
/// One hashing step of a batch of sets or transitions (`cm_mem_batch_plan`): the `n_nodes` nodes of `depth` all parts produce
/// together, the most any one part has and the kernel that runs it (0 per cell, 1 per level, 2 the tail, one workgroup per part)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_batch_step {
    pub depth: u32,
    pub n_nodes: u32,
    pub widest_part: u32,
    pub kernel: u32,
}
/// A followed memory image (`cm_mem_image_create`): opaque, freed with `cm_mem_image_free`
#[repr(C)]
pub struct cm_mem_image {
    _private: [u8; 0],
}
/// What `cm_mem_image_stats_get` fills; set `struct_size` before the call
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct cm_mem_image_stats {
    pub struct_size: u32,
    pub device: u32,
    pub n_cells: u64,
    pub n_nodes: u64,
    pub bytes: u64,
}
/// One part of `cm_mem_images_apply`: an update of `n` cells to the device image `img`; a null `old_values`, `root_before` or
/// `root_after` is not compared; set `struct_size` before the call
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_image_update {
    pub struct_size: u32,
    pub n: u32,
    pub img: *mut cm_mem_image,
    pub addresses: *const u32,
    pub new_values: *const u32,
    pub old_values: *const u32,
    pub root_before: *const u32,
    pub root_after: *const u32,
}
/// What `cm_mem_images_apply` says of one part: 0 applied, 1 a bad part, 11 refused; the image's root when the call returns;
/// the single call's message, NUL-terminated ("" when applied)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_image_result {
    pub status: i32,
    pub root: u32,
    pub message: [u8; 248],
}
/// One part of `cm_mem_images_open_memory_sets`: the set of `n` cells `addresses` under the device image `img` (several parts may
/// name one image); `values` takes 4 n words, `siblings` up to `cap_siblings`; set `struct_size` before the call
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_set_request {
    pub struct_size: u32,
    pub n: u32,
    pub img: *mut cm_mem_image,
    pub addresses: *const u32,
    pub values: *mut u32,
    pub siblings: *mut u32,
    pub cap_siblings: u32,
    pub reserved: u32,
}
/// What `cm_mem_images_open_memory_sets` says of one part: 0 opened, 1 a bad part; the image's root; the words the set needs;
/// the single call's message, NUL-terminated ("" when opened)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_set_result {
    pub status: i32,
    pub root: u32,
    pub n_siblings: u32,
    pub reserved: u32,
    pub message: [u8; 240],
}
/// What a chain of proofs states (`cm_run_statement_of`): the program's id and range, the registers and memory roots the run
/// starts from and ends at, the counts of its input and output entries; set `struct_size` before the call
#[repr(C)]
#[derive(Clone, Copy, Default, Debug, PartialEq, Eq)]
pub struct cm_run_statement {
    pub struct_size: u32,
    pub n_segments: u32,
    pub program_id: u32,
    pub program_start: u32,
    pub n_program: u32,
    pub initial_pc: u32,
    pub initial_fp: u32,
    pub final_pc: u32,
    pub final_fp: u32,
    pub initial_root: u32,
    pub final_root: u32,
    pub n_input: u32,
    pub n_output: u32,
    pub reserved0: u32,
}
/// One cell that makes a link's roots differ (`cm_link_diff`): kind 1 present on both sides with different values, 2 present only
/// in the later segment's initial memory, 3 only in the earlier segment's final memory
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct cm_link_cell {
    pub kind: u32,
    pub address: u32,
    pub prev_value: [u32; 4],
    pub next_value: [u32; 4],
    pub prev_clock: u32,
}
/// Registers and roots on both sides of a link, totals per kind, the cells present on one side only with an all-zero value (not
/// listed: they do not change the root), and the message; set `struct_size` before `cm_link_diff`
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_link_report {
    pub struct_size: u32,
    pub reserved0: u32,
    pub prev_final_pc: u32,
    pub prev_final_fp: u32,
    pub next_initial_pc: u32,
    pub next_initial_fp: u32,
    pub pc_equal: u32,
    pub fp_equal: u32,
    pub roots_equal: u32,
    pub reserved1: u32,
    pub prev_final_root: u32,
    pub next_initial_root: u32,
    pub n_changed: u64,
    pub n_only_next: u64,
    pub n_only_prev: u64,
    pub n_zero_only: u64,
    pub message: [c_char; 160],
}
/// One segment's record of `cm_check_run` / `cm_check_chain`: its AIR verdict, the link to its predecessor, the cells written
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_run_check {
    pub check: cm_check_report,
    pub link: cm_link_report,
    pub link_cells_written: u64,
    pub link_cells_total: u64,
}
/// One cell's value and its authentication path under a 31-bit memory root (`cm_input_open_memory`, `cm_run_open_memory`):
/// `siblings[k]` is the sibling at depth 28 - k; an absent cell (`present` = 0) opens as the value (0, 0, 0, 0)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_opening {
    pub address: u32,
    pub present: u32,
    pub value: [u32; 4],
    pub siblings: [u32; 28],
}
pub type CmMemOpening = cm_mem_opening;
/// A contiguous run of cells under a 31-bit memory root (`cm_input_open_memory_range`, `cm_run_open_memory_range`): with
/// last = start + n_cells - 1, `left[k]` is the node of depth 28 - k left of the interval [start >> k, last >> k] when
/// start >> k is odd and `right[k]` the node right of it when last >> k is even; a slot the range does not need is 0.  The values
/// travel beside the record, four words per cell
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_range_opening {
    pub start: u32,
    pub n_cells: u32,
    pub left: [u32; 28],
    pub right: [u32; 28],
}
pub type CmMemRangeOpening = cm_mem_range_opening;
/// One hashing step of a range's verification (`cm_mem_range_plan`): the nodes `lo ..= hi` of `depth` it produces, the kernel
/// that runs it (0 per cell, 1 per level, 2 the single-workgroup tail) and which sibling words it reads
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_range_step {
    pub depth: u32,
    pub lo: u32,
    pub hi: u32,
    pub kernel: u32,
    pub uses_left: u32,
    pub uses_right: u32,
}
/// One hashing step of a set's verification (`cm_mem_set_plan`): the `n_nodes` nodes of `depth` it produces, the sibling words
/// it reads and the kernel that runs it (0 per cell, 1 per level, 2 the single-workgroup tail)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_mem_set_step {
    pub depth: u32,
    pub n_nodes: u32,
    pub n_siblings: u32,
    pub kernel: u32,
}

/// One piece of the decommitment for `cm_tail_tables_op` (test surface of the device-side proof tail).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_tail_piece {
    pub kind: u32,
    pub k: u32,
    pub width: u32,
    pub reserved: u32,
    pub cols: *const cm_handle,
}
/// Host buffers `cm_tail_tables_op` fills.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_tail_tables_out {
    pub struct_size: u32,
    pub reserved: u32,
    pub hdr: *mut u32,
    pub positions: *mut u32,
    pub tab: *mut u32,
    pub offsets: *mut u32,
    pub words: *mut u32,
    pub words_cap: u64,
}
/// One sampling group for `cm_eval_at_points_op` (test surface of the provers' out-of-domain sampling).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_eval_job {
    pub log_n: u32,
    pub n_cols: u32,
    pub coeffs: *const cm_handle,
    pub point: [u32; 8],
    pub has_shift: u32,
    pub shift_x: u32,
    pub shift_y: u32,
    pub reserved: u32,
}
/// `CM_VERIFY_ARITH_ON_DEVICE`: the public LogUp sum and the OODS check of every proof decided on the GPU (`cm_verify_many_ex`).
pub const CM_VERIFY_ARITH_ON_DEVICE: u32 = 1;
/// `cm_fri_fold_rows_op` flags.
pub const CM_FOLD_CIRCLE: u32 = 1;
pub const CM_FOLD_ACCUMULATE: u32 = 2;
pub const CM_FOLD_ALPHA_ON_DEVICE: u32 = 4;
/// The kernel family `cm_accumulate_quotients_rows_op` reports in `*path`.
pub const CM_QUOT_PATH_ROWS2: u32 = 1;
pub const CM_QUOT_PATH_ROWS4: u32 = 2;
pub const CM_QUOT_PATH_ROWS2_LEAF: u32 = 3;
pub const CM_QUOT_PATH_ONE_ROW: u32 = 4;
pub const CM_QUOT_PATH_SLICES8: u32 = 5;
pub const CM_QUOT_PATH_SLICES64: u32 = 6;
/// One public data set for `cm_public_logup_sum_op` / `cm_public_logup_sum_host` (test surface of the verifier's prelude kernels).
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_public_sum_job {
    pub head: [u32; 7],
    pub n_program: u32,
    pub n_input: u32,
    pub n_output: u32,
    pub entries: *const u32,
    pub rel_words: *const u32,
}
/// One component's mask values for `cm_point_eval_op` / `cm_point_eval_host`.
#[repr(C)]
#[derive(Clone, Copy)]
pub struct cm_point_eval_job {
    pub component: u32,
    pub n_tr_words: u32,
    pub n_it_words: u32,
    pub n_coeff_words: u32,
    pub tr: *const u32,
    pub it: *const u32,
    pub pp: *const u32,
    pub rel_words: *const u32,
    pub coeff: *const u32,
    pub shift: [u32; 4],
}
unsafe extern "C" {
    pub fn cm_init(device: i32) -> i32;
    pub fn cm_shutdown() -> i32;
    pub fn cm_pool_trim() -> i32;
    pub fn cm_device_mem_info(free_bytes: *mut u64, total_bytes: *mut u64) -> i32;
    pub fn cm_last_error(buf: *mut c_char, buf_len: usize) -> i32;
    pub fn cm_stream_create(out: *mut cm_stream_t) -> i32;
    pub fn cm_stream_destroy(s: cm_stream_t) -> i32;
    pub fn cm_stream_sync(s: cm_stream_t) -> i32;
    pub fn cm_set_cpu_affinity(mode: i32) -> i32;
    pub fn cm_get_cpu_affinity() -> i32;
    pub fn cm_set_framing(spec: *const c_char) -> i32;
    pub fn cm_get_framing(buf: *mut c_char, buf_len: usize) -> i32;
    pub fn cm_set_transcript_log(on: i32) -> i32;
    pub fn cm_col_alloc(n_u32: u64, out: *mut cm_handle) -> i32;
    pub fn cm_col_free(h: cm_handle) -> i32;
    pub fn cm_col_h2d(h: cm_handle, src: *const u32, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_col_d2h(h: cm_handle, dst: *mut u32, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_col_read(h: cm_handle, offset_u32: u64, dst: *mut u32, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_col_write(h: cm_handle, offset_u32: u64, src: *const u32, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_col_copy(dst: cm_handle, src: cm_handle, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_bit_reverse(cols: *const cm_handle, n_cols: u32, log_n: u32, s: cm_stream_t) -> i32;
    pub fn cm_twiddles_precompute(log_size: u32, tw_out: *mut cm_handle) -> i32;
    pub fn cm_twiddles_free(tw: cm_handle) -> i32;
    pub fn cm_interpolate(cols: *const cm_handle, n_cols: u32, log_n: u32, tw: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_evaluate(coeffs: *const cm_handle, n_cols: u32, log_n: u32, log_out: u32, tw: cm_handle, out: *const cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_interpolate_extend(evals: *const cm_handle, coeffs: *const cm_handle, lde: *const cm_handle, n_cols: u32, log_n: u32, tw: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_fft_plan(log_n: u32, out: *mut [u32; 4], n_passes: *mut u32) -> i32;
    pub fn cm_fft_extend_fused(log_n: u32, fused: *mut u32) -> i32;
    pub fn cm_eval_at_point(coeffs: *const cm_handle, n_cols: u32, log_n: u32, pt_xy: *const u32, out: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_merkle_commit_layer(log_size: u32, prev_layer: cm_handle, cols: *const cm_handle, n_cols: u32, out_hashes: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_merkle_commit(cols: *const cm_handle, col_logs: *const u32, n_cols: u32, root: *mut u8, s: cm_stream_t) -> i32;
    pub fn cm_merkle_commit_layers(cols: *const cm_handle, col_logs: *const u32, n_cols: u32, root: *mut u8, layers_out: *mut u32, cap_words: u64, s: cm_stream_t) -> i32;
    pub fn cm_merkle_plan(col_logs: *const u32, n_cols: u32, out: *mut [u32; CM_MERKLE_PLAN_WORDS], cap_launches: u32, n_launches: *mut u32) -> i32;
    pub fn cm_merkle_layer_npw(log_size: u32, has_prev: u32, n_cols: u32, npw: *mut u32) -> i32;
    pub fn cm_grind(digest: *const u8, pow_bits: u32, nonce_out: *mut u64, s: cm_stream_t) -> i32;
    pub fn cm_batch_inverse_m31(src: cm_handle, out: cm_handle, n: u64, s: cm_stream_t) -> i32;
    pub fn cm_batch_inverse_qm31(src: *const cm_handle, out: *const cm_handle, n: u64, s: cm_stream_t) -> i32;
    pub fn cm_fri_fold_circle_into_line(dst: *const cm_handle, src: *const cm_handle, alpha: *const u32, log_n: u32, tw: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_fri_fold_line(src: *const cm_handle, alpha: *const u32, log_n: u32, tw: cm_handle, out: *const cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_fri_fold_line_leaves(src: *const cm_handle, circle: *const cm_handle, alpha: *const u32, alpha_circle: *const u32, log_n: u32, tw: cm_handle, out: *const cm_handle, leaf_hashes: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_accumulate_quotients(log_size: u32, cols: *const cm_handle, n_cols: u32, batches: *const cm_sample_batches, random_coeff: *const u32, out: *const cm_handle, tw: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_vm_run(instr_words: *const u32, instr_lens: *const u32, n_instr: u32, entry_pc: u32, args: *const u32, n_args: u32, n_returns: u32, max_steps: u64, segment_index: u32, out: *mut *mut cm_host_input, n_segments_out: *mut u32) -> i32;
    pub fn cm_synth_fibonacci(n: u32, max_steps: u64, segment_index: u32, out: *mut *mut cm_host_input) -> i32;
    pub fn cm_host_input_view(h: *const cm_host_input) -> *const cm_prover_input;
    pub fn cm_host_input_steps(h: *const cm_host_input) -> u64;
    pub fn cm_host_input_free(h: *mut cm_host_input) -> i32;
    pub fn cm_adapter_memory_script(preload: *const u32, n_preload: u32, script: *const u32, n: u32, results: *mut u32, n_clock_updates: *mut u32, clock_updates_out: *mut u32, cu_cap: u32, query_addrs: *const u32, n_query: u32, state_out: *mut u32) -> i32;
    pub fn cm_adapter_partial_tree(cells: *const u32, n: u32, initial: i32, ranges: *const u32, nodes_out: *mut u32, cap: u64, n_nodes: *mut u64, root: *mut u32) -> i32;
    pub fn cm_poseidon2_permute(state: *mut u32) -> i32;
    pub fn cm_prove_segment(input: *const cm_prover_input, config: *const cm_pcs_config, out: *mut *mut cm_proof) -> i32;
    pub fn cm_proof_free(p: *mut cm_proof) -> i32;
    pub fn cm_input_upload(input: *const cm_prover_input, out: *mut *mut cm_device_input) -> i32;
    pub fn cm_input_free(h: *mut cm_device_input) -> i32;
    pub fn cm_prove_device(input: *const cm_device_input, config: *const cm_pcs_config, out: *mut *mut cm_proof) -> i32;
    pub fn cm_verify_proof(p: *const cm_proof, expected: *const cm_pcs_config) -> i32;
    pub fn cm_verify_proof_words(words: *const u32, n_words: u64, expected: *const cm_pcs_config) -> i32;
    pub fn cm_shard_plan(input: *const cm_prover_input, config: *const cm_pcs_config, world: u32, owner: *mut i32, staging_words: *mut u64) -> i32;
    pub fn cm_shard_plan_columns(input: *const cm_prover_input, config: *const cm_pcs_config, world: u32, trace_col_owner: *mut i32, n_trace_cols: *mut u32, interaction_col_owner: *mut i32, n_interaction_cols: *mut u32, load_cells: *mut u64) -> i32;
    pub fn cm_prove_sharded(input: *const cm_device_input, config: *const cm_pcs_config, comm: *const cm_comm, out: *mut *mut cm_proof) -> i32;
    pub fn cm_rccl_unique_id(id_out: *mut u8) -> i32;
    pub fn cm_rccl_comm_create(id: *const u8, rank: u32, world: u32, staging_words: u64, out: *mut *mut cm_rccl_comm) -> i32;
    pub fn cm_rccl_comm_view(c: *const cm_rccl_comm) -> *const cm_comm;
    pub fn cm_rccl_comm_destroy(c: *mut cm_rccl_comm) -> i32;
    pub fn cm_prove_many(inputs: *const *const cm_device_input, n: u32, config: *const cm_pcs_config, inflight: u32, outs: *mut *mut cm_proof) -> i32;
    pub fn cm_prove_many_host(inputs: *const *const cm_prover_input, n: u32, config: *const cm_pcs_config, inflight: u32, outs: *mut *mut cm_proof) -> i32;
    pub fn cm_prove_many_segments(segments: *const *const cm_runner_segment, n: u32, config: *const cm_pcs_config, inflight: u32, outs: *mut *mut cm_proof) -> i32;
    pub fn cm_run_begin(initial_memory: *const u32, n_initial_memory: u64, initial_heap: *const u32, n_initial_heap: u64, ranges: *const u32, out: *mut *mut cm_run) -> i32;
    pub fn cm_run_adapt_next(r: *mut cm_run, seg: *const cm_run_segment, out: *mut *mut cm_device_input) -> i32;
    pub fn cm_run_memory(r: *const cm_run, locals: *mut u32, cap_l: u64, n_l: *mut u64, heap: *mut u32, cap_h: u64, n_h: *mut u64) -> i32;
    pub fn cm_run_free(r: *mut cm_run) -> i32;
    pub fn cm_prove_run(r: *mut cm_run, segs: *const *const cm_run_segment, n: u32, config: *const cm_pcs_config, inflight: u32, outs: *mut *mut cm_proof) -> i32;
    pub fn cm_proof_public_data(p: *const cm_proof, out: *mut cm_public_data) -> i32;
    pub fn cm_proof_public_entries(p: *const cm_proof, which: u32, out: *mut u32, cap_entries: u64, n_entries: *mut u64) -> i32;
    pub fn cm_device_input_public_entries(input: *const cm_device_input, which: u32, out: *mut u32, cap_entries: u64, n_entries: *mut u64) -> i32;
    pub fn cm_verify_run(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config) -> i32;
    pub fn cm_verify_many(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, results: *mut cm_verify_result, s: cm_stream_t) -> i32;
    pub fn cm_verify_run_device(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config) -> i32;
    pub fn cm_verify_many_timing(ms: *mut f64) -> i32;
    pub fn cm_verify_plan_stats(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, out: *mut cm_verify_stats) -> i32;
    pub fn cm_verify_many_detail(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, results: *mut cm_verify_result,
                                 slots: *mut cm_verify_slot, cap_slots: u32, slot_first: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_host_segment_end_lengths(h: *const cm_host_segment, n_memory_end: *mut u64, n_heap_end: *mut u64) -> i32;
    pub fn cm_set_preprocessed_cache(on: i32) -> i32;
    pub fn cm_set_twiddle_cache(on: i32) -> i32;
    pub fn cm_set_device_tail(on: i32) -> i32;
    pub fn cm_set_tuning(key: *const c_char, value: i32) -> i32;
    pub fn cm_tail_list(positions: *const u32, n_positions: u32, log_domain: u32, qmask: u32, list: u32, k: u32, out: *mut u32, cap: u32, n_out: *mut u32) -> i32;
    pub fn cm_tail_grind_op(digest: *const u32, bits: u32, nonce_out: *mut u64, s: cm_stream_t) -> i32;
    pub fn cm_tail_tables_op(digest: *const u32, nonce: u64, n_queries: u32, nq_pad: u32, log_domain: u32, qmask: u32, pieces: *const cm_tail_piece, n_pieces: u32, n_small: u32, out: *mut cm_tail_tables_out, s: cm_stream_t) -> i32;
    pub fn cm_tail_tab_words(nq_pad: u32) -> u64;
    pub fn cm_tail_last_op(digest: *const u32, last: *const cm_handle, log_n: u32, log_keep: u32, ar: *const u32, n_ar_words: u32, digest_out: *mut u32, degree_flag: *mut u32, last_out: *mut u32, ar_out: *mut u32, nonce_cell: *mut u64, s: cm_stream_t) -> i32;
    pub fn cm_eval_at_points_op(jobs: *const cm_eval_job, n_jobs: u32, t4: *const u32, want_landing: u32, out: *mut u32, landing: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_fri_fold_rows_op(out: *const cm_handle, src: *const cm_handle, alpha: *const u32, log_n: u32, tw: cm_handle, i0: u32, n_out: u32, flags: u32, s: cm_stream_t) -> i32;
    pub fn cm_fri_fold_leaves_rows_op(src: *const cm_handle, circle: *const cm_handle, alpha: *const u32, alpha_circle: *const u32, log_n: u32, tw: cm_handle, row0: u32, n_rows: u32, out: *const cm_handle, leaf_hashes: cm_handle, fused: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_accumulate_quotients_rows_op(log_size: u32, cols: *const cm_handle, n_cols: u32, batches: *const cm_sample_batches, random_coeff: *const u32, out: *const cm_handle, tw: cm_handle, row0: u32, n_rows: u32, leaf_hashes: cm_handle, device_coeffs: u32, sample_idx: *const u32, n_samples: u32, path: *mut u32, coef_c_out: *mut u32, sums_out: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_pack_parity_op(src: cm_handle, dst: cm_handle, half_len: u32, parity: u32, s: cm_stream_t) -> i32;
    pub fn cm_halo_build_op(even_half: cm_handle, odd_half: cm_handle, even_src: u32, odd_src: u32, row0: u32, len: u32, n: u32, trace_log: u32, log_ranks: u32, out: cm_handle, err: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_sum_copies_op(src: cm_handle, n_copies: u32, stride: u64, words: u64, out: cm_handle, modular: u32, s: cm_stream_t) -> i32;
    pub fn cm_copy_segments_op(src: *const cm_handle, dst: *const cm_handle, words: *const u64, n_segs: u32, s: cm_stream_t) -> i32;
    pub fn cm_verify_many_ex(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, flags: u32, results: *mut cm_verify_result, s: cm_stream_t) -> i32;
    pub fn cm_verify_many_detail_ex(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, flags: u32, results: *mut cm_verify_result, slots: *mut cm_verify_slot, cap_slots: u32, slot_first: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_verify_run_device_ex(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, flags: u32) -> i32;
    pub fn cm_public_logup_sum_op(jobs: *const cm_public_sum_job, n_jobs: u32, s: cm_stream_t, out: *mut u32) -> i32;
    pub fn cm_public_logup_sum_host(job: *const cm_public_sum_job, out4: *mut u32) -> i32;
    pub fn cm_point_eval_op(jobs: *const cm_point_eval_job, n_jobs: u32, s: cm_stream_t, out: *mut u32) -> i32;
    pub fn cm_point_eval_host(job: *const cm_point_eval_job, out4: *mut u32) -> i32;
    pub fn cm_proof_from_words(words: *const u32, n_words: u64, out: *mut *mut cm_proof) -> i32;
    pub fn cm_proof_words(p: *const cm_proof, words_out: *mut *const u32, n_out: *mut u64) -> i32;
    pub fn cm_proof_json(p: *const cm_proof, json_out: *mut *const c_char, len_out: *mut usize) -> i32;
    pub fn cm_proof_transcript(p: *const cm_proof, json_out: *mut *const c_char, len_out: *mut usize) -> i32;
    pub fn cm_proof_commitments(p: *const cm_proof, roots: *mut [u8; 32]) -> i32;
    pub fn cm_adapt_segment_device(seg: *const cm_runner_segment, out: *mut *mut cm_device_input) -> i32;
    pub fn cm_adapt_segment_host(seg: *const cm_runner_segment, out: *mut *mut cm_host_input) -> i32;
    pub fn cm_device_input_download(src: *const cm_device_input, out: *mut *mut cm_host_input) -> i32;
    pub fn cm_vm_segment(instr_words: *const u32, instr_lens: *const u32, n_instr: u32, entry_pc: u32, args: *const u32, n_args: u32, n_returns: u32, max_steps: u64, segment_index: u32, out: *mut *mut cm_host_segment, n_segments_out: *mut u32) -> i32;
    pub fn cm_synth_fibonacci_segment(n: u32, max_steps: u64, segment_index: u32, out: *mut *mut cm_host_segment) -> i32;
    pub fn cm_host_segment_view(h: *const cm_host_segment) -> *const cm_runner_segment;
    pub fn cm_segment_serialize_trace(s: *const cm_runner_segment, out: *mut u8, cap: u64, len: *mut u64) -> i32;
    pub fn cm_segment_serialize_memory_trace(s: *const cm_runner_segment, with_header: i32, out: *mut u8, cap: u64, len: *mut u64) -> i32;
    pub fn cm_host_segment_set_initial_heap(h: *mut cm_host_segment, initial_heap: *const u32, n_initial_heap: u64) -> i32;
    pub fn cm_segment_from_artifacts(trace: *const u8, trace_len: u64, mem: *const u8, mem_len: u64, mem_has_header: i32, initial_memory: *const u32, n_initial_memory: u64, ranges: *const u32, out: *mut *mut cm_host_segment) -> i32;
    pub fn cm_host_segment_free(h: *mut cm_host_segment) -> i32;
    pub fn cm_component_info(component: i32, n_trace_cols: *mut u32, n_interaction_cols: *mut u32, n_constraints: *mut u32) -> i32;
    pub fn cm_component_log_size(input: *const cm_device_input, component: i32, log_size: *mut u32) -> i32;
    pub fn cm_trace_write(input: *const cm_device_input, component: i32, cols: *const cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_histogram(component: i32, trace_cols: *const cm_handle, log_size: u32, rc8: cm_handle, rc16: cm_handle, rc20: cm_handle, bitwise: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_preprocessed_column(id: i32, col: cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_interaction_write(component: i32, trace_cols: *const cm_handle, preprocessed: *const cm_handle, log_size: u32, relations: *const cm_relations, out: *const cm_handle, claimed_sum: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_constraints_accumulate(component: i32, trace_lde: *const cm_handle, interaction_lde: *const cm_handle, preprocessed_lde: *const cm_handle, log_size: u32, relations: *const cm_relations, coeff_powers: *const u32, claimed_sum: *const u32, acc: *const cm_handle, s: cm_stream_t) -> i32;
    pub fn cm_check_constraints(input: *const cm_device_input, relations: *const cm_relations, out: *mut cm_check_report) -> i32;
    pub fn cm_constraints_check(component: i32, trace_cols: *const cm_handle, interaction_cols: *const cm_handle, preprocessed: *const cm_handle, log_size: u32, relations: *const cm_relations, claimed_sum: *const u32, row_status: cm_handle, failing_rows: *mut u64, first_constraint: *mut i32, first_row: *mut u64, s: cm_stream_t) -> i32;
    pub fn cm_track_relations(input: *const cm_device_input, relations: *const cm_relations, relation_mask: u32, report: *mut cm_check_report, entries: *mut cm_relation_entry, cap: u64, n_total: *mut u64) -> i32;
    pub fn cm_relation_entries(component: i32, trace_cols: *const cm_handle, preprocessed: *const cm_handle, log_size: u32, relations: *const cm_relations, relation_mask: u32, entries: *mut cm_relation_entry, cap: u64, n_total: *mut u64, s: cm_stream_t) -> i32;
    pub fn cm_link_diff(prev: *const cm_device_input, next: *const cm_device_input, report: *mut cm_link_report, cells: *mut cm_link_cell, cap: u64, n_total: *mut u64) -> i32;
    pub fn cm_check_chain(inputs: *const *const cm_device_input, n: u32, out: *mut cm_run_check, cells: *mut cm_link_cell, cap_per_link: u64) -> i32;
    pub fn cm_check_run(r: *mut cm_run, segs: *const *const cm_run_segment, n: u32, relations: *const cm_relations, out: *mut cm_run_check, cells: *mut cm_link_cell, cap_per_link: u64) -> i32;
    pub fn cm_input_open_memory(input: *const cm_device_input, which: u32, addresses: *const u32, n: u64, out: *mut cm_mem_opening, root: *mut u32) -> i32;
    pub fn cm_run_open_memory(r: *mut cm_run, addresses: *const u32, n: u64, out: *mut cm_mem_opening, root: *mut u32) -> i32;
    pub fn cm_verify_memory_openings(root: u32, openings: *const cm_mem_opening, n: u64, ok: *mut u8, s: cm_stream_t) -> i32;
    pub fn cm_verify_memory_opening(root: u32, opening: *const cm_mem_opening) -> i32;
    pub fn cm_input_open_memory_range(input: *const cm_device_input, which: u32, start: u32, n_cells: u32, values: *mut u32, out: *mut cm_mem_range_opening, root: *mut u32) -> i32;
    pub fn cm_run_open_memory_range(r: *mut cm_run, start: u32, n_cells: u32, values: *mut u32, out: *mut cm_mem_range_opening, root: *mut u32) -> i32;
    pub fn cm_verify_memory_range(root: u32, opening: *const cm_mem_range_opening, values: *const u32, ok: *mut u8, s: cm_stream_t) -> i32;
    pub fn cm_verify_memory_range_host(root: u32, opening: *const cm_mem_range_opening, values: *const u32) -> i32;
    pub fn cm_mem_range_plan(start: u32, n_cells: u32, steps: *mut cm_mem_range_step, cap: u32, n_steps: *mut u32) -> i32;
    pub fn cm_mem_set_plan(addresses: *const u32, n: u64, steps: *mut cm_mem_set_step, cap: u32, n_steps: *mut u32, n_siblings: *mut u32) -> i32;
    pub fn cm_input_open_memory_set(input: *const cm_device_input, which: u32, addresses: *const u32, n: u64, values: *mut u32, siblings: *mut u32, cap_siblings: u32, n_siblings: *mut u32, root: *mut u32) -> i32;
    pub fn cm_run_open_memory_set(r: *mut cm_run, addresses: *const u32, n: u64, values: *mut u32, siblings: *mut u32, cap_siblings: u32, n_siblings: *mut u32, root: *mut u32) -> i32;
    pub fn cm_verify_memory_set(root: u32, addresses: *const u32, n: u64, values: *const u32, siblings: *const u32, n_siblings: u32, ok: *mut u8, computed_root: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_memory_set_root_host(addresses: *const u32, n: u64, values: *const u32, siblings: *const u32, n_siblings: u32, root_out: *mut u32) -> i32;
    pub fn cm_verify_memory_set_host(root: u32, addresses: *const u32, n: u64, values: *const u32, siblings: *const u32, n_siblings: u32) -> i32;
    pub fn cm_input_write_set(input: *const cm_device_input, addresses: *mut u32, cap: u64, n_total: *mut u64, n_zero_only: *mut u64) -> i32;
    pub fn cm_input_open_transition(input: *const cm_device_input, addresses: *const u32, n: u64, out: *mut *mut cm_mem_transition) -> i32;
    pub fn cm_mem_transition_get(t: *const cm_mem_transition, out: *mut cm_mem_transition_view) -> i32;
    pub fn cm_mem_transition_free(t: *mut cm_mem_transition) -> i32;
    pub fn cm_verify_memory_transition(root_before: u32, root_after: u32, addresses: *const u32, n: u64, old_values: *const u32, new_values: *const u32, siblings: *const u32, n_siblings: u32, ok: *mut u8, computed: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_verify_memory_transition_host(root_before: u32, root_after: u32, addresses: *const u32, n: u64, old_values: *const u32, new_values: *const u32, siblings: *const u32, n_siblings: u32) -> i32;
    pub fn cm_prove_run_transitions(r: *mut cm_run, segs: *const *const cm_run_segment, n: u32, config: *const cm_pcs_config, inflight: u32, outs: *mut *mut cm_proof, transitions: *mut *mut cm_mem_transition) -> i32;
    pub fn cm_compose_transitions(parts: *const cm_mem_transition_view, n_parts: u32, device: u32, out: *mut *mut cm_mem_transition) -> i32;
    pub fn cm_verify_memory_transitions(parts: *const cm_mem_transition_view, n_parts: u32, ok: *mut u8, computed: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_verify_memory_sets(parts: *const cm_mem_set_view, n_parts: u32, ok: *mut u8, computed: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_mem_batch_plan(addresses: *const *const u32, n: *const u32, n_parts: u32, steps: *mut cm_mem_batch_step, cap: u32, n_steps: *mut u32) -> i32;
    pub fn cm_mem_image_create(addresses: *const u32, values: *const u32, n: u64, device: u32, out: *mut *mut cm_mem_image) -> i32;
    pub fn cm_mem_image_free(img: *mut cm_mem_image) -> i32;
    pub fn cm_mem_image_root(img: *mut cm_mem_image, root: *mut u32) -> i32;
    pub fn cm_mem_image_stats_get(img: *mut cm_mem_image, out: *mut cm_mem_image_stats) -> i32;
    pub fn cm_mem_image_read(img: *mut cm_mem_image, addresses: *const u32, n: u64, values: *mut u32) -> i32;
    pub fn cm_mem_image_cells(img: *mut cm_mem_image, addresses: *mut u32, values: *mut u32, cap: u64, n_total: *mut u64) -> i32;
    pub fn cm_mem_image_nodes(img: *mut cm_mem_image, nodes: *mut cm_merkle_node, cap: u64, n_total: *mut u64) -> i32;
    pub fn cm_mem_image_apply(img: *mut cm_mem_image, addresses: *const u32, new_values: *const u32, n: u64, old_values: *const u32, root_before: *const u32, root_after: *const u32, root_out: *mut u32, record_out: *mut *mut cm_mem_transition) -> i32;
    pub fn cm_mem_image_apply_transition(img: *mut cm_mem_image, t: *const cm_mem_transition_view, record_out: *mut *mut cm_mem_transition) -> i32;
    pub fn cm_mem_images_apply(parts: *const cm_mem_image_update, n_parts: u32, results: *mut cm_mem_image_result) -> i32;
    pub fn cm_mem_images_open_memory_sets(parts: *const cm_mem_set_request, n_parts: u32, results: *mut cm_mem_set_result) -> i32;
    pub fn cm_mem_image_open_memory(img: *mut cm_mem_image, addresses: *const u32, n: u64, out: *mut cm_mem_opening, root: *mut u32) -> i32;
    pub fn cm_mem_image_open_memory_range(img: *mut cm_mem_image, start: u32, n_cells: u32, values: *mut u32, out: *mut cm_mem_range_opening, root: *mut u32) -> i32;
    pub fn cm_mem_image_open_memory_set(img: *mut cm_mem_image, addresses: *const u32, n: u64, values: *mut u32, siblings: *mut u32, cap_siblings: u32, n_siblings: *mut u32, root: *mut u32) -> i32;
    pub fn cm_program_id_entries(entries: *const u32, n: u64, id: *mut u32) -> i32;
    pub fn cm_proof_program_id(p: *const cm_proof, id: *mut u32) -> i32;
    pub fn cm_program_ids(entries: *const *const u32, n_entries: *const u64, n: u32, ids: *mut u32, status: *mut i32, s: cm_stream_t) -> i32;
    pub fn cm_proofs_program_ids(proofs: *const *const cm_proof, n: u32, ids: *mut u32, status: *mut i32, s: cm_stream_t) -> i32;
    pub fn cm_run_statement_of(proofs: *const *const cm_proof, n: u32, expected: *const cm_pcs_config, expected_program_id: *const u32, device: u32, out: *mut cm_run_statement) -> i32;
    pub fn cm_relation_sums(component: i32, trace_cols: *const cm_handle, preprocessed: *const cm_handle, log_size: u32, relations: *const cm_relations, sums: *mut [u32; 4], s: cm_stream_t) -> i32;
    pub fn cm_accumulate(dst: *const cm_handle, src: *const cm_handle, n: u64, s: cm_stream_t) -> i32;
    pub fn cm_generate_secure_powers(felt: *const u32, n: u64, out: *mut u32) -> i32;
    pub fn cm_col_zero(h: cm_handle, n_u32: u64, s: cm_stream_t) -> i32;
    pub fn cm_fri_decompose(f: *const cm_handle, log_n: u32, lambda_out: *mut u32, s: cm_stream_t) -> i32;
    pub fn cm_kprof_enable(on: i32) -> i32;
    pub fn cm_kprof_report(buf: *mut c_char, buf_len: usize) -> i32;
    pub fn cm_kprof_filter(name: *const c_char) -> i32;
    pub fn cm_mem_stats_get(out: *mut cm_mem_stats) -> i32;
    pub fn cm_mem_reset_peak() -> i32;
    pub fn cm_proof_memory(p: *const cm_proof, out: *mut cm_proof_mem) -> i32;
    pub fn cm_estimate_memory(input: *const cm_prover_input, config: *const cm_pcs_config, world: u32, out: *mut cm_mem_estimate) -> i32;
    pub fn cm_estimate_memory_logs(log_size: *const u32, config: *const cm_pcs_config, world: u32, out: *mut cm_mem_estimate) -> i32;
    pub fn cm_set_memory_budget(bytes: u64) -> i32;
    pub fn cm_proof_stats(p: *const cm_proof, cells: *mut u64, steps: *mut u64, phase_ms: *mut f64, n_phases: u32) -> i32;
}
