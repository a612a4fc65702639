/*
 * cairom_hip.h — C ABI of libcairom_hip.so, the MI355X (gfx950) proving backend for Cairo-M.
 *
 * Drop-in boundary for ONE path of kkrt-labs/cairo-m: `prove_cairo_m::<Blake2sMerkleChannel>`
 * (crates/prover/src/prover.rs:23-147) and the Stwo backend-trait surface it drives
 * (ColumnOps / PolyOps / MerkleOps / GrindOps / QuotientOps / FriOps / AccumulationOps), plus the
 * Cairo-M component operations that are NOT reachable through those traits in the reference
 * (trace generation, LogUp interaction trace, constraint-quotient evaluation).
 *
 * Conventions
 *   - every function returns int32_t status: 0 = OK, non-zero = error; the message is available
 *     through cm_last_error() (thread-local).
 *   - cm_handle is an opaque 64-bit handle to library-owned device memory (a column = u32[n] of
 *     canonical M31 values; evaluations are stored in Stwo's BitReversedOrder).  Handles are freed
 *     by the caller with the matching cm_*_free.
 *   - QM31 / SecureField values cross the boundary as uint32_t[4] = to_m31_array()
 *     (reference layout: crates/prover/src/public_data.rs:146-149).
 *   - all functions take a cm_stream_t (0 = the library's default stream) and are safe to call
 *     concurrently from several host threads on different streams (the reference calls backend ops
 *     from rayon workers).
 *   - plain pointers and sizes only; no torch / C++ types.
 */
#ifndef CAIROM_HIP_H
#define CAIROM_HIP_H
#include <stddef.h>
#include <stdint.h>
/* Revision of this header.  4: cm_comm.struct_size at offset 0 (breaking for cm_comm users).  5: cm_shard_plan* take the PCS
 * config and column-array capacities; cm_set_device_tail, cm_tail_list.  6: cm_runner_segment grows by initial_heap /
 * n_initial_heap at its END (a revision-5 caller must be recompiled: the library reads the two fields);
 * cm_host_segment_set_initial_heap.  7: cm_check_report, cm_check_constraints, cm_constraints_check, cm_relation_sums.
 * 8: cm_relation_entry, cm_track_relations, cm_relation_entries.
 * 9: cm_mem_stats, cm_proof_mem, cm_mem_estimate; cm_mem_stats_get, cm_mem_reset_peak, cm_proof_memory, cm_estimate_memory,
 *    cm_estimate_memory_logs, cm_set_memory_budget.
 * 10: a whole run (additive): cm_run, cm_run_segment, cm_public_data; cm_run_begin, cm_run_adapt_next, cm_run_memory, cm_run_free,
 *    cm_prove_run, cm_proof_public_data, cm_proof_public_entries, cm_verify_run, cm_host_segment_end_lengths.
 *    Still 10 (additive: new symbols and one struct, nothing moved): cm_verify_result, CM_VERIFY_*, cm_verify_many,
 *    cm_verify_run_device, cm_verify_many_timing; cm_link_cell, cm_link_report, cm_run_check, cm_link_diff, cm_check_chain,
 *    cm_check_run.
 *    Still 10 (additive: four new functions and one struct, nothing moved): cm_mem_opening, cm_input_open_memory, cm_run_open_memory,
 *    cm_verify_memory_openings, cm_verify_memory_opening.
 *    Still 10 (additive: two host-only queries): cm_fft_plan, cm_fft_extend_fused.
 *    Still 10 (additive: two host-only queries, one op): cm_merkle_plan, cm_merkle_layer_npw, cm_merkle_commit_layers.
 *    Still 10 (additive: five new functions and two structs, nothing moved): cm_mem_range_opening, cm_mem_range_step,
 *    cm_input_open_memory_range, cm_run_open_memory_range, cm_verify_memory_range, cm_verify_memory_range_host, cm_mem_range_plan.
 *    Still 10 (additive: two host-side entry points): cm_adapt_segment_host, cm_device_input_public_entries.
 *    Still 10 (additive: six new functions and one struct, nothing moved): cm_mem_set_step, cm_mem_set_plan,
 *    cm_input_open_memory_set, cm_run_open_memory_set, cm_verify_memory_set, cm_memory_set_root_host, cm_verify_memory_set_host.
 *    Still 10 (additive: five new functions and one struct, nothing moved): cm_run_statement, cm_program_id_entries,
 *    cm_proof_program_id, cm_program_ids, cm_proofs_program_ids, cm_run_statement_of.
 *    Still 10 (additive: seven new functions, one view struct and one opaque handle, nothing moved): cm_mem_transition,
 *    cm_mem_transition_view, cm_input_write_set, cm_input_open_transition, cm_mem_transition_get, cm_mem_transition_free,
 *    cm_verify_memory_transition, cm_verify_memory_transition_host, cm_prove_run_transitions.
 *    Still 10 (additive: one host-only query, one entry point, two structs): cm_verify_stats, cm_verify_plan_stats, cm_verify_slot,
 *    cm_verify_many_detail.
 *    Still 10 (additive: one new function, no struct): cm_compose_transitions.
 *    Still 10 (additive: three new functions and two structs, nothing moved; listed with the family they batch): cm_mem_set_view,
 *    cm_mem_batch_step, cm_verify_memory_transitions, cm_verify_memory_sets, cm_mem_batch_plan.
 *    Still 10 (additive: one new function and two structs, nothing moved; listed with the batches): cm_mem_image_update,
 *    cm_mem_image_result, cm_mem_images_apply.
 *    Still 10 (additive: one new function and two structs, nothing moved; listed with the batches): cm_mem_set_request,
 *    cm_mem_set_result, cm_mem_images_open_memory_sets.
 *    Still 10 (additive: four new functions and two structs, nothing moved): cm_tail_piece, cm_tail_tables_out, cm_tail_grind_op,
 *    cm_tail_tables_op, cm_tail_tab_words, cm_tail_last_op.
 *    Still 10 (additive: one new function and one struct, nothing moved): cm_eval_job, cm_eval_at_points_op.
 *    Still 10 (additive: seven new functions and two sets of constants, nothing moved): CM_FOLD_*, CM_QUOT_PATH_*,
 *    cm_fri_fold_rows_op, cm_fri_fold_leaves_rows_op, cm_accumulate_quotients_rows_op, cm_pack_parity_op, cm_halo_build_op,
 *    cm_sum_copies_op, cm_copy_segments_op.
 *    Still 10 (additive: seven new functions, two structs and one flag, nothing moved): CM_VERIFY_ARITH_ON_DEVICE, cm_verify_many_ex,
 *    cm_verify_many_detail_ex, cm_verify_run_device_ex, cm_public_sum_job, cm_public_logup_sum_op, cm_public_logup_sum_host,
 *    cm_point_eval_job, cm_point_eval_op, cm_point_eval_host. */
#define CM_ABI_REVISION 10

#ifdef __cplusplus
extern "C" {
#endif

typedef uint64_t cm_handle;
typedef uint64_t cm_stream_t;

/* ---- runtime ------------------------------------------------------------------------------- */
int32_t cm_init(int32_t device);
int32_t cm_shutdown(void);
/* Returns the calling host thread's cached device blocks to the driver (the per-thread pool otherwise keeps the high-water
 * mark of the largest segment proved: a 2^26-row segment leaves ~116 GiB cached) — including what the thread's last proof parked
 * for its successor (the FRI phase and quotient columns of the deferred teardown: round 6; cm_shutdown and the pool's own
 * out-of-memory retry release them too). */
int32_t cm_pool_trim(void);
/* Free / total bytes of the library device's HBM (hipMemGetInfo): segment sizing for the 288 GB of an MI355X. */
int32_t cm_device_mem_info(uint64_t* free_bytes, uint64_t* total_bytes);
int32_t cm_last_error(char* buf, size_t buf_len);
int32_t cm_stream_create(cm_stream_t* out);
int32_t cm_stream_destroy(cm_stream_t s);
int32_t cm_stream_sync(cm_stream_t s);
/* CPU placement of proving threads.  A proof is ~450 kernel launches and ~10 host round trips; on a two-socket host a
 * thread on the socket away from the GPU pays the inter-socket fabric on each of them (0.1-0.5 ms per proof).
 *   mode 1 (default; env CM_CPU_AFFINITY=1): SCOPED — during cm_prove_device / cm_prove_segment / cm_prove_sharded the
 *          calling thread's affinity is narrowed to the GPU's sysfs local_cpulist (intersected with the mask it
 *          already had) and the caller's own mask is restored before the call returns, so nothing leaks into the
 *          host application, into threads it creates later or into child processes.  The library's own
 *          cm_prove_many worker threads stay on the GPU's node.
 *   mode 2 (env CM_CPU_AFFINITY=2): STICKY — a thread that calls cm_prove* is narrowed the same way ONCE and stays there: a
 *          dedicated proving thread saves the three affinity system calls of every proof (30-50 us on the hosts this was
 *          measured on; bench.py's worker threads use it and say so in their line).
 *   mode 0 (env CM_CPU_AFFINITY=0 or CM_NO_CPU_AFFINITY=1): the library never calls sched_setaffinity.
 * cm_get_cpu_affinity returns the mode in force. */
int32_t cm_set_cpu_affinity(int32_t mode);
int32_t cm_get_cpu_affinity(void);
/* Framing switches for the Stwo-side conventions that no in-tree reference vector settles (Stwo @ ab57a1c is an empty
 * submodule of the reference, .gitmodules:1-3; crates/prover/tests/prover.rs only asserts verify(..).is_ok()).  spec =
 * comma-separated name=value pairs, "" / "default" = all defaults; process-wide; env CM_FRAMING gives the initial value:
 *   mix_u64       = raw (default: one raw compression F(digest, [lo, hi, 0..]) — what SimdBackend::grind searches over,
 *                   prover.rs:90 / verifier.rs:55-58)  |  u32s (Blake2s256(digest || lo || hi) = mix_u32s(&[lo, hi]))
 *   hash_node     = raw (default: compression chain from the zero state, t = f = 0)  |  rfc (RFC 7693 Blake2s-256 of
 *                   left || right || le32(values))                       — Blake2sMerkleHasher::hash_node / commit_on_layer
 *   sample_batch  = insertion (default)  |  sorted (by point)           — ColumnSampleBatch::new_vec
 *   pcs_mix       = bql (default: pow_bits, log_blowup, n_queries, log_last_layer)  |  blq   — PcsConfig::mix_into, prover.rs:36
 * A reference-produced transcript (integration/prover-hip/tests/golden_dump.rs -> tests/golden/ref_*.json, compared step by
 * step by tests/test_ref_golden.py) tells which value is right; prover and verifier must run under the same setting.
 * cm_get_framing writes the setting in force ("mix_u64=raw,hash_node=raw,...") and returns its length (-1: the environment
 * variable CM_FRAMING is malformed — a hard error for every entry point until cm_set_framing replaces it).
 * cm_set_framing is refused (status 1) while a proof or a verification is running: one proof = one framing. */
int32_t cm_set_framing(const char* spec);
int32_t cm_get_framing(char* buf, size_t buf_len);
/* Transcript log: on = every proof records one entry per Fiat-Shamir call the reference prover makes (Stwo Channel::{mix_u32s,
 * mix_felts, mix_u64, draw_felt, draw_felts, draw_random_bytes} + MerkleChannel::mix_root, in the order of prover.rs:36-131)
 * with the channel digest after the call.  cm_proof_transcript returns them as JSON (buffer owned by the proof):
 * [{"op": "mix_u64", "digest": "<64 hex>", "n_words": 2, "words": [first <= 16 words mixed / drawn]}, ...]. */
int32_t cm_set_transcript_log(int32_t on);

/* ---- Column<T> / ColumnOps (Stwo core::backend::{Column, ColumnOps}; used through
 *      `ComponentTrace::to_evals`, crates/prover/src/components/mod.rs:168-177) ----------------- */
int32_t cm_col_alloc(uint64_t n_u32, cm_handle* out);
int32_t cm_col_free(cm_handle h);
int32_t cm_col_h2d(cm_handle h, const uint32_t* src, uint64_t n_u32, cm_stream_t s);
int32_t cm_col_d2h(cm_handle h, uint32_t* dst, uint64_t n_u32, cm_stream_t s);
/* Column::at / Column::set (element ranges, offsets in u32 words) and Column::clone (device to device) */
int32_t cm_col_read(cm_handle h, uint64_t offset_u32, uint32_t* dst, uint64_t n_u32, cm_stream_t s);
int32_t cm_col_write(cm_handle h, uint64_t offset_u32, const uint32_t* src, uint64_t n_u32, cm_stream_t s);
int32_t cm_col_copy(cm_handle dst, cm_handle src, uint64_t n_u32, cm_stream_t s);
/* ColumnOps::bit_reverse_column, in place, on n_cols columns of 2^log_n */
int32_t cm_bit_reverse(const cm_handle* cols, uint32_t n_cols, uint32_t log_n, cm_stream_t s);

/* ---- PolyOps (Stwo core::poly::circle::PolyOps) --------------------------------------------- */
/* PolyOps::precompute_twiddles for CanonicCoset(log_size).circle_domain().half_coset
 * (reference: crates/prover/src/prover.rs:56-60). */
int32_t cm_twiddles_precompute(uint32_t log_size, cm_handle* tw_out);
int32_t cm_twiddles_free(cm_handle tw);
/* PolyOps::interpolate_columns (reference: tree_builder.extend_evals, prover.rs:72, 81, 101):
 * bit-reversed evaluations on CanonicCoset(log_n).circle_domain() -> coefficients, in place. */
int32_t cm_interpolate(const cm_handle* cols, uint32_t n_cols, uint32_t log_n, cm_handle tw, cm_stream_t s);
/* PolyOps::evaluate / evaluate_polynomials (reference: tree_builder.commit, prover.rs:73, 82, 102):
 * coefficients of 2^log_n -> bit-reversed evaluations on CanonicCoset(log_out).circle_domain(). */
int32_t cm_evaluate(const cm_handle* coeffs, uint32_t n_cols, uint32_t log_n, uint32_t log_out, cm_handle tw,
                    const cm_handle* out, cm_stream_t s);
/* tree_builder.extend_evals at log_blowup_factor 1 (prover.rs:71-73, 80-82, 100-102): interpolate_columns followed by
 * evaluate on CanonicCoset(log_n + 1) in one call — evals (2^log_n each, bit-reversed) -> coeffs (2^log_n) and lde (2^(log_n+1)).
 * Results equal cm_interpolate + cm_evaluate word for word; for 2^18..2^21 rows the last inverse pass and the first forward
 * pass are one sweep over HBM.  evals[i] may equal coeffs[i] (in place). */
int32_t cm_interpolate_extend(const cm_handle* evals, const cm_handle* coeffs, const cm_handle* lde, uint32_t n_cols, uint32_t log_n,
                              cm_handle tw, cm_stream_t s);
/* The shape of a 2^log_n transform (1 <= log_n <= 28) as cm_interpolate / cm_evaluate run it: host code only, no GPU is
 * touched or initialised.  out[i] = { lo, hi, tile_log, M } of pass i in layer order (the inverse transform runs the passes
 * first to last, the forward one last to first): butterfly layers [lo, hi), the tile log of the register-blocked kernel that
 * runs them (11, 12, 13 or 14; 0 = the generic LDS-sweep kernel) and M, the log of a tile's contiguous run.  The launches
 * read the same function, so this is what runs.  CM_FFT_OLD_PLAN=1 in the environment (read once) selects the older plan. */
int32_t cm_fft_plan(uint32_t log_n, uint32_t out[8][4], uint32_t* n_passes);
/* *fused = 1 when cm_interpolate_extend takes the fused sweep at 2^log_n rows (1 <= log_n <= 27) under the current plan and
 * tuning ("fft_fused"), 0 when it runs the two transforms one after the other.  Host code only. */
int32_t cm_fft_extend_fused(uint32_t log_n, uint32_t* fused);
/* PolyOps::eval_at_point for n_cols polynomials at one QM31 circle point (x[4], y[4]);
 * out = n_cols * 4 u32 (host). */
int32_t cm_eval_at_point(const cm_handle* coeffs, uint32_t n_cols, uint32_t log_n, const uint32_t pt_xy[8],
                         uint32_t* out, cm_stream_t s);

/* ---- MerkleOps<Blake2sMerkleHasher>::commit_on_layer (reached from tree_builder.commit) ----- */
/* out_hashes: handle of 8 * 2^log_size u32.  prev_layer = 0 for the largest layer. */
int32_t cm_merkle_commit_layer(uint32_t log_size, cm_handle prev_layer, const cm_handle* cols, uint32_t n_cols,
                               cm_handle out_hashes, cm_stream_t s);
/* Whole mixed-degree tree (Stwo MerkleProver::commit): columns in commitment order with their
 * log sizes; writes the 32-byte root. */
int32_t cm_merkle_commit(const cm_handle* cols, const uint32_t* col_logs, uint32_t n_cols, uint8_t root[32],
                         cm_stream_t s);
/* cm_merkle_commit, and every stored layer copied out: layers_out (host, cap_words u32) receives the layers largest first, 8 u32
 * per node, ((2 << max_log) - 1) * 8 words in all (max_log = the largest column log).  The words are read back from the
 * tree's own layer buffers, the ones a decommitment gathers its hash witnesses from; nothing is recomputed. */
int32_t cm_merkle_commit_layers(const cm_handle* cols, const uint32_t* col_logs, uint32_t n_cols, uint8_t root[32],
                                uint32_t* layers_out, uint64_t cap_words, cm_stream_t s);
/* The launches of cm_merkle_commit for columns of these log sizes (commitment order), in launch order: host code only, no GPU
 * is touched or initialised.  The commitment consumes the same records, and the flags below come from the predicates the
 * kernels and the launch code evaluate, so this is what runs.  out[i] = one launch:
 *   [0] kind: 0 k_merkle_layer, 1 k_merkle_narrow, 2 k_merkle_layer_quad, 3 k_merkle_multi, 4 k_merkle_top, 5 k_merkle_tail
 *   [1] hi, [2] lo: the launch produces the layers 2^hi .. 2^lo      [3] 1 when layer hi + 1 exists (the launch reads children)
 *   [4] PREV, [5] NC, [6] chunks per wave of a k_merkle_narrow launch (0 otherwise)
 *   [7] bit l set: layer 2^l streams its columns through LDS (the quad kernel's layer, phase 2 of the top kernel, the tail)
 *   [8] index of the launch's first column among the columns sorted by size, descending
 *   [9 + k] columns of layer hi - k, k = 0 .. hi - lo
 * Depends on the tuning keys "merkle_npw" and "merkle_multi_top" and on CM_NO_MERKLE_TOP in the environment (read once).
 * At most 33 launches; cap_launches = the rows of `out`. */
#define CM_MERKLE_PLAN_WORDS 26
int32_t cm_merkle_plan(const uint32_t* col_logs, uint32_t n_cols, uint32_t out[][CM_MERKLE_PLAN_WORDS], uint32_t cap_launches,
                       uint32_t* n_launches);
/* What cm_merkle_commit_layer launches for a layer of 2^log_size nodes with n_cols columns, with (has_prev != 0) or without
 * children: *npw = 0 for k_merkle_layer, else the chunks per wave of k_merkle_narrow.  The predicate the launch itself and
 * cm_merkle_plan evaluate, under the current "merkle_npw".  Host code only. */
int32_t cm_merkle_layer_npw(uint32_t log_size, uint32_t has_prev, uint32_t n_cols, uint32_t* npw);

/* ---- GrindOps<Blake2sChannel>::grind (reference: prover.rs:90) ------------------------------- */
int32_t cm_grind(const uint8_t digest[32], uint32_t pow_bits, uint64_t* nonce_out, cm_stream_t s);

/* ---- FieldOps::batch_inverse ---------------------------------------------------------------- */
int32_t cm_batch_inverse_m31(cm_handle in, cm_handle out, uint64_t n, cm_stream_t s);
int32_t cm_batch_inverse_qm31(const cm_handle in[4], const cm_handle out[4], uint64_t n, cm_stream_t s);

/* ---- FriOps (Stwo core::fri::FriOps), SecureColumnByCoords = 4 coordinate handles ------------ */
/* dst (line evaluation, 2^(log_n-1)) = dst * alpha^2 + fold(src circle evaluation of 2^log_n) */
int32_t cm_fri_fold_circle_into_line(const cm_handle dst[4], const cm_handle src[4], const uint32_t alpha[4],
                                     uint32_t log_n, cm_handle tw, cm_stream_t s);
/* out (2^(log_n-1)) = fold_line(in (2^log_n), alpha) */
int32_t cm_fri_fold_line(const cm_handle in[4], const uint32_t alpha[4], uint32_t log_n, cm_handle tw,
                         const cm_handle out[4], cm_stream_t s);
/* A FRI layer and the leaf layer of its commitment in one pass (what FriProver::commit_inner_layers does per layer: fold, then
 * MerkleProver::commit over the folded SecureColumn — prover.rs:131 -> Stwo fri.rs).  Sources, each with its challenge:
 *   in (4 handles, 2^log_n line evaluations) + alpha              -> out = fold_line(in, alpha)
 *   circle (4 handles, 2^log_n circle evaluations) + alpha_circle -> FriOps::fold_circle_into_line of the quotient columns of
 *   that size: out = out * alpha_circle^2 + fold_circle(circle, alpha_circle); alone (in == NULL, alpha == NULL) it folds into a
 *   blank layer: out = fold_circle(circle, alpha_circle).
 * out: 4 handles of 2^(log_n-1).  leaf_hashes: 8 words per row of `out` = MerkleOps::commit_on_layer(log_n - 1, None, out). */
int32_t cm_fri_fold_line_leaves(const cm_handle* in, const cm_handle* circle, const uint32_t* alpha, const uint32_t* alpha_circle,
                                uint32_t log_n, cm_handle tw, const cm_handle out[4], cm_handle leaf_hashes, cm_stream_t s);

/* ---- QuotientOps::accumulate_quotients ------------------------------------------------------ */
/* One call per distinct LDE log size.  cols: the n_cols committed LDE columns of that size.
 * Sample batches (Stwo ColumnSampleBatch): batch b has point pts[b] (x[4],y[4]) and the entries
 * batch_cols[batch_off[b] .. batch_off[b+1]) = (column index, sampled value[4]).
 * out: 4 coordinate columns of 2^log_size. */
typedef struct {
  uint32_t n_batches;
  const uint32_t* points;       /* n_batches * 8 */
  const uint32_t* batch_off;    /* n_batches + 1 */
  const uint32_t* col_index;    /* total entries */
  const uint32_t* values;       /* total entries * 4 */
} cm_sample_batches;
int32_t cm_accumulate_quotients(uint32_t log_size, const cm_handle* cols, uint32_t n_cols,
                                const cm_sample_batches* batches, const uint32_t random_coeff[4],
                                const cm_handle out[4], cm_handle tw, cm_stream_t s);

/* ---- Cairo-M prover input (mirror of crates/prover/src/adapter/mod.rs:27-83 ProverInput) ----- */
#define CM_N_OPCODE_COMPONENTS 26
#define CM_N_COMPONENTS 34

/* ExecutionBundle (crates/prover/src/adapter/memory.rs:95-124) flattened the way
 * PackedExecutionBundle does (crates/prover/src/utils/execution_bundle.rs:12-31). */
typedef struct {
  uint32_t pc, fp, clock, inst_prev_clock;
  uint32_t inst[6];      /* instruction words incl. opcode, zero padded */
  uint32_t span_start;   /* AccessSpan.start into data_accesses */
  uint32_t span_len;     /* AccessSpan.len */
} cm_bundle;
/* DataAccess (adapter/memory.rs:57-67) */
typedef struct {
  uint32_t address, prev_clock, prev_value, value;
} cm_data_access;
/* one boundary memory cell: (addr, value[4], clock, multiplicity) (adapter/memory.rs:186-193) */
typedef struct {
  uint32_t address, value[4], clock, multiplicity;
} cm_memory_cell;
/* clock_update_data entry (adapter/memory.rs:192) */
typedef struct {
  uint32_t address, prev_clock, value[4];
} cm_clock_update;
/* NodeData (adapter/merkle.rs:92-104) */
typedef struct {
  uint32_t index, depth, left_value, right_value, parent_value, left_mult, right_mult, parent_mult;
} cm_merkle_node;

typedef struct {
  /* Instructions (adapter/mod.rs:69-83) */
  uint32_t initial_pc, initial_fp, final_pc, final_fp;
  /* bundles grouped by opcode COMPONENT, in the macro order of
   * crates/prover/src/components/opcodes/mod.rs:223-268 */
  const cm_bundle* bundles[CM_N_OPCODE_COMPONENTS];
  uint64_t n_bundles[CM_N_OPCODE_COMPONENTS];
  const cm_data_access* data_accesses;
  uint64_t n_data_accesses;
  /* Memory (adapter/memory.rs:186-193): rows are given in the order the memory component must
   * emit them (the reference iterates HashMaps; the caller fixes the order — SURVEY F3). */
  const cm_memory_cell* initial_memory;
  uint64_t n_initial_memory;
  const cm_memory_cell* final_memory;
  uint64_t n_final_memory;
  const cm_clock_update* clock_updates;
  uint64_t n_clock_updates;
  /* MerkleTrees (adapter/mod.rs:47-58) */
  const cm_merkle_node* initial_tree;
  uint64_t n_initial_tree;
  const cm_merkle_node* final_tree;
  uint64_t n_final_tree;
  uint32_t initial_root, final_root;
  /* PublicAddressRanges (crates/common/src/program.rs:111-122): [start, end) */
  uint32_t program_range[2], input_range[2], output_range[2];
} cm_prover_input;

/* ---- host-side input pipeline (no GPU needed) ------------------------------------------------------
 * Synthetic VM + adapter: runs a CASM program (instruction = 1..6 M31 words, opcode first; encodings of
 * crates/common/src/instruction.rs:314-577) from `entry_pc` with the runner's calling convention
 * (crates/runner/src/vm/mod.rs:249-281), cuts segments every max_steps like vm/mod.rs:158-240, and
 * converts segment `segment_index` with `import_from_runner_output`
 * (crates/prover/src/adapter/mod.rs:251-266).  Memory rows are emitted in ascending address order. */
typedef struct cm_host_input cm_host_input;
int32_t cm_vm_run(const uint32_t* instr_words, const uint32_t* instr_lens, uint32_t n_instr, uint32_t entry_pc,
                  const uint32_t* args, uint32_t n_args, uint32_t n_returns, uint64_t max_steps,
                  uint32_t segment_index, cm_host_input** out, uint32_t* n_segments_out);
/* The hand-assembled fibonacci_loop of SURVEY §8d: 10*n + 12 steps. */
int32_t cm_synth_fibonacci(uint32_t n, uint64_t max_steps, uint32_t segment_index, cm_host_input** out);
const cm_prover_input* cm_host_input_view(const cm_host_input* h);
uint64_t cm_host_input_steps(const cm_host_input* h);
int32_t cm_host_input_free(cm_host_input* h);
/* Test hook: replay `Memory::push` (crates/prover/src/adapter/memory.rs:470-535) over a script of accesses. */
int32_t cm_adapter_memory_script(const uint32_t* preload, uint32_t n_preload, const uint32_t* script, uint32_t n,
                                 uint32_t* results, uint32_t* n_clock_updates, uint32_t* clock_updates_out, uint32_t cu_cap,
                                 const uint32_t* query_addrs, uint32_t n_query, uint32_t* state_out);
/* Test hook: build_partial_merkle_tree (crates/prover/src/adapter/merkle.rs:183-295) over n cells (addr, v0..v3); nodes_out
 * = up to cap cm_merkle_node records, *n_nodes = their total count, *root = the root (0 for an empty memory). */
int32_t cm_adapter_partial_tree(const uint32_t* cells, uint32_t n, int32_t initial, const uint32_t ranges[6], uint32_t* nodes_out,
                                uint64_t cap, uint64_t* n_nodes, uint32_t* root);
/* Poseidon2-M31 t=16 permutation in place (reference KAT: crates/prover/tests/poseidon2.rs:14-34). */
int32_t cm_poseidon2_permute(uint32_t state[16]);

/* PcsConfig (crates/prover/src/prover_config.rs:13-20) */
typedef struct {
  uint32_t pow_bits;
  uint32_t log_blowup_factor;
  uint32_t log_last_layer_degree_bound;
  uint32_t n_queries;
} cm_pcs_config;

/* Proof object: opaque; serialised with cm_proof_json (serde layout of `Proof<Blake2sHash>`,
 * crates/prover/src/lib.rs:61-73 + main.rs:86-91). */
typedef struct cm_proof cm_proof;

/* prove_cairo_m::<Blake2sMerkleChannel> (crates/prover/src/prover.rs:23-147).
 * config == NULL selects REGULAR_96_BITS. */
int32_t cm_prove_segment(const cm_prover_input* input, const cm_pcs_config* config, cm_proof** out);
int32_t cm_proof_free(cm_proof* p);
/* Same path with the input already resident in HBM (what bench.py times): upload once, prove many. */
typedef struct cm_device_input cm_device_input;
int32_t cm_input_upload(const cm_prover_input* input, cm_device_input** out);
int32_t cm_input_free(cm_device_input* h);
int32_t cm_prove_device(const cm_device_input* input, const cm_pcs_config* config, cm_proof** out);
/* verify_cairo_m (crates/prover/src/verifier.rs:17-95 + Stwo verify): host code, works without a GPU.
 * 0 = the proof is accepted; otherwise status 11 and cm_last_error() names the failed check
 * (InvalidLogupSum, OodsNotMatching, Merkle(...), Fri(...), ProofOfWork, ...).  `words` = cm_proof_words format.
 * `expected` is the VERIFIER's PcsConfig (verify_cairo_m's `pcs_config: Option<PcsConfig>` argument, verifier.rs:19; NULL =
 * REGULAR_96_BITS {16, 1, 0, 80}): it is what goes into the transcript and what bounds the PoW / query count; a proof
 * made under any other config is rejected with InvalidStructure(config) — the prover never chooses the security level. */
int32_t cm_verify_proof(const cm_proof* p, const cm_pcs_config* expected);
int32_t cm_verify_proof_words(const uint32_t* words, uint64_t n_words, const cm_pcs_config* expected);
/* ---- intra-proof sharding (BASELINE configs[3]): `world` ranks (one process per GPU) prove ONE segment.
 * Whole components are assigned to ranks (cm_shard_plan: longest-processing-time bin packing by columns x rows) for trace
 * generation, LogUp, IFFT / LDE, constraint evaluation and OODS sampling; an all-to-all turns the committed LDE columns
 * into row-range ownership, so every rank hashes the Merkle subtree of its rows (sub-roots are all-gathered, the top
 * log2(world) levels are hashed by everyone) and accumulates the DEEP quotients of its rows; partial composition
 * accumulators are reduced across ranks.  FRI is committed by row range above 2^16 rows (folds are pair-local; a layer's tree
 * is the rank's subtree + a 32-byte all-gather) and finished on every rank below; the transforms of the preprocessed and the
 * composition tree are computed by every rank (replicated).  Every rank returns the same proof, bit-identical to cm_prove_device's.
 * The library does no communication itself: the host side (torch.distributed / RCCL in bench.py, anything else
 * elsewhere) provides two blocking collectives over two DEVICE staging buffers it owns.  Layouts are rank-major and
 * contiguous: all_to_all_v sends send_words[d] words to rank d from send_buf (blocks in rank order) and receives
 * recv_words[s] words from rank s into recv_buf; all_gather sends send_buf[0, words_per_rank) and receives world blocks. */
typedef struct cm_comm {
  uint32_t struct_size;              /* sizeof(cm_comm) as the CALLER compiled it: the fields behind all_gather are optional and are
                                      * only read when this size covers them (a binding that stops at all_gather works); smaller
                                      * than that = status 1.  ABI note: this field was inserted at offset 0 in header revision 4
                                      * (CM_ABI_REVISION), which moved every other field — a caller compiled against a revision-3
                                      * header is NOT compatible and is rejected with status 1 (its `rank` is read as a size) */
  uint32_t rank, world;              /* world: a power of two, 1..8 */
  void* ctx;
  uint32_t* send_buf;
  uint32_t* recv_buf;
  uint64_t buf_words;                /* capacity of each staging buffer (cm_shard_plan reports what a proof needs) */
  int32_t (*all_to_all_v)(void* ctx, const uint64_t* send_words, const uint64_t* recv_words);
  int32_t (*all_gather)(void* ctx, uint64_t words_per_rank);
  /* Optional (zero / NULL = the blocking form above).  CM_COMM_STREAM_ORDERED: the callbacks only ENQUEUE the exchange on the
   * stream given through set_stream and return at once; the prover then neither drains its stream before a collective nor waits
   * after it — everything stays ordered on that stream.  The prover calls set_stream with its own stream when a proof starts and
   * MAY call it again between two collectives (round 6: the claimed sums' all-gather follows the LogUp tail onto a side stream and
   * the communicator is handed back to the main stream right behind it): a callback always uses the stream of the latest call. */
  uint32_t flags;
  int32_t (*set_stream)(void* ctx, cm_stream_t stream);
  /* Optional.  Called when THIS rank fails inside cm_prove_sharded, before the error is returned: the other ranks are about to
   * block in their next collective, and only the communicator can release them (the in-library RCCL communicator calls
   * ncclCommAbort).  NULL: the host relies on its communicator's own timeout. */
  void (*abort)(void* ctx);
} cm_comm;
#define CM_COMM_STREAM_ORDERED 1u
/* host code (no GPU): which rank owns which component, and the staging capacity (words) a sharded proof of `input` needs UNDER
 * `config` (NULL = REGULAR_96_BITS) — the plan and the bound are the ones cm_prove_sharded runs with that config (components are
 * split only at log_blowup_factor 1; the exchanges grow with the blowup).  Revision 5: the `config` argument is new. */
int32_t cm_shard_plan(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, int32_t owner[CM_N_COMPONENTS],
                      uint64_t* staging_words);
/* owner[c] = -1: component c is SPLIT over all ranks — a large opcode component (more than an eighth of a rank's fair share of
 * the cells, at least 2^12 rows) is generated, looked up and constrained by ROW RANGE on every rank, and its columns are
 * transformed by the ranks the plan gives them to one by one (the four cumulative-sum columns of its LogUp stay together).
 * cm_shard_plan_columns reports that column-level plan: the owner of every column of trees 1 / 2 in commitment order and the
 * cells every rank transforms (load_cells[r], r < world).  *n_trace_cols / *n_interaction_cols: the CAPACITY of the array on
 * entry, the column count on return; an array that is too small is status 1 (nothing is written past it).  Pass NULL arrays to
 * learn the counts. */
int32_t cm_shard_plan_columns(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, int32_t* trace_col_owner,
                              uint32_t* n_trace_cols, int32_t* interaction_col_owner, uint32_t* n_interaction_cols,
                              uint64_t load_cells[8]);
int32_t cm_prove_sharded(const cm_device_input* input, const cm_pcs_config* config, const cm_comm* comm, cm_proof** out);
/* In-library cm_comm on RCCL (xGMI inside a node), stream-ordered: no host synchronisation around an exchange, nothing but
 * the library in the data path.  Rank 0 makes the 128-byte id (cm_rccl_unique_id) and the launcher hands it to every rank;
 * every rank creates its communicator with the staging capacity cm_shard_plan reports and passes cm_rccl_comm_view() to
 * cm_prove_sharded.  librccl.so is loaded on first use (dlopen; a copy the process already mapped is reused). */
typedef struct cm_rccl_comm cm_rccl_comm;
int32_t cm_rccl_unique_id(uint8_t id_out[128]);
int32_t cm_rccl_comm_create(const uint8_t id[128], uint32_t rank, uint32_t world, uint64_t staging_words, cm_rccl_comm** out);
const cm_comm* cm_rccl_comm_view(const cm_rccl_comm* c);
int32_t cm_rccl_comm_destroy(cm_rccl_comm* c);
/* Segment pipeline: prove n independent segments with up to `inflight` (1..8) proofs in flight on the
 * GPU (persistent worker threads inside the library, one stream set / device pool each).  outs[i] = proof of
 * inputs[i]; on error the first failure is returned and the proofs already built stay in outs (free them). */
int32_t cm_prove_many(const cm_device_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                      cm_proof** outs);
/* Streaming ingest: cm_prove_many from HOST inputs — the entry point of the reference takes a host
 * `&mut ProverInput` (crates/prover/src/prover.rs:23-29).  The calling thread uploads input i + 1 (cm_prove_many_host) or runs
 * the device adapter on runner segment i + 1 (cm_prove_many_segments = import_from_runner_output, adapter/mod.rs:97-193) on
 * its own stream while up to `inflight` (1..8) library threads prove the inputs before it: the PCIe copies hide under the
 * proofs.  At most inflight + 1 inputs are resident in HBM at any time (inflight + 2 for cm_prove_many_segments, whose adapter —
 * uploads, sorts and five host round trips per segment — runs on a second library thread as well).  outs[i] = proof of item i (bit-identical to
 * cm_prove_segment / cm_adapt_segment_device + cm_prove_device of the same item); error contract of cm_prove_many. */
int32_t cm_prove_many_host(const cm_prover_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                           cm_proof** outs);
/* Preprocessed-tree cache: tree 0 commits constant tables (crates/prover/src/preprocessed/mod.rs:75-82;
 * verifier.rs:38 notes its root is a known constant).  Off by default (every proof recomputes it, as prover.rs:70-73
 * does); on = each host thread keeps the committed tree (coefficients, LDE, Merkle layers) between proofs of one
 * PCS config.  Env CM_PREPROCESSED_CACHE=1 sets the initial value.  Proof bytes are identical either way. */
int32_t cm_set_preprocessed_cache(int32_t on);
/* Twiddle tables: the reference recomputes them in every prove_cairo_m (prover.rs:56-60), and so does every proof here by
 * default (pool memory, on a side stream next to trace generation).  on = keep one table per domain size for the whole
 * process (env CM_TWIDDLE_CACHE=1 sets the initial value).  Off in every quoted number.  Proof bytes are identical. */
int32_t cm_set_twiddle_cache(int32_t on);
/* Tail of a proof — everything stwo `prove` (prover.rs:131) does behind the last FRI fold: the last layer's polynomial, the
 * proof of work, the query draws and the decommitment of every tree.  1 (default; env CM_DEVICE_TAIL=0 sets the initial value
 * to 0) = four launches enqueued behind the last fold, witnesses written to pinned host memory in proof order, the host
 * replays the transcript steps afterwards and refuses the proof on a mismatch (cairo_m_amd/csrc/tail_device.hpp);
 * 0 = the host drives each step (round trip per step, symbolic decommitment walk on the host).  Proof bytes are identical. */
int32_t cm_set_device_tail(int32_t on);
/* (revision 6) Measurement switches, flipped inside one process so that two forms can be timed alternately on the same box
 * (tools/ab_switch.py: paired blocks of lone proofs); every form produces the same proof bytes.  Each has an environment
 * variable of the same name in capitals behind CM_ for its initial value.  key (default):
 *   "oods_poll" (1)          the sampled values are watched arriving in pinned host memory; 0 = event / stream synchronisation
 *   "oods_host_write" (1)    (with oods_poll) the kernel that reduces them writes the pinned words; 0 = copy commands, watched
 *   "oods_split" (780)       per mille of the sampled values evaluated, copied and hashed first (1000 = one chunk)
 *   "stage_copy_kernel" (1)  small host -> device uploads are a kernel reading the pinned staging ring; 0 = hipMemcpyAsync (the SDMA
 *                            engine above a few KB)
 *   "stage_lazy_events" (1)  the staging ring's event of the thread's main stream is recorded when the ring wraps; 0 = per upload
 *   "defer_teardown" (1)     the pool blocks of a proof's FRI phase / quotient plan are given back by the calling thread's NEXT
 *                            proof while it waits for tree 1 (or when the thread ends); 0 = before cm_prove* returns
 *   "tail_flags" (1)         the host follows the device-side tail by two header words the kernels set behind their pinned writes;
 *                            0 = two events recorded between the tail's launches
 *   "flag_join" / "flag_fork" (1)  fork regions joined / forked by flag words polled by one-wave kernels; 0 = HIP events
 *   "commit_prep_early" (1)  the interaction tree's launch plan is prepared under the LogUp kernels; 0 = behind them
 *   "trace_hist_fuse" (1)    trace cells and lookup histogram of a large opcode component in one launch; 0 = two
 *   "logup_defer" (1)        the LogUp tail (claimed sums, prefix scans) on a side stream next to the first transforms; 0 = in front
 *   "fri_top_fuse" (1)       fold + transcript step inside the tree-top launch of the FRI layers <= 2^16; 0 = three launches
 * and the policy choices of earlier rounds, numeric where the environment variable was: "fork_main" (1), "merkle_npw" (-1 = by
 * layer size, 0 = k_merkle_layer, 1..8 chunks per wave), "fork_width" (0 = all side streams), "pp_side" (1), "tree0_prio" (-1 high
 * priority stream, 0 fork side stream, 1 low), "tree1_first" (1), "logup_width" (4), "quot_rows" (2), "fri_fold_leaf" (1),
 * "fft_fused" (1), "commit_pipe" (1), "fft_chunk_mb" (0 = off), "pace" (-1 = by load), "pace_early" (1).
 * Round 6: "cons_wide_first" (1: a wide component of few rows — poseidon2's 443 columns — is the first launch of the constraint
 * region), "cons_plan" (side-stream plan of that region as eight octal digits, default 01237456), "logup_small_stream" (-1 = stream
 * `logup_width`; 0..7 picks the side stream of the batched small LogUp launch), "quot_leaf" (1: the DEEP-quotient kernel of the largest
 * size group also writes the leaf hashes of the FRI first-layer tree), "shard_fri_stream" (1: cm_prove_sharded keeps its row-sharded
 * FRI layers on the stream — tree top and transcript step on the device, one host replay per proof), "shard_halo" (1: the previous-row
 * neighbours of a split component's cumulative-sum columns come from the two neighbouring row ranges instead of an all-gather), "tree0_guest"
 * (0; 1 = the preprocessed columns are transformed inside the trace tree's size-group launches: measured neutral), "tw_batch" (8), "fft_half_occ" (0; bit 0 / 1 =
 * one 2^14-tile / four 2^12-tile transform blocks per CU instead of two / eight: measured slower, kept for A/B), "shard_tree_stream" (1:
 * cm_prove_sharded keeps the transcript steps behind its four commitment trees on the stream — tree top on the device, the single-GPU
 * prover's step kernels, host replay at the two waits that are left before FRI; 0 = a host round trip per root), "shard_fri_stop_log"
 * (16: FRI layers of at most 2^v rows are gathered and finished on every rank; 99 = FRI not sharded; also CM_SHARD_FRI_STOP_LOG).
 * Test hook: "tail_grind_cap" (0 = off; v > 0 stops the device tail's proof-of-work search after 2^(v-1) nonces, so that the
 * host-driven fallback behind a missed nonce — probability e^-16 in production — can be exercised; same proof bytes).
 * status 1 for an unknown key or a value outside the key's range.  Flip a switch only while no proof is running in the process: a
 * proof reads some of them more than once (a fork region decides at its fork AND at every side stream how it synchronises). */
int32_t cm_set_tuning(const char* key, int32_t value);
/* The node lists the device-side tail gathers by (host code, no GPU: the mirror the prover checks the device against; the CPU
 * tests compare it with a restatement of MerkleProver::decommit).  positions: the sorted, de-duplicated query positions on the
 * domain of 2^log_domain points; qmask: bit l = the first FRI tree carries columns of 2^l rows; list: 0 = U[k] (queried nodes
 * of the layer of 2^(log_domain - k) nodes), 1 = W[k] (their unqueried siblings), 2 = F[k] (hashes of the layer below that the
 * first FRI tree's walk asks for at that layer).  Writes min(*n_out, cap) entries; *n_out = the list's length. */
int32_t cm_tail_list(const uint32_t* positions, uint32_t n_positions, uint32_t log_domain, uint32_t qmask, uint32_t list, uint32_t k,
                     uint32_t* out, uint32_t cap, uint32_t* n_out);
/* ---- the device-side tail, kernel by kernel (test surface; cairo_m_amd/csrc/tail_ops.hip) ---------------------------------------
 * Each entry runs ONE step of the tail the prover enqueues behind the last FRI fold — the same kernels through the same host
 * wrappers, on the same pinned buffers — on inputs the caller chooses instead of the ones a transcript happens to produce, and
 * synchronises the stream before it returns.  Every argument is checked before the first device call (status 1 and a message);
 * what cannot be checked is the height of the caller's columns, stated per piece below.  digest = the channel digest as 8 words.
 *
 * cm_tail_grind_op: k_tail_grind on a device channel holding `digest` and a nonce cell armed with ~0, under the "tail_grind_cap"
 * tuning in force.  *nonce_out = the nonce cell afterwards: the smallest nonce with `bits` trailing zero bits, ~0 = not found within
 * the search limit (2^max(bits + 4, 8) nonces, or the cap).  bits <= 26. */
int32_t cm_tail_grind_op(const uint32_t digest[8], uint32_t bits, uint64_t* nonce_out, cm_stream_t s);
/* One piece of the decommitment, in output order.  kind 0: hashes (8 words per node) of the nodes W[k], cols[0] = a layer of
 * 2^(log_domain - k) nodes; kind 1: hashes of the nodes F[k] (k >= 1), cols[0] = the layer of 2^(log_domain - k + 1) nodes;
 * kind 2: 4 words per row W[k], interleaved from the four columns cols[0..3] of 2^(log_domain - k) rows; kind 3: `width` words per
 * row U[k], word c from cols[c] (2^(log_domain - k) rows; a handle may repeat).  `width` is read for kind 3 only. */
typedef struct cm_tail_piece {
  uint32_t kind, k, width, reserved;
  const cm_handle* cols;
} cm_tail_piece;
enum { CM_TAIL_HDR_WORDS = 16, CM_TAIL_SHIFTS = 32, CM_TAIL_NO_NONCE = 1 };
/* Host buffers cm_tail_tables_op fills.  hdr: CM_TAIL_HDR_WORDS words {status (0 / CM_TAIL_NO_NONCE), nonce lo, nonce hi, n_unique,
 * total words, -, -, -, tables done}; positions: nq_pad words, the first n_unique are the sorted query positions; tab: the device
 * tables as they are, cm_tail_tab_words(nq_pad) words = {cntU[32] | cntW[32] | cntF[32] | U[32][nq_pad] | W[32][nq_pad] |
 * F[32][4 nq_pad]} (a list's entries behind its count are unspecified); offsets: n_pieces words, the first output word of every
 * piece; words: the gathered words (hdr[4] of them; words_cap must be at least the bound the prover sizes its buffer by: per piece
 * min(n_queries, 2^(log_domain - k)) items, three times that for kind 1, times the words per item). */
typedef struct cm_tail_tables_out {
  uint32_t struct_size, reserved;
  uint32_t* hdr;
  uint32_t* positions;
  uint32_t* tab;
  uint32_t* offsets;
  uint32_t* words;
  uint64_t words_cap;
} cm_tail_tables_out;
/* k_tail_tables, then k_tail_gather: mix_u64(nonce) into a device channel holding `digest`, the n_queries raw-word draws of
 * Queries::generate masked to log_domain bits, sorted and de-duplicated; the U / W / F lists of every shift k <= log_domain under
 * `qmask` (cm_tail_list's definitions); the offset of every piece; the gathers.  pieces [0, n_small) are of kind 0 - 2, the rest of
 * kind 3.  1 <= n_queries <= 1024; nq_pad = a power of two in [n_queries, 1024]; log_domain <= 31.  nonce = ~0 (the proof of work
 * missed) comes back as hdr[0] = CM_TAIL_NO_NONCE. */
int32_t cm_tail_tables_op(const uint32_t digest[8], uint64_t nonce, uint32_t n_queries, uint32_t nq_pad, uint32_t log_domain,
                          uint32_t qmask, const cm_tail_piece* pieces, uint32_t n_pieces, uint32_t n_small, cm_tail_tables_out* out,
                          cm_stream_t s);
uint64_t cm_tail_tab_words(uint32_t nq_pad);
/* k_tail_last on the 2^log_n evaluations last[0..3] (bit-reversed order, log_n <= 6) with the prover's own twiddle table:
 * digest_out = the device channel's digest after mix_felts(the first 2^log_keep coefficients in LinePoly order), *degree_flag = 1
 * if a coefficient above the bound is non-zero, last_out = the 4 * 2^log_n words handed to the host (coordinate-major), ar_out =
 * the copy of the n_ar_words (<= 384) words `ar` (the commit phase's challenges and roots), *nonce_cell = the armed nonce cell (~0). */
int32_t cm_tail_last_op(const uint32_t digest[8], const cm_handle last[4], uint32_t log_n, uint32_t log_keep, const uint32_t* ar,
                        uint32_t n_ar_words, uint32_t digest_out[8], uint32_t* degree_flag, uint32_t* last_out, uint32_t* ar_out,
                        uint64_t* nonce_cell, cm_stream_t s);
/* ---- the prover's out-of-domain sampling, on inputs the caller chooses (test surface; cairo_m_amd/csrc/capi_ops.hip) -----------
 * One sampling group: n_cols coefficient columns of 2^log_n words (log_n <= 26, n_cols >= 1; a handle may repeat) evaluated at one
 * QM31 circle point.  point = x[4] then y[4], read in the host-point form only.  has_shift / shift_x / shift_y (canonical M31
 * words, refused otherwise even when has_shift is 0): read in the device-point form only, where the job samples at the point of
 * the felt plus the M31 point (shift_x, shift_y) in the circle group — the previous-row mask of the prover. */
typedef struct cm_eval_job {
  uint32_t log_n, n_cols;
  const cm_handle* coeffs;
  uint32_t point[8];
  uint32_t has_shift, shift_x, shift_y, reserved;
} cm_eval_job;
enum { CM_EVAL_MAX_JOBS = 64, CM_EVAL_GUARD_WORDS = 4 };
#define CM_EVAL_GUARD 0xA5A5A5A5u
/* All n_jobs groups (1 <= n_jobs <= CM_EVAL_MAX_JOBS; n_jobs == 0 is refused) through the host wrapper the provers call for their
 * sampling, eval_at_point_multi: k_point_tables_multi, k_eval_partial_multi, k_reduce_partials_multi and, when t4 is not NULL,
 * k_oods_maps in front of them.  t4 == NULL: the host-point form, every job samples at its own `point`.  t4 != NULL (four canonical
 * words): the felt is uploaded and every job's point is derived on the device as CirclePoint::get_random_point does from a drawn
 * felt, ((1 - t^2) / (1 + t^2), 2t / (1 + t^2)), plus the job's shift; a felt with 1 + t^2 = 0 has no point and is the caller's
 * to avoid.
 * out: 4 * sum(n_cols) + CM_EVAL_GUARD_WORDS * n_jobs words, the device output buffer as it is after the kernels: per job, in job
 * order, 4 words per column and then CM_EVAL_GUARD_WORDS words that the entry set to CM_EVAL_GUARD before the launch and no kernel
 * may touch (the entry fills the whole buffer with that word, which no M31 takes: a value left unwritten shows too).
 * want_landing != 0: every job's h_out points into a pinned landing buffer of the same layout, filled with 0xFF bytes before the
 * launch as the prover fills its own; `landing` receives it whole (same size as out), guards and all.  want_landing == 0: landing
 * is not read and the kernels store to device memory only.
 * Every argument is checked before the first device call (status 1 and a message): NULL jobs / out / coeffs / handle / landing
 * with want_landing, n_jobs outside 1..64, n_cols == 0 or above 65536, log_n above 26, a shift, felt or point word >= P.  The
 * heights of the caller's columns cannot be checked.  The stream is synchronised before the call returns. */
int32_t cm_eval_at_points_op(const cm_eval_job* jobs, uint32_t n_jobs, const uint32_t* t4, uint32_t want_landing, uint32_t* out,
                             uint32_t* landing, cm_stream_t s);
/* ---- the row-range and prover-only forms of the FRI and quotient kernels, and the sharded prover's data movement, on inputs the
 * caller chooses (test surface; cairo_m_amd/csrc/shard_ops.hip) ------------------------------------------------------------------
 * Each entry calls the host wrapper the provers call and synchronises the stream.  Every argument is checked before the first
 * device call (status 1 and a message that starts with the entry's name): NULL pointers and handles, a count of 0, log_n / log_size
 * against what the twiddle handle covers, a row range that leaves the domain, an index out of range, a field word >= P.  The
 * lengths of the caller's columns cannot be checked.  Handles of "slices" are plain column handles whose word 0 is the first row
 * of the range.
 *
 * Outputs [i0, i0 + n_out) of a fold of 2^log_n values (fold_line_rows; with CM_FOLD_CIRCLE fold_circle_into_line_rows, which with
 * CM_FOLD_ACCUMULATE computes out * alpha^2 + fold): src holds source rows [2 i0, 2 (i0 + n_out)), out holds the n_out outputs.
 * CM_FOLD_ALPHA_ON_DEVICE: the challenge is uploaded and passed as the wrappers' d_alpha, the way both provers pass it (the kernel
 * argument is then another value); otherwise it is the kernel argument.  n_out >= 1, i0 + n_out <= 2^(log_n - 1). */
#define CM_FOLD_CIRCLE 1u
#define CM_FOLD_ACCUMULATE 2u
#define CM_FOLD_ALPHA_ON_DEVICE 4u
int32_t cm_fri_fold_rows_op(const cm_handle out[4], const cm_handle src[4], const uint32_t alpha[4], uint32_t log_n, cm_handle tw,
                            uint32_t i0, uint32_t n_out, uint32_t flags, cm_stream_t s);
/* cm_fri_fold_line_leaves on outputs [row0, row0 + n_rows) of the layer (n_rows a power of two, row0 + n_rows <= 2^(log_n - 1)):
 * in / circle hold source rows [2 row0, 2 (row0 + n_rows)), out the n_rows outputs, leaf_hashes 8 words per output row.
 * *fused = 1 when k_fold_leaf made the launch (fold_line_leaf / fold_circle_leaf with row0, n_rows), 0 when the wrapper declined
 * and the entry did what the sharded prover then does: fold_line_rows / fold_circle_into_line_rows with device challenges, then
 * the leaf layer of the slice (merkle_layer). */
int32_t cm_fri_fold_leaves_rows_op(const cm_handle* in, const cm_handle* circle, const uint32_t* alpha, const uint32_t* alpha_circle,
                                   uint32_t log_n, cm_handle tw, uint32_t row0, uint32_t n_rows, const cm_handle out[4],
                                   cm_handle leaf_hashes, uint32_t* fused, cm_stream_t s);
/* cm_accumulate_quotients on rows [row0, row0 + n_rows) of the 2^log_size domain: cols and out hold that row range only
 * (n_rows == 0 with row0 == 0: the whole domain, as the single-GPU prover launches it).  *path = the kernel family
 * launch_quotients chose, one of CM_QUOT_PATH_*.
 * leaf_hashes != 0: 8 words per row of the range, written by k_quotients_rows<2, LEAF> = MerkleOps::commit_on_layer(no children,
 * out); the launch must be one quotient_leaf_serves admits (one or two batches, "quot_rows" 2, a power-of-two range of at least
 * 2^"merkle_multi_top" rows with row0 a multiple of it), any other is refused.
 * device_coeffs != 0: the provers' route from sampled values to quotients.  batches->values then holds n_samples sampled values
 * (4 words each) and sample_idx[e] < n_samples names entry e's; the entry builds one QuotientCoefJob per batch, k_quotient_coeffs
 * fills coef_c, sum_a, sum_b and batch_coeff on the device, the quotient launch reads them there, and they come back: coef_c_out
 * (4 words per entry), sums_out (per batch 12 words: sum_a, sum_b, batch_coeff).  device_coeffs == 0: batches->values holds one
 * value per entry, the coefficients are computed on the host as in cm_accumulate_quotients, and sample_idx, n_samples, coef_c_out
 * and sums_out are not read. */
#define CM_QUOT_PATH_ROWS2 1u
#define CM_QUOT_PATH_ROWS4 2u
#define CM_QUOT_PATH_ROWS2_LEAF 3u
#define CM_QUOT_PATH_ONE_ROW 4u
#define CM_QUOT_PATH_SLICES8 5u
#define CM_QUOT_PATH_SLICES64 6u
int32_t cm_accumulate_quotients_rows_op(uint32_t log_size, const cm_handle* cols, uint32_t n_cols, const cm_sample_batches* batches,
                                        const uint32_t random_coeff[4], const cm_handle out[4], cm_handle tw, uint32_t row0,
                                        uint32_t n_rows, cm_handle leaf_hashes, uint32_t device_coeffs, const uint32_t* sample_idx,
                                        uint32_t n_samples, uint32_t* path, uint32_t* coef_c_out, uint32_t* sums_out, cm_stream_t s);
/* The sharded prover's data movement (kernels_shard.hip).  pack_parity: dst[i] = src[2 i + parity], i < half_len.
 * halo_build: out[q] = the column at the previous trace row of global position row0 + q, q < len, looked up in the halves
 * (2^(n - log_ranks - 1) words each) received from ranks even_src / odd_src; n = log of the domain, trace_log <= n the trace
 * domain's (the prover passes n - 1), 1 <= log_ranks < n; *err = the kernel's error word: 1 when a lookup fell outside the two
 * neighbours, whose output words are then left unwritten.
 * sum_copies: out[i] = sum over k < n_copies of in[k * stride + i], i < words, stride >= words; modular != 0: M31 sums of
 * canonical words, else u32 sums that wrap.
 * copy_segments: dst[i][j] = src[i][j], j < words[i], every segment in one launch; a segment of 0 words is skipped and a call
 * whose segments are all empty, or that has none, launches nothing. */
int32_t cm_pack_parity_op(cm_handle src, cm_handle dst, uint32_t half_len, uint32_t parity, cm_stream_t s);
int32_t cm_halo_build_op(cm_handle even_half, cm_handle odd_half, uint32_t even_src, uint32_t odd_src, uint32_t row0, uint32_t len,
                         uint32_t n, uint32_t trace_log, uint32_t log_ranks, cm_handle out, uint32_t* err, cm_stream_t s);
int32_t cm_sum_copies_op(cm_handle in, uint32_t n_copies, uint64_t stride, uint64_t words, cm_handle out, uint32_t modular,
                         cm_stream_t s);
int32_t cm_copy_segments_op(const cm_handle* src, const cm_handle* dst, const uint64_t* words, uint32_t n_segs, cm_stream_t s);
/* Proof object from its flat word stream (host code, no GPU): re-serialise with cm_proof_json / verify with cm_verify_proof. */
int32_t cm_proof_from_words(const uint32_t* words, uint64_t n_words, cm_proof** out);
/* Flat u32 serialisation of the proof (format: cairo_m_amd/csrc/proof.hpp), used by the parity tests. */
int32_t cm_proof_words(const cm_proof* p, const uint32_t** words_out, uint64_t* n_out);
/* JSON text of the proof; *len_out = length without the terminating NUL; the buffer is owned by
 * the proof object. */
int32_t cm_proof_json(const cm_proof* p, const char** json_out, size_t* len_out);
int32_t cm_proof_transcript(const cm_proof* p, const char** json_out, size_t* len_out);
/* The four commitment roots (trees 0..3), 32 bytes each. */
int32_t cm_proof_commitments(const cm_proof* p, uint8_t roots[4][32]);
/* ---- device-memory accounting, estimate and budget (revision 9) --------------------------------------------------------------
 * Every block a proof uses comes from a caching pool per host thread (cairo_m_amd/csrc/pool.hip).  The counters below are
 * process-wide sums over all thread pools, kept with relaxed atomics on the pool's own paths (no lock, no driver call):
 *   live_bytes      capacity of the blocks handed out and not yet given back (a proof's columns, a resident cm_device_input,
 *                   what a finished proof parked for its successor, a cached preprocessed tree)
 *   reserved_bytes  live + cached = everything the library holds from the driver through the pool
 *   peak_*          high-water marks since the last cm_mem_reset_peak
 *   driver_allocs   hipMalloc calls of the pool since the last reset (0 in a steady state of equal proofs)
 *   pinned_host_bytes  the pinned host buffers of the threads that entered the library: upload ring, landing buffer, the
 *                   device tail's two buffers, the fixed result words
 * NOT counted (direct driver allocations outside the pool): caller-owned columns of cm_col_alloc, the process-wide twiddle tables
 * of cm_set_twiddle_cache(1) (cm_mem_estimate.cached_bytes does include them), the proof-of-work result ring, the 128-byte flag
 * words of a thread's side streams and the 4 bytes of the flag-synchronisation self-test, RCCL's own buffers.
 * A struct's leading struct_size is sizeof as the CALLER compiled it (like cm_comm): set it before the call; the library writes
 * at most that many bytes, and a size that does not cover the revision-9 fields is status 1. */
typedef struct {
  uint32_t struct_size, proofs_in_flight, peak_proofs_in_flight, reserved0;
  uint64_t live_bytes, reserved_bytes, peak_live_bytes, peak_reserved_bytes, pinned_host_bytes, driver_allocs, budget_bytes;
} cm_mem_stats;
/* host code; works before cm_init and without a GPU (all zero) */
int32_t cm_mem_stats_get(cm_mem_stats* out);
/* peaks := current values, driver_allocs := 0, peak_proofs_in_flight := proofs_in_flight */
int32_t cm_mem_reset_peak(void);
/* What ONE proof took, measured on the proving thread's own pool (for cm_prove_sharded: this rank's numbers).  Phases are those
 * of cm_proof_stats' phase_ms, same order and count.  A proof rebuilt by cm_proof_from_words reports zeros. */
typedef struct {
  uint32_t struct_size, n_phases;
  uint64_t start_live_bytes;        /* the proving thread's pool at entry: caches, blocks parked by the previous proof */
  uint64_t peak_live_bytes;         /* high-water mark of that pool during this proof */
  uint64_t peak_reserved_bytes;
  uint64_t input_bytes;             /* the cm_device_input it read (owned by another pool under cm_prove_many*) */
  uint64_t driver_allocs;           /* hipMalloc calls this proof caused */
  uint64_t phase_peak_live_bytes[32];   /* same order and count as cm_proof_stats' phase_ms */
} cm_proof_mem;
int32_t cm_proof_memory(const cm_proof* p, cm_proof_mem* out);
/* Estimate (host code, no GPU): a closed formula of the 34 component log sizes, the PCS config, `world` (1 = cm_prove_device,
 * 2 / 4 / 8 = one rank of cm_prove_sharded) and the memory-relevant switches in force (preprocessed / twiddle cache, deferred
 * teardown).  working_bytes is an UPPER BOUND of peak_live_bytes - start_live_bytes of a lone proof, monotone in every log size
 * and in log_blowup_factor; how tight it is is measured (tools/mem_report.py), not promised.  For world > 1 the bound does not
 * yet credit what sharding saves.  log sizes above 26, a blowup outside 1..4 or a world that is not 1, 2, 4 or 8 are status 1. */
typedef struct {
  uint32_t struct_size, reserved0;
  uint64_t input_bytes;     /* the resident cm_device_input */
  uint64_t working_bytes;   /* upper bound of peak_live_bytes - start_live_bytes of a lone proof */
  uint64_t cached_bytes;    /* what the preprocessed / twiddle caches and the parked teardown may hold between proofs */
} cm_mem_estimate;
int32_t cm_estimate_memory(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, cm_mem_estimate* out);
/* the same from the component log sizes alone (plan a max_steps without having an input): input_bytes is 0 */
int32_t cm_estimate_memory_logs(const uint32_t log_size[CM_N_COMPONENTS], const cm_pcs_config* config, uint32_t world,
                                cm_mem_estimate* out);
/* Budget for the pool's LIVE bytes, process-wide; 0 = none (default); env CM_MEMORY_BUDGET sets the initial value.  With a budget
 * cm_prove_many, cm_prove_many_host and cm_prove_many_segments admit work by bytes as well as by `inflight`: the next device
 * input is made, and the next proof started, only while resident inputs + the working_bytes of the proofs running + the new item
 * fit; a worker gives its parked teardown back before it waits and trims its pool when reserved_bytes is over the budget; when
 * nothing is running the next item is always admitted (no deadlock).  An item whose own input_bytes + working_bytes exceeds the
 * budget fails with status 2 and a message naming both numbers, before any GPU work for it (cm_prove_many_segments: before its
 * proof — its component sizes are only known once the device adapter has run); the other items are proved.  cm_prove_device,
 * cm_prove_segment and cm_prove_sharded apply that last rule only.  Order of outs and proof bytes never depend on the budget. */
int32_t cm_set_memory_budget(uint64_t bytes);
/* ---- device-side adapter -----------------------------------------------------------------
 * One runner segment in the runner's own terms: the VM trace, the memory access log and the memory at
 * segment start (crates/runner/src/vm/mod.rs:306-375, crates/common/src/execution.rs:28-66).
 * cm_adapt_segment_device = import_from_runner_output (crates/prover/src/adapter/mod.rs:97-193) with the
 * per-step work (previous-access tracking, clock updates, opcode bucketing) on the GPU; the result is the
 * device-resident ProverInput cm_prove_device consumes.  Same row order as the host adapter (cm_vm_run).
 * Every step's slice of the log is sized by the opcode the memory at segment start holds at its pc: a segment whose log shows
 * another opcode at a fetch (code stored over inside the segment) is refused by name (status 1), here and in a run. */
typedef struct {
  const uint32_t* trace;           /* (pc, fp) pairs: n_trace = steps + 1 entries */
  uint64_t n_trace;
  const uint32_t* memory_trace;    /* (address, v0, v1, v2, v3): 5 words per logged access, in execution order */
  uint64_t n_memory_trace;
  const uint32_t* initial_memory;  /* 4 words per cell: addresses 0 .. n_initial_memory-1 at segment start */
  uint64_t n_initial_memory;
  uint32_t program_range[2], input_range[2], output_range[2];
  /* (revision 6) the HEAP at segment start, 4 words per cell: index i = the cell at MAX_ADDRESS - i = 2^28 - 1 - i — the second
   * half of the reference's Segment::initial_memory (crates/runner/src/vm/mod.rs:205-221: `heap[i]` maps to MAX_ADDRESS - i;
   * the allocator of `new T[n]` grows it downwards).  Empty for a program's first segment; NULL / 0 when there is none. */
  const uint32_t* initial_heap;
  uint64_t n_initial_heap;
} cm_runner_segment;
int32_t cm_adapt_segment_device(const cm_runner_segment* seg, cm_device_input** out);
/* The host adapter (the sequential restatement of adapter/mod.rs:97-193 behind cm_vm_run) over a caller-supplied segment: the same
 * cm_host_input cm_vm_run returns, no GPU.  The log defines every step's opcode.  Status 1 for the input errors of
 * cm_adapt_segment_device, with its messages (empty trace, invalid opcode, a memory trace whose length does not match the
 * instructions executed, a step whose first entry is not the fetch at pc, overlapping regions). */
int32_t cm_adapt_segment_host(const cm_runner_segment* seg, cm_host_input** out);
/* streaming ingest from runner segments: see cm_prove_many_host */
int32_t cm_prove_many_segments(const cm_runner_segment* const* segments, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                               cm_proof** outs);
/* ---- a whole run (revision 10) ----------------------------------------------------------------------------------------
 * The reference cuts a run into segments at max_steps and chains them by public data: segment i's final registers and final
 * memory root are segment i + 1's initial ones (crates/prover/tests/prover.rs:198-243, public_data.rs:192-227).  A cm_run keeps
 * the program's memory ON THE DEVICE between segments, so a segment brings only its trace and its memory log; the image is
 * uploaded once (cm_run_begin) and lives in the device pool of the thread that made it (cm_mem_stats counts it).
 *
 * cm_run_begin: the memory at the start of the run — locals dense from address 0, heap dense from MAX_ADDRESS downwards (the two
 * arrays of cm_runner_segment; NULL / 0 for none) — and ranges = program, input, output [start, end).
 * cm_run_adapt_next: the same cm_device_input cm_adapt_segment_device makes for this segment with this memory at its start; then
 * the image advances to the memory at the segment's end: each region grows to the given end length (the lengths of the runner's
 * two vectors when the segment ends), a touched cell inside a region takes its last logged value, an untouched one keeps its
 * value (zero where the region grew over it), a touched cell outside both regions is a read of an untouched cell and is not
 * carried.  Status 1, with the run left as it was: an end length below the current one; regions that overlap; a touched cell
 * outside both regions whose last value is not zero; every input error of cm_adapt_segment_device.
 * The boundary memory, both partial Merkle trees (from CM_ADAPTER_DEVICE_TREE_MIN rows up, default 2048; below it the rows are
 * downloaded and hashed on the host), the public entries and the advance are built on the calling thread's stream: no
 * NULL-stream copy, no device-wide wait; three host round trips with data per segment and one wait behind the tree nodes'
 * copy or upload.
 * cm_run_memory: the image as it is now; n_l / n_h always receive the lengths, an array is filled when it is not NULL (status 1
 * when its capacity, in cells, is too small).  Calls on one run are serialised; they may come from different threads. */
typedef struct cm_run cm_run;
typedef struct {
  const uint32_t* trace;           /* as cm_runner_segment */
  uint64_t n_trace;
  const uint32_t* memory_trace;
  uint64_t n_memory_trace;
  uint64_t n_memory_end, n_heap_end;   /* cells in the runner's locals / heap vectors when the segment ends */
} cm_run_segment;
int32_t cm_run_begin(const uint32_t* initial_memory, uint64_t n_initial_memory, const uint32_t* initial_heap, uint64_t n_initial_heap,
                     const uint32_t ranges[6], cm_run** out);
int32_t cm_run_adapt_next(cm_run* r, const cm_run_segment* seg, cm_device_input** out);
int32_t cm_run_memory(const cm_run* r, uint32_t* locals, uint64_t cap_l, uint64_t* n_l, uint32_t* heap, uint64_t cap_h, uint64_t* n_h);
int32_t cm_run_free(cm_run* r);
/* The next n segments of the run, proved: the calling thread adapts them in order (the image is serial) while up to `inflight`
 * library workers prove.  Error contract, order of outs, memory-budget admission as cm_prove_many_segments; at most inflight + 1
 * inputs are resident.  A segment that cannot be adapted fails the call, leaves the image at that segment's start and stops the
 * ingest; the run may be continued by a later cm_prove_run or cm_run_adapt_next. */
int32_t cm_prove_run(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                     cm_proof** outs);
/* A proof's public data (public_data.rs:192-227).  Set struct_size = sizeof(cm_public_data) before the call. */
typedef struct {
  uint32_t struct_size, reserved0;
  uint32_t initial_pc, initial_fp, final_pc, final_fp, clock, initial_root, final_root;
  uint32_t n_program, n_input, n_output;   /* public entries: one per address of each range */
} cm_public_data;
int32_t cm_proof_public_data(const cm_proof* p, cm_public_data* out);
/* which: 0 program, 1 input, 2 output.  *n_entries always receives the count; out (NULL = count only) receives seven words per
 * entry: present, address, value[4], clock (all zero where the boundary memory has no such cell). */
int32_t cm_proof_public_entries(const cm_proof* p, uint32_t which, uint32_t* out, uint64_t cap_entries, uint64_t* n_entries);
/* The same entries, read from a device input (they are what its proof will carry): contract of cm_proof_public_entries.  The data
 * is held in host memory: no GPU work. */
int32_t cm_device_input_public_entries(const cm_device_input* in, uint32_t which, uint32_t* out, uint64_t cap_entries, uint64_t* n_entries);
/* Host code, no GPU: every proof passes cm_verify_proof, and for every i > 0 the initial pc, fp and memory root of proof i equal
 * the final ones of proof i - 1.  Status 11; the message names the link and the field, e.g.
 * "run: segment 3 initial_root != segment 2 final_root", or "run: segment 3: verification failed: ...". */
int32_t cm_verify_run(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected);
/* ---- batched verification on the GPU (additive to revision 10) -------------------------------------------------------------
 * cm_verify_many verifies n independent proofs in one batch.  Per proof the host replays the transcript and does every check in
 * front of the queries (cm_verify_proof's own code), then plans the query phase as flat tables; the GPU computes the DEEP-quotient
 * answers, folds the FRI layers and hashes every decommitment path of every tree of every proof (one upload, four launches on
 * stream s, one download).  There is no CPU fallback: without a GPU the status is cm_init's (3).  The verdict and the words are
 * the host verifier's: results[i].status / message equal what cm_verify_proof(proofs[i], expected) returns and leaves in
 * cm_last_error() — the EARLIEST failed check in the host's order, whose id (below, numbered in that order) is results[i].check.
 * Returns 0 when every proof is accepted; otherwise 11 and cm_last_error() reads "proof <i>: <message>" for the lowest rejected
 * i.  n == 0, a null array or a null proof: status 1.  The framing in force (cm_set_framing) is honoured.  The call keeps
 * nothing: its device buffers come from the calling thread's pool and are back there when it returns.  A level of one tree
 * holds at most 1024 nodes on the device (that is n_queries <= 512); more is status 1. */
#define CM_VERIFY_STRUCTURE 1            /* InvalidStructure..., config and shape */
#define CM_VERIFY_POW_INTERACTION 2      /* ProofOfWork(interaction) */
#define CM_VERIFY_LOGUP_SUM 3            /* InvalidLogupSum */
#define CM_VERIFY_OODS 4                 /* OodsNotMatching */
#define CM_VERIFY_FRI_STRUCTURE 5        /* Fri(InvalidNumFriLayers), Fri(LastLayerDegreeInvalid) */
#define CM_VERIFY_POW 6                  /* ProofOfWork */
#define CM_VERIFY_MERKLE 7               /* Merkle(tree 0..3): ... */
#define CM_VERIFY_QUERIED_VALUES 8       /* InvalidStructure(queried values) */
#define CM_VERIFY_FRI_FIRST_EVALS 9      /* Fri(FirstLayerEvaluationsInvalid) */
#define CM_VERIFY_FRI_FIRST_COMMITMENT 10 /* Fri(FirstLayerCommitmentInvalid): ... */
#define CM_VERIFY_FRI_INNER_EVALS 11     /* Fri(InnerLayerEvaluationsInvalid), layer by layer in front of ... */
#define CM_VERIFY_FRI_INNER_COMMITMENT 12 /* ... Fri(InnerLayerCommitmentInvalid <i>): ... of the same layer */
#define CM_VERIFY_FRI_LAST_EVALS 13      /* Fri(LastLayerEvaluationsInvalid) */
typedef struct cm_verify_result {
  int32_t status;      /* 0 = accepted, 11 = rejected (same code cm_verify_proof returns) */
  int32_t check;       /* 0, or the CM_VERIFY_* id of the failed check */
  char    message[160];/* exactly the string the host verifier gives for this proof, NUL-terminated */
} cm_verify_result;
int32_t cm_verify_many(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_result* results,
                       cm_stream_t s);
/* cm_verify_many plus the register / root chain check of cm_verify_run, with cm_verify_run's messages. */
int32_t cm_verify_run_device(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected);
/* Where the calling thread's last cm_verify_many / cm_verify_run_device spent its time, in milliseconds: 0 host planning,
 * 1 upload, 2 kernels, 3 download of the result words (1-3 from events on the stream). */
int32_t cm_verify_many_timing(double ms[4]);
/* The shapes of the plan cm_verify_many would launch for each proof ALONE, read back from the tables its planner built (host
 * code, works without a GPU; the tests read it to prove that a config reaches a kernel's second stride trip or the LDS limit).
 * Set out[i].struct_size = sizeof(cm_verify_stats) before the call.  A proof decided in front of the queries reports its
 * CM_VERIFY_* id in early_check and zeros elsewhere.  A proof wider than the device limit still gets its stats: the refusal
 * stays with cm_verify_many.  Development aid: with CM_VERIFY_PLAN_MARKS=1 in the environment the call also prints one line per
 * proof on stderr, how its planning time splits into replay and host checks, public LogUp sum, OODS evaluation and tables
 * (tools/verify_bench.py --plan-split); nothing else reads the switch. */
typedef struct cm_verify_stats {
  uint32_t struct_size;
  int32_t  early_check;        /* 0, or the CM_VERIFY_* id of the check that failed in front of the queries */
  uint32_t n_answer_jobs;      /* workgroups of the answers kernel: one per (size group, query row) */
  uint32_t max_batch_entries;  /* the largest number of entries in one sample batch */
  uint32_t max_first_pairs;    /* the largest pair count of a first-layer size group */
  uint32_t max_inner_pairs;    /* the largest pair count of an inner FRI layer */
  uint32_t max_level_nodes;    /* the widest level of any tree, in nodes */
  uint32_t merkle_lds_bytes;   /* dynamic LDS the Merkle launch would ask for: 2 * max_level_nodes * 32 */
  uint32_t n_tree_jobs;        /* workgroups of the Merkle kernel: one per tree */
  uint32_t n_slots;            /* checks of the query phase, planned ones included */
  uint64_t blob_words, scratch_words;
} cm_verify_stats;
int32_t cm_verify_plan_stats(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_stats* out);
/* cm_verify_many — the same plan, the same launches, the same verdicts in results (may be NULL) — that also hands back every
 * proof's slots in the host verifier's order: the slots of proof i are slots[slot_first[i] .. slot_first[i + 1]) (slot_first
 * has n + 1 entries and is filled whenever the batch ran; a proof decided in front of the queries has none).  When
 * slot_first[n] > cap_slots nothing is written to slots and the status is 1: call again with that many.  One more download than cm_verify_many: the flag words next to the verdicts.
 * The call's status and cm_last_error() are cm_verify_many's. */
typedef struct cm_verify_slot {
  int32_t  check;        /* CM_VERIFY_* id of this slot's check */
  uint32_t on_device;    /* 1: a kernel decides it (a tree's root, the last layer's evaluations); 0: it failed while planning */
  uint32_t raised;       /* 1: this check failed — on its own, whatever the slots in front of it say */
  char     message[116]; /* what the host verifier says when this check is the first to fail, NUL-terminated */
} cm_verify_slot;
int32_t cm_verify_many_detail(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_result* results,
                              cm_verify_slot* slots, uint32_t cap_slots, uint32_t* slot_first, cm_stream_t s);
/* ---- the prelude's arithmetic on the GPU (additive to revision 10) -----------------------------------------------------------
 * Two checks in front of the queries are pure field arithmetic whose outcome the transcript does not depend on: the public LogUp
 * sum (InvalidLogupSum: one QM31 inverse per register / root term and five per present public entry) and the OODS composition
 * check (OodsNotMatching: all 34 components evaluated over the sampled mask values).  With CM_VERIFY_ARITH_ON_DEVICE in `flags`
 * the host skips both while it replays the transcript and the device decides them: they become the FIRST TWO slots of the proof,
 * CM_VERIFY_LOGUP_SUM then CM_VERIFY_OODS, each with its own flag word, in front of the four tree slots, decided by six more
 * launches (k_verify_public_sum, k_verify_oods once per component group, k_verify_prelude_fin; the number depends on neither the
 * batch nor the public entries) in front of k_verify_reduce: same stream, same upload, same single download.  The verdict rule is unchanged (the lowest raised or failed slot), and so are the verdicts and words.
 * A host check that fails in front of the LogUp sum (config, structure, ProofOfWork(interaction)) still decides the proof early
 * and sends nothing.  A host check that fails behind a deferred one (the sampled values' shape, Fri(InvalidNumFriLayers),
 * Fri(LastLayerDegreeInvalid), ProofOfWork) becomes a planned slot behind the deferred slots, which still run: they may be the
 * earlier failure.  The sampled values' shape sits between the two: the LogUp slot goes out and the OODS slot does not.
 * flags == 0: exactly cm_verify_many / cm_verify_many_detail / cm_verify_run_device.  An unknown flag bit: status 1.
 * cm_verify_many_timing reports the same four fields after either. */
/* (a flag bit, not a check id: set apart from the CM_VERIFY_<check> <id> list above by its alignment) */
#define CM_VERIFY_ARITH_ON_DEVICE   1u
int32_t cm_verify_many_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags,
                          cm_verify_result* results, cm_stream_t s);
int32_t cm_verify_many_detail_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags,
                                 cm_verify_result* results, cm_verify_slot* slots, uint32_t cap_slots, uint32_t* slot_first, cm_stream_t s);
int32_t cm_verify_run_device_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags);
/* Op-level entries: the same kernels on inputs the caller chooses, each with a host twin that calls the host verifier's own
 * function (initial_logup_sum, point_eval) and nothing else.  Every argument is checked on the host before any launch (status 1
 * and a message): null pointers, n_jobs outside 1..65536, a list longer than 2^24 entries, a component id outside 0..33, counts
 * that differ from cm_component_info's, `present` above 1 and any field word not below P.
 * cm_public_logup_sum_op: out = 4 words per job, initial_logup_sum of the job's public data under rel_words (k_verify_public_sum,
 * one workgroup per CM_PUBLIC_SUM_ENTRIES entries of a list, then k_verify_prelude_fin).  An entry with present == 0 is
 * skipped; a zero denominator contributes nothing, as inv(0) = 0 does on the host. */
#define CM_PUBLIC_SUM_ENTRIES 256u
#define CM_RELATIONS_WORDS (4u * CM_N_RELATIONS * (1u + CM_MAX_RELATION_SIZE))
typedef struct cm_public_sum_job {
  uint32_t head[7];          /* initial_pc, initial_fp, final_pc, final_fp, clock, initial_root, final_root */
  uint32_t n_program, n_input, n_output;
  const uint32_t* entries;   /* 7 words per entry (present, addr, value[4], clock): program, then input, then output; may be
                              * NULL when all three counts are 0 */
  const uint32_t* rel_words; /* CM_RELATIONS_WORDS words in cm_relations' layout */
} cm_public_sum_job;
int32_t cm_public_logup_sum_op(const cm_public_sum_job* jobs, uint32_t n_jobs, cm_stream_t s, uint32_t* out);
int32_t cm_public_logup_sum_host(const cm_public_sum_job* job, uint32_t out4[4]);
/* cm_point_eval_op: out = 4 words per job, sum_k coeff[k] * C_k of component `component` at the mask values (k_verify_oods, one
 * lane per job, in job order).  tr: one QM31 per trace column; it: one QM31 per interaction column and a second one ([-1, 0]
 * mask, previous row first) for each of the last four; pp: CM_N_PREPROCESSED QM31; coeff: one QM31 per constraint, base
 * constraints first.  n_*_words count uint32 words (4 per QM31). */
typedef struct cm_point_eval_job {
  uint32_t component, n_tr_words, n_it_words, n_coeff_words;
  const uint32_t *tr, *it, *pp, *rel_words, *coeff;
  uint32_t shift[4];         /* the cumulative-sum shift, claimed_sum / 2^log_size */
} cm_point_eval_job;
int32_t cm_point_eval_op(const cm_point_eval_job* jobs, uint32_t n_jobs, cm_stream_t s, uint32_t* out);
int32_t cm_point_eval_host(const cm_point_eval_job* job, uint32_t out4[4]);
/* (Checking a whole run BEFORE proving it — cm_link_diff, cm_check_chain, cm_check_run — is declared behind the relation tracker
 * below: its records embed cm_check_report.) */
/* Copy a device-resident ProverInput back (tests: device adapter vs host adapter). */
int32_t cm_device_input_download(const cm_device_input* in, cm_host_input** out);
/* The synthetic VM's raw output for one segment (what cm_vm_run feeds to the host adapter). */
typedef struct cm_host_segment cm_host_segment;
int32_t cm_vm_segment(const uint32_t* instr_words, const uint32_t* instr_lens, uint32_t n_instr, uint32_t entry_pc,
                      const uint32_t* args, uint32_t n_args, uint32_t n_returns, uint64_t max_steps,
                      uint32_t segment_index, cm_host_segment** out, uint32_t* n_segments_out);
int32_t cm_synth_fibonacci_segment(uint32_t n, uint64_t max_steps, uint32_t segment_index, cm_host_segment** out);
const cm_runner_segment* cm_host_segment_view(const cm_host_segment* h);
/* (revision 10) cells in the synthetic VM's locals / heap vectors when the segment ended: cm_run_segment.n_memory_end / n_heap_end
 * (a segment built from artifacts reports its initial lengths) */
int32_t cm_host_segment_end_lengths(const cm_host_segment* h, uint64_t* n_memory_end, uint64_t* n_heap_end);
/* Runner artifact wire formats (crates/common/src/execution.rs:28-66, crates/prover/src/adapter/io.rs:38-80):
 * trace = (fp, pc) little-endian u32 pairs; memory trace = [u32 program_length header] + (address, v0..v3)
 * records.  out == NULL only reports *len.  The reference does not serialise the initial memory and the public
 * ranges (adapter/mod.rs:215-237): cm_segment_from_artifacts takes them from the caller
 * (ranges = program, input, output [start, end)). */
int32_t cm_segment_serialize_trace(const cm_runner_segment* s, uint8_t* out, uint64_t cap, uint64_t* len);
int32_t cm_segment_serialize_memory_trace(const cm_runner_segment* s, int32_t with_header, uint8_t* out, uint64_t cap, uint64_t* len);
int32_t cm_segment_from_artifacts(const uint8_t* trace, uint64_t trace_len, const uint8_t* mem, uint64_t mem_len,
                                  int32_t mem_has_header, const uint32_t* initial_memory, uint64_t n_initial_memory,
                                  const uint32_t ranges[6], cm_host_segment** out);
/* (revision 6) the heap cells of a segment built from artifacts (copied; see cm_runner_segment.initial_heap) */
int32_t cm_host_segment_set_initial_heap(cm_host_segment* h, const uint32_t* initial_heap, uint64_t n_initial_heap);
int32_t cm_host_segment_free(cm_host_segment* h);
/* ---- per-component AIR ops --------------------------------------------------------------------
 * What the reference does per component through Rust generics that name SimdBackend — and therefore cannot be
 * reached through Stwo's Backend traits — on caller-owned device columns (cm_handle = u32[2^log_size]):
 *   cm_trace_write            = <component>::Claim::write_trace (e.g. opcodes/store_fp_imm.rs:147-296, memory.rs:93-195,
 *                               merkle.rs:92-201, clock_update.rs:77-166, poseidon2.rs:172-325)
 *   cm_histogram              = range_check_N / bitwise Claim::write_trace multiplicities
 *                               (preprocessed/range_check/range_check_macro.rs:62-112, preprocessed/bitwise.rs:72-157)
 *   cm_preprocessed_column    = PreProcessedTrace::gen_trace columns (preprocessed/mod.rs:36-38, bitwise.rs:283-319)
 *   cm_interaction_write      = <component>::InteractionClaim::write_interaction_trace + LogupTraceGenerator::finalize_last
 *   cm_constraints_accumulate = FrameworkComponent::evaluate_constraint_quotients_on_domain of <component>::Eval
 * Component ids: 0..25 = opcode components in the order of define_opcodes! (opcodes/mod.rs:223-268), then memory 26,
 * merkle 27, clock_update 28, poseidon2 29, range_check_8/16/20 30..32, bitwise 33.  The whole-segment prover runs the
 * same kernels. */
#define CM_N_RELATIONS 8
#define CM_MAX_RELATION_SIZE 16
#define CM_N_PREPROCESSED 7
/* Relations::draw (components/mod.rs:311-323): z and the powers alpha^0.. of every relation, QM31 as 4 words */
typedef struct {
  uint32_t z[CM_N_RELATIONS][4];
  uint32_t alpha_pow[CM_N_RELATIONS][CM_MAX_RELATION_SIZE][4];
} cm_relations;
int32_t cm_component_info(int32_t component, uint32_t* n_trace_cols, uint32_t* n_interaction_cols, uint32_t* n_constraints);
/* log size of the component's trace for this input: max(4, ceil_log2(rows)) — fixed 8/16/20/18 for the lookup tables */
int32_t cm_component_log_size(const cm_device_input* input, int32_t component, uint32_t* log_size);
/* components 0..29; cols = n_trace_cols columns of 2^log_size (padding rows included) */
int32_t cm_trace_write(const cm_device_input* input, int32_t component, const cm_handle* cols, cm_stream_t s);
/* adds the lookups of one opcode component's trace (padding rows included) to the four multiplicity columns
 * (2^8, 2^16, 2^20, 2^18 words, zeroed by the caller); an out-of-range value is status 1 */
int32_t cm_histogram(int32_t component, const cm_handle* trace_cols, uint32_t log_size, cm_handle rc8, cm_handle rc16,
                     cm_handle rc20, cm_handle bitwise, cm_stream_t s);
/* preprocessed column id 0..6 (bitwise op / a / b / result, range_check_8, _16, _20) on its trace domain */
int32_t cm_preprocessed_column(int32_t id, cm_handle col, cm_stream_t s);
/* trace_cols / preprocessed: trace-domain columns (preprocessed = all CM_N_PREPROCESSED columns);
 * out = n_interaction_cols columns; claimed_sum = the component's InteractionClaim */
int32_t cm_interaction_write(int32_t component, const cm_handle* trace_cols, const cm_handle* preprocessed, uint32_t log_size,
                             const cm_relations* relations, const cm_handle* out, uint32_t claimed_sum[4], cm_stream_t s);
/* *_lde: the component's columns evaluated on CanonicCoset(log_size + 1) (cm_interpolate + cm_evaluate), preprocessed_lde
 * likewise (column k on CanonicCoset(its log + 1)); coeff_powers = the random-coefficient powers of this component's
 * n_constraints constraints, 4 words each, in constraint order; acc += sum_k coeff_k * C_k / vanishing */
int32_t cm_constraints_accumulate(int32_t component, const cm_handle* trace_lde, const cm_handle* interaction_lde,
                                  const cm_handle* preprocessed_lde, uint32_t log_size, const cm_relations* relations,
                                  const uint32_t* coeff_powers, const uint32_t claimed_sum[4], const cm_handle acc[4],
                                  cm_stream_t s);
/* ---- PCS-free AIR check (reference: debug_tools::assert_constraints; the per-relation sums of the report tell WHICH relation does
 * not balance, cm_track_relations below is the reference's relation tracker and tells which tuples) ---------------------------
 * Builds the three traces of a segment on their trace domains only (no twiddles, LDE, Merkle trees or FRI), draws the relations
 * (from a default channel unless the caller passes them), and checks that every constraint of every component vanishes on every
 * row and that the LogUp sums cancel.  Verdict, in the order of precedence:
 *   status 1  a range-check / bitwise lookup value is out of range: message "lookup value out of range for <rc8|rc16|rc20|bitwise>: ..."
 *   status 2  the lowest component id with a failing row: "<ComponentName>: constraint <k> fails on row <r>" (r = lowest failing
 *             row in column storage order, k = lowest failing constraint on that row: base constraints first, then LogUp)
 *   status 3  the LogUp sums do not cancel: "LogUp sums do not cancel: <names of the relations whose sum is not zero>"
 *   status 0  none of the above
 * Relation ids (relation_sum / public_sum): 0 registers, 1 memory, 2 merkle, 3 poseidon2, 4 range_check_8, 5 range_check_16,
 * 6 range_check_20, 7 bitwise.  For every component c, sum_r relation_sum[c][r] = claimed_sum[c]; the segment balances when
 * sum_c relation_sum[c][r] + public_sum[r] = 0 for every r, and total = sum_c claimed_sum[c] + sum_r public_sum[r]. */
typedef struct {
  int32_t status;                      /* 0 ok, 1 lookup out of range, 2 constraint fails, 3 LogUp sums do not cancel */
  int32_t component, constraint;       /* status 1: component (constraint = table: 0 rc8, 1 rc16, 2 rc20, 3 bitwise); 2: as named; else -1 */
  int32_t reserved;                    /* keeps `row` 8-byte aligned without implicit padding */
  uint64_t row;                        /* status 1 / 2: the row named in the message */
  uint64_t failing_rows[CM_N_COMPONENTS];
  int32_t first_constraint[CM_N_COMPONENTS];   /* -1 = none */
  uint64_t first_row[CM_N_COMPONENTS];
  uint32_t claimed_sum[CM_N_COMPONENTS][4];
  uint32_t relation_sum[CM_N_COMPONENTS][CM_N_RELATIONS][4];
  uint32_t public_sum[CM_N_RELATIONS][4];
  uint32_t total[4];
  cm_relations relations;              /* the relations the check used */
  char message[256];
} cm_check_report;
/* relations NULL = drawn from a default channel (debug_tools/assert_constraints.rs:42).  Returns 0 when the check ran (the verdict
 * is in the report), non-zero when it could not run (cm_last_error).  Threading as cm_prove_device: the calling thread's stream
 * and device pool. */
int32_t cm_check_constraints(const cm_device_input* input, const cm_relations* relations, cm_check_report* out);
/* op level, beside cm_constraints_accumulate: the trace-domain columns of one component (preprocessed = all CM_N_PREPROCESSED
 * columns on their trace domains), claimed_sum = its InteractionClaim.  row_status (0 = none): a column of 2^log_size words that
 * receives the lowest failing constraint of every row, 0xFFFFFFFF = none.  first_constraint = -1 when no row fails. */
int32_t cm_constraints_check(int32_t component, const cm_handle* trace_cols, const cm_handle* interaction_cols,
                             const cm_handle* preprocessed, uint32_t log_size, const cm_relations* relations,
                             const uint32_t claimed_sum[4], cm_handle row_status, uint64_t* failing_rows, int32_t* first_constraint,
                             uint64_t* first_row, cm_stream_t s);
/* sums[r] = sum over the component's rows and its entries of relation r of multiplicity / (sum_i alpha_r^i v_i - z_r) */
int32_t cm_relation_sums(int32_t component, const cm_handle* trace_cols, const cm_handle* preprocessed, uint32_t log_size,
                         const cm_relations* relations, uint32_t sums[CM_N_RELATIONS][4], cm_stream_t s);
/* ---- relation tracker (reference: debug_tools/relation_tracker.rs, RelationSummary::summarize_relations(..).cleaned()) --------
 * An entry is one add_to_relation(relation, multiplicity, values) of a component on one trace-domain row (padding rows included;
 * zero multiplicities contribute nothing), and for a whole segment also one term of the verifier's public-data LogUp sum
 * (registers [pc, fp, 1] +1 and [pc, fp, clock + 1] -1, the two Merkle root tuples, per public memory cell one memory tuple and
 * four Merkle leaf tuples).  Two entries are the same tuple when they belong to the same relation and their values are equal after
 * removing trailing zeros (the LogUp denominator cannot see those).  The summary lists the tuples whose multiplicities do not sum
 * to zero modulo P.  Tuples are grouped by their LogUp denominator under the relations of the call: two different tuples of one
 * relation are merged with probability <= 16 / |QM31| ~ 2^-120 over drawn relations; degenerate caller-supplied relations
 * (alpha = 0) merge tuples exactly as they blind the sum check. */
typedef struct {
  uint32_t relation;                 /* 0..7, the relation ids of cm_check_report */
  uint32_t multiplicity;             /* net, canonical M31, never 0 (a consumer's -1 is P - 1) */
  uint32_t n_values;                 /* after removing trailing zeros, 0..CM_MAX_RELATION_SIZE */
  uint32_t first_component;          /* lowest (component, row) merged in; CM_N_COMPONENTS = public data (row 0) */
  uint64_t first_row;
  uint64_t n_entries;                /* entries merged into this tuple (zero multiplicities not counted) */
  uint32_t values[CM_MAX_RELATION_SIZE];   /* zero beyond n_values */
} cm_relation_entry;
/* Whole segment: runs the passes of cm_check_constraints (report, optional, receives its verdict; the tracker runs whatever the
 * verdict is), then the tracker.  relations NULL = drawn from a default channel, as the check.  relation_mask 0 = the relations
 * whose sums do not cancel (a valid segment costs the check and nothing more); bit r set = track relation r regardless.
 * entries[0, min(*n_total, cap)) are written; *n_total > cap means truncated, which is not an error (entries may be NULL when
 * cap is 0).  Order: by relation id, then by the grouping key's words: deterministic for given input and relations.  The record
 * buffers (88 bytes per entry of the largest tracked relation) come from the calling thread's device pool; when it cannot supply
 * them the call fails with a message naming the bytes.  Threading as cm_check_constraints. */
int32_t cm_track_relations(const cm_device_input* input, const cm_relations* relations, uint32_t relation_mask,
                           cm_check_report* report, cm_relation_entry* entries, uint64_t cap, uint64_t* n_total);
/* op level, beside cm_relation_sums: the summary of ONE component's columns (no public data); relation_mask 0 = all 8 */
int32_t cm_relation_entries(int32_t component, const cm_handle* trace_cols, const cm_handle* preprocessed, uint32_t log_size,
                            const cm_relations* relations, uint32_t relation_mask, cm_relation_entry* entries, uint64_t cap,
                            uint64_t* n_total, cm_stream_t s);
/* ---- a whole run, checked before it is proved (additive to revision 10: new symbols and structs, nothing moved) ---------------
 * A run can be invalid in a way no single-segment check sees: its LINKS.  A segment that first-writes a cell beyond the memory it
 * was handed enters that cell into its initial tree with the written value (adapter/memory.rs:493-503), so its initial root is
 * not its predecessor's final root, and cm_verify_run refuses the proved run naming two 31-bit roots.  cm_link_diff names the
 * cells instead, from the two device inputs, without proving anything.
 *
 * cm_link_diff compares prev's FINAL boundary memory with next's INITIAL boundary memory (both in ascending address order, both
 * stay where they are) on the calling thread's stream and pool (threading as cm_check_constraints).  Only the four value words of
 * a cell are leaves of the partial Merkle tree; clocks and multiplicities are not compared.  An absent leaf hashes like a zero
 * leaf (adapter/merkle.rs: missing nodes take the default hash of their depth, and the default leaf is 0), so a cell present on
 * one side only with value (0, 0, 0, 0) does not change the root: such cells are counted in n_zero_only and are NOT listed.
 * Contract, for inputs whose roots belong to their memories: roots_equal <=> *n_total == 0.
 * cells[0, min(*n_total, cap)) are written in ascending address order; *n_total > cap means truncated, which is not an error;
 * cells may be NULL when cap is 0.  The result is deterministic: its order comes from addresses and a scan.
 * message: first the sentence cm_verify_run would give for this link — for the first field that differs, initial_pc, then
 * initial_fp, then initial_root ("run: segment 1 initial_root != segment 0 final_root"; cm_link_diff numbers prev 0 and next 1,
 * cm_check_run / cm_check_chain use the segments' own indices), nothing when all three are equal — then, when cells are listed,
 * ". <n> cells differ: <a> changed, <b> new, <c> gone; first address <x>" (without the ". " when the first sentence is empty).
 * Without a GPU the status is cm_init's (3).  Set struct_size = sizeof(cm_link_report) before cm_link_diff. */
typedef struct {
  uint32_t kind;            /* 1 present in both, values differ; 2 present only in next's initial memory; 3 only in prev's final memory */
  uint32_t address;
  uint32_t prev_value[4];   /* zero for kind 2 */
  uint32_t next_value[4];   /* zero for kind 3 */
  uint32_t prev_clock;      /* clock of prev's final row (the last access of the cell in prev); zero for kind 2 */
} cm_link_cell;             /* sizeof = 44 */
typedef struct {
  uint32_t struct_size, reserved0;
  uint32_t prev_final_pc, prev_final_fp, next_initial_pc, next_initial_fp;
  uint32_t pc_equal, fp_equal, roots_equal, reserved1;
  uint32_t prev_final_root, next_initial_root;
  uint64_t n_changed, n_only_next, n_only_prev;   /* totals of kind 1, 2, 3: their sum is *n_total */
  uint64_t n_zero_only;                           /* present on one side only, all-zero value: not listed */
  char message[160];
} cm_link_report;           /* sizeof = 240 */
int32_t cm_link_diff(const cm_device_input* prev, const cm_device_input* next, cm_link_report* report, cm_link_cell* cells, uint64_t cap,
                     uint64_t* n_total);
/* One record per segment of a checked run: the AIR verdict of segment i (cm_check_constraints' report; all zero from
 * cm_check_chain), the link between segment i - 1 and i (all zero for i = 0; struct_size is set by the library), and how many of
 * the link's cells were written to cells[i * cap_per_link ...] out of how many there are. */
typedef struct {
  cm_check_report check;
  cm_link_report link;
  uint64_t link_cells_written, link_cells_total;
} cm_run_check;             /* sizeof = sizeof(cm_check_report) + 240 + 16 = 8432 */
/* The links of n segments adapted one by one (cm_adapt_segment_device, cm_input_upload): out = n records, cells = n * cap_per_link
 * cells (NULL when cap_per_link is 0).  Returns 0 when the call ran; the verdicts are in out, and cm_last_error() holds a one-line
 * summary of the first bad link ("link 3: run: segment 3 initial_root != ...") or is empty. */
int32_t cm_check_chain(const cm_device_input* const* inputs, uint32_t n, cm_run_check* out, cm_link_cell* cells, uint64_t cap_per_link);
/* The next n segments of a run, checked instead of proved.  Segment i goes through cm_run_adapt_next (the image advances exactly
 * as under cm_prove_run), then the passes of cm_check_constraints run on its input (relations as there: NULL = drawn from a
 * default channel), then, for i > 0, cm_link_diff against segment i - 1's input, which is kept until then and freed after: at most
 * two inputs are resident.  The call does NOT stop at a bad verdict: it returns 0 when it ran, out holds every verdict, and
 * cm_last_error() holds a one-line summary of the first bad link or segment in run order ("link 2: ...", "segment 2: ...") or is
 * empty.  It does stop at a segment that cannot be adapted, with cm_run_adapt_next's own status and contract: the records in
 * front of it are filled, the image is left at that segment's start, and the run may be continued from there. */
int32_t cm_check_run(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_relations* relations, cm_run_check* out,
                     cm_link_cell* cells, uint64_t cap_per_link);
/* ---- memory openings (additive to revision 10: new symbols and one struct, nothing moved) --------------------------------------
 * A memory root commits to every cell; an opening is one cell's value plus its authentication path, checkable without the
 * memory: a heap result outside the output range, a checkpoint image shown to be the one the proofs end in, one cell for a bridge.
 * The tree (adapter/merkle.rs:183-295) has height 30: cell a < 2^28 owns the leaves 4a .. 4a + 3, the four words of its value;
 * h29_0 = H(v0, v1), h29_1 = H(v2, v3), n28 = H(h29_0, h29_1) is the node of depth 28 with index a; above it there is one sibling
 * per depth 28 .. 1 (at depth d the path's node has index a >> (28 - d) and is the right child when that index is odd).  A node
 * the tree does not hold is the default hash of its depth (default[30] = 0, default[d] = H(default[d + 1], default[d + 1])), so the
 * root is a function of the non-zero cells only: an absent cell opens as the value (0, 0, 0, 0), and a cell the tree holds with
 * that value may be claimed with present = 1 or 0 alike.  Multiplicities enter no hash.
 *
 * cm_input_open_memory / cm_run_open_memory build out[i] = the opening of addresses[i] on the GPU, on the calling thread's stream
 * and pool (threading as cm_link_diff): the addresses go up, two launches bisect the tree's node list (ordered by depth 30 .. 1,
 * then by index), the records come back: one host round trip per call.  Addresses may repeat and come in any order; the same
 * call gives the same bytes.  n == 0 is status 0 (out may be NULL) and *root is still written.  Status 1, with nothing written
 * to out: an address >= 2^28, which > 1, a NULL argument, a run whose image is empty.  Without a GPU the status is cm_init's (3).
 * cm_verify_memory_openings recomputes the 31 hashes of every record on the GPU, one lane per record (upload, one launch,
 * download on stream s; 0 = the calling thread's own stream): ok[i] = 1 when record i hashes to `root`.  A record with an address
 * >= 2^28, present > 1, a word >= P, or present = 0 with a non-zero value gets ok[i] = 0; it does not fail the call.
 * cm_verify_memory_opening is the same check of one record in host code, for a light client: it needs no GPU. */
typedef struct {
  uint32_t address;
  uint32_t present;         /* 1: the tree holds the cell; 0: absent, value is (0, 0, 0, 0) */
  uint32_t value[4];
  uint32_t siblings[28];    /* siblings[k] = the sibling at depth 28 - k */
} cm_mem_opening;           /* sizeof = 136 */
/* which: 0 = the input's initial tree, 1 = its final tree.  *root receives that tree's root. */
int32_t cm_input_open_memory(const cm_device_input* in, uint32_t which, const uint32_t* addresses, uint64_t n, cm_mem_opening* out,
                             uint32_t* root);
/* Under the root of the run's image as it is now (= the final root of the last adapted segment = the initial root of the next).
 * The image's tree is built on first use (every image cell through the device tree builder: one more round trip and one wait)
 * and dropped, not rebuilt, when the image advances; cm_mem_stats counts it while it lives.  A run that never calls this pays
 * nothing for it.  Serialised with the other calls on the run. */
int32_t cm_run_open_memory(cm_run* r, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root);
/* GPU, batched: ok[i] in {0, 1}; returns 0 when it ran. */
int32_t cm_verify_memory_openings(uint32_t root, const cm_mem_opening* openings, uint64_t n, uint8_t* ok, cm_stream_t s);
/* Host code, no GPU: 0 accepted, 11 rejected.  cm_last_error() then reads "memory opening of address <a>: " and what is wrong:
 * the field that makes the record malformed with its depth (a value word: depth 30; "the sibling at depth <d>"), or, for a
 * well-formed record, "the path hashes to root <x>, not <y>". */
int32_t cm_verify_memory_opening(uint32_t root, const cm_mem_opening* opening);
/* ---- range openings (additive to revision 10: new symbols and two structs, nothing moved) ---------------------------------------
 * A contiguous run of cells under one root: a checkpoint image, an array-shaped result.  Neighbouring cells share almost every
 * node above them, so the statement needs the values (16 bytes per cell), at most two siblings per depth and about 4 hashes per
 * cell, where cell-by-cell openings cost 136 bytes and 31 hashes each.  The range [start, start + n_cells), with
 * last = start + n_cells - 1, covers the nodes [start >> k, last >> k] of depth 28 - k, k = 0 .. 27; hashing that interval up one
 * depth needs the node left of it exactly when start >> k is odd and the node right of it exactly when last >> k is even.
 * The values travel beside the record: 4 * n_cells words, an absent cell as (0, 0, 0, 0).  There is no `present` flag: a cell
 * held with zeros hashes like an absent one and a range has no use for the distinction.  A slot the range does not need is 0
 * and a record with a non-zero unused slot is malformed, so a range has exactly one valid record and the same call gives the
 * same bytes.  For n_cells = 1 exactly one of left[k] / right[k] is used at every k and equals siblings[k] of the cm_mem_opening
 * of that address.
 *
 * cm_input_open_memory_range / cm_run_open_memory_range build the record and the values on the GPU, on the calling thread's stream
 * and pool (threading as cm_run_open_memory): one lane per cell half bisects depth 30 of the node list, 56 more lanes bisect the
 * sibling slots — the lookup rule of the single openings, so the two can never disagree about a tree — and the words come back
 * in one host round trip (one more per further 2^19 cells).  cm_run_open_memory_range shares the cached image tree of
 * cm_run_open_memory: built on first use by either call, dropped when the image advances.  *root is written whenever the status
 * is 0.  Status 1, with nothing written to values or out: n_cells == 0, start + n_cells > 2^28, n_cells > 2^24, which > 1, a
 * NULL argument, a run whose image is empty.  Without a GPU the status is cm_init's (3).
 * cm_verify_memory_range uploads the values and the record and recomputes the root on the GPU (stream s; 0 = the calling
 * thread's own): one lane per cell gives the nodes of depth 28, one launch per depth halves the interval while it is wider than
 * 128 nodes, one workgroup finishes the remaining depths, checks the record's own words and compares with `root`; one word comes
 * back.  *ok = 1 when record and values are well formed and hash to `root`; a word >= P, a non-zero unused slot, n_cells == 0 or
 * start + n_cells > 2^28 give *ok = 0 and do not fail the call.  Status 1: a NULL argument or n_cells > 2^24 (read before
 * anything is allocated).  The call keeps nothing.
 * cm_verify_memory_range_host is the same check in host code, for a light client: it needs no GPU.
 * cm_mem_range_plan lists the hashing steps of the verification, host code only: steps[0] = the cells (depth 28, lo = start,
 * hi = last), steps[k + 1] = the step that hashes the interval of depth 28 - k into the nodes [lo, hi] of `depth` = 27 - k and
 * reads left[k] / right[k] where uses_left / uses_right are 1; `kernel` = 0 the per-cell kernel, 1 the per-level kernel, 2 the
 * single-workgroup tail (consecutive tail steps are one launch).  Always 29 steps; the device verifier launches from the same
 * records, so this is what runs.  Status 1: a bad range, a NULL argument, cap < 29. */
typedef struct {
  uint32_t start, n_cells;      /* n_cells >= 1, start + n_cells <= 2^28 */
  uint32_t left[28];            /* left[k]  = node (depth 28-k, index (start>>k) - 1) when (start>>k) is odd,  else 0 */
  uint32_t right[28];           /* right[k] = node (depth 28-k, index (last>>k) + 1)  when (last>>k) is even, else 0 */
} cm_mem_range_opening;         /* sizeof = 232 */
typedef struct {
  uint32_t depth, lo, hi;       /* the step produces the nodes lo .. hi of this depth */
  uint32_t kernel;              /* 0 k_fold_cells, 1 k_range_level, 2 k_range_tail */
  uint32_t uses_left, uses_right;
} cm_mem_range_step;            /* sizeof = 24 */
/* which: 0 = the input's initial tree, 1 = its final tree.  values: 4 * n_cells words.  *root receives that tree's root. */
int32_t cm_input_open_memory_range(const cm_device_input* in, uint32_t which, uint32_t start, uint32_t n_cells, uint32_t* values,
                                   cm_mem_range_opening* out, uint32_t* root);
/* Under the root of the run's image as it is now.  Serialised with the other calls on the run. */
int32_t cm_run_open_memory_range(cm_run* r, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out, uint32_t* root);
/* GPU: *ok in {0, 1}; returns 0 when it ran. */
int32_t cm_verify_memory_range(uint32_t root, const cm_mem_range_opening* opening, const uint32_t* values, uint8_t* ok, cm_stream_t s);
/* Host code, no GPU: 0 accepted, 11 rejected (1: a NULL argument or n_cells > 2^24).  cm_last_error() then reads
 * "memory range [<start>, <end>): " and what is wrong: "value word <i> of cell <a> is not below P", "the left sibling at depth
 * <d> is not below P" / "the right sibling ...", "unused left slot at depth <d> is not zero" / "unused right slot ...", a bad
 * start or n_cells, or, for a well-formed record, "the range hashes to root <x>, not <y>". */
int32_t cm_verify_memory_range_host(uint32_t root, const cm_mem_range_opening* opening, const uint32_t* values);
int32_t cm_mem_range_plan(uint32_t start, uint32_t n_cells, cm_mem_range_step* steps, uint32_t cap, uint32_t* n_steps);
/* ---- set openings (additive to revision 10: new symbols and one struct, nothing moved) -----------------------------------------
 * Any set of cells under one root: a few thousand unrelated cells for a bridge, a heap result behind pointers, the cells a segment
 * wrote, program + input + output + a few heap objects.  The third and general member of the family: a single cell and a
 * contiguous range are its special cases.  Paths that meet share every node above the meeting point, so the record holds each
 * sibling word once.
 *
 * The statement.  The addresses a[0] < a[1] < ... < a[n-1] < 2^28 are strictly ascending.  For k = 0 .. 27 let S_k be the
 * ascending list of distinct a[i] >> k: the nodes of depth 28 - k on some path.  A node x of S_k needs a sibling exactly when
 * x ^ 1 is not in S_k.  The record's sibling words come depth by depth, k = 0 first, inside a depth by ascending node index, and
 * each word is node(28 - k, x ^ 1).  count[k] is the number of words of depth 28 - k and n_siblings the sum of the counts: both
 * are functions of the addresses alone.  The values travel beside the record: 4 n words, an absent cell as (0, 0, 0, 0); there is
 * no `present` flag, as for ranges.
 * The fold walks S_k in order.  The cells first become nodes of depth 28 (H(H(v0, v1), H(v2, v3)), as for ranges).  An even x
 * whose successor in S_k is x + 1 hashes with it; any other x takes the next unread sibling word, on the right when x is even and
 * on the left when x is odd.  The parents form S_{k+1}; after k = 27 one node is left, the root.
 * A set has exactly one valid record: n_siblings must equal the sum of the counts, every word must be below P, the addresses must
 * be strictly ascending and below 2^28, and the same call gives the same bytes.  A record of m words travels as 20 n + 4 m bytes
 * (addresses, values, words) and folds with 3 n + sum_k |S_{k+1}| hashes.  For a contiguous set the words of depth 28 - k are
 * [left[k] if used] + [right[k] if used] of the cm_mem_range_opening of that range; for n = 1 they are siblings[0 .. 27] of the
 * cm_mem_opening.  When only cells of the set change between two trees the sibling words under both trees are identical, so
 * folding them with the new values (cm_memory_set_root_host) gives the root AFTER the write.
 *
 * cm_mem_set_plan lists the hashing steps of the verification, host code only, always 29: steps[0] = the cells (depth 28, n
 * nodes), steps[k + 1] = the step that hashes S_k into the n_nodes = |S_{k+1}| nodes of `depth` = 27 - k and reads
 * n_siblings = count[k] words; `kernel` = 0 the per-cell kernel, 1 the per-level kernel (while S_k is wider than 128 nodes), 2 the
 * single-workgroup tail (consecutive tail steps are one launch).  *n_siblings receives the sum of the counts: what a caller
 * allocates for.  The device verifier launches from these same records, so this is what runs.  Status 1: a NULL argument, n == 0
 * or n > 2^20, addresses not strictly ascending or not below 2^28, cap < 29.
 * cm_input_open_memory_set / cm_run_open_memory_set build the values and the words on the GPU, on the calling thread's stream and
 * pool (threading, stream, pool and image-tree cache as cm_run_open_memory_range): the addresses go up; a flag pass over the
 * 28 n pairs (depth, address lane), depth-major, applies the one rule the plan and the verifier also use; one exclusive scan turns
 * the flags into each word's position in the canonical order; a gather has every flagged lane bisect its depth's slice of the node
 * list — the lookup of the range and the single openings, a missing record being the default hash — while 2 n more lanes store
 * the value halves.  Every word is written by exactly one lane, without atomics; values, words and the device's count come back
 * in one host round trip (one more per further 8 MB) and the count is checked against the host plan's.  Temporaries: 448 bytes
 * per cell (the 28 flags and their scan, two words each).  *n_siblings receives the needed count whenever the addresses are good,
 * also when cap_siblings is too small.  Status 1, with nothing written to values or siblings: a NULL argument, n == 0 or
 * n > 2^20 ("split the set"), an address >= 2^28, a[i] <= a[i-1] (the message names the first such i), which > 1, an empty image,
 * cap_siblings too small (the message states the need).  Without a GPU the status is cm_init's (3).
 * cm_verify_memory_set uploads addresses, values and words and recomputes the root on the GPU (stream s; 0 = the calling thread's
 * own), with one hashing lane per PARENT, not per address: the opener's flag pass and one scan over all 28 depths give every
 * node's rank in S_k and every word's position (one scan for both: fewer launches than a scan per level), a scatter lists the head
 * lane of every node, one lane per cell gives the nodes of depth 28, one launch per depth hashes S_k into S_{k+1} while S_k is
 * wider than 128 nodes, and one workgroup finishes the remaining depths in LDS with a barrier between them, checks the count,
 * compares with `root` and writes the verdict and the computed root; three words come back.  Temporaries: 588 bytes per cell at
 * the most (flags and scan 448, head lanes up to 112, values 16, address 4, two node buffers 8) plus the words.  *ok = 1 when the
 * statement is well formed and folds to `root`; *computed_root (may be NULL) receives the root it folds to when well formed, else
 * 0.  Malformed input — n == 0, addresses not ascending or not below 2^28, a word not below P, a wrong n_siblings — gives
 * *ok = 0 and does not fail the call.  Status 1 only for a NULL argument or n > 2^20.  The call keeps nothing.
 * cm_memory_set_root_host and cm_verify_memory_set_host are the same fold in host code, for a light client: no GPU. */
typedef struct {
  uint32_t depth;               /* the step produces n_nodes nodes of this depth */
  uint32_t n_nodes;
  uint32_t n_siblings;          /* sibling words the step reads: count[27 - depth], 0 for the cells */
  uint32_t kernel;              /* 0 k_fold_cells, 1 k_fold_level, 2 k_fold_tail */
} cm_mem_set_step;              /* sizeof = 16 */
int32_t cm_mem_set_plan(const uint32_t* addresses, uint64_t n, cm_mem_set_step* steps, uint32_t cap, uint32_t* n_steps, uint32_t* n_siblings);
/* which: 0 = the input's initial tree, 1 = its final tree.  values: 4 * n words.  siblings: cap_siblings words.  *root receives
 * that tree's root. */
int32_t cm_input_open_memory_set(const cm_device_input* in, uint32_t which, const uint32_t* addresses, uint64_t n, uint32_t* values,
                                 uint32_t* siblings, uint32_t cap_siblings, uint32_t* n_siblings, uint32_t* root);
/* Under the root of the run's image as it is now.  Serialised with the other calls on the run. */
int32_t cm_run_open_memory_set(cm_run* r, const uint32_t* addresses, uint64_t n, uint32_t* values, uint32_t* siblings, uint32_t cap_siblings,
                               uint32_t* n_siblings, uint32_t* root);
/* GPU: *ok in {0, 1}; returns 0 when it ran. */
int32_t cm_verify_memory_set(uint32_t root, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings,
                             uint32_t n_siblings, uint8_t* ok, uint32_t* computed_root, cm_stream_t s);
/* Host code, no GPU: 0 = well formed, *root_out = the root it folds to; 11 = malformed (1: a NULL argument or n > 2^20).
 * cm_last_error() then reads "memory set of <n> cells: " and what is wrong: "address <i> is not above address <i-1>" (or, for
 * an address alone, "address <i> is beyond the address space of 2^28 cells"), "value word <j> of cell <a> is not below P",
 * "sibling <q> (depth <d>) is not below P", "<m> sibling words where the addresses need <m'>". */
int32_t cm_memory_set_root_host(const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings, uint32_t n_siblings,
                                uint32_t* root_out);
/* The same, compared with `root`: 0 accepted, 11 rejected; for a well-formed record "the set hashes to root <x>, not <y>". */
int32_t cm_verify_memory_set_host(uint32_t root, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings,
                                  uint32_t n_siblings);
/* ---- memory transitions (additive to revision 10: new symbols and structs, nothing moved) --------------------------------------
 * A proof states initial_root -> final_root.  A transition says which cells changed, and to what, in a form a holder of only the
 * two roots can check: the state diff a client following a run applies to its own copy of the memory.
 *
 * The statement.  A transition from root R0 to root R1 is: strictly ascending addresses a[0 .. n) < 2^28, old_values (4 n words),
 * new_values (4 n words) and ONE list of sibling words, exactly the record of a set opening of `a`: same order, same count[k],
 * same n_siblings.  It is valid when the set fold of (a, old_values, words) is R0 and the fold of (a, new_values, words) is R1,
 * and then says that the two memories agree in every cell outside `a` (the words ARE every subtree beside the set's paths).  An
 * absent cell is (0, 0, 0, 0) on either side, as for sets; there is no `present` flag.  A superset of the write set is allowed
 * (cells with old == new).  n == 0 is well formed only with n_siblings == 0 and is accepted exactly when R0 == R1, a read-only
 * segment; nothing is launched for it.  n <= 2^20, as for sets.  A transition travels as 36 n + 4 m bytes.
 *
 * cm_input_write_set lists, ascending, the cells whose four value words differ between the input's initial and final boundary
 * memory.  Built on the GPU, on the calling thread's stream and pool, by the classification and the scan of cm_link_diff with the
 * roles (initial, final) and a compaction to addresses: no atomic decides an order, the same call gives the same bytes.  A cell
 * present on one side only with an all-zero value does not change the root: it is counted in *n_zero_only and not listed
 * (cm_link_diff's rule).  *n_total = all there are; *n_total > cap means truncated and is not an error.  An input without
 * boundary memory (trees alone) has an empty write set.  Status 1: a NULL argument, NULL addresses with a capacity, rows not in
 * ascending address order.
 * cm_input_open_transition opens the transition of the input from its initial to its final tree over `addresses`; addresses ==
 * NULL means the write set (n is ignored), which then stays on the device between the diff and the opening.  The result is an
 * opaque handle because the sizes are not known before the call; cm_mem_transition_get fills a view (set struct_size =
 * sizeof(cm_mem_transition_view) first) whose pointers stay valid until cm_mem_transition_free.  On the GPU: the set opener's flag
 * pass and scan, then one gather launch of 28 n + 2 n + 2 n lanes — the sibling words and the old value halves from the INITIAL
 * tree exactly as cm_input_open_memory_set takes them, and 2 n more lanes that bisect depth 30 of the FINAL tree for the new
 * halves.  For a supplied set a membership launch over the diff's listed cells finds the lowest one the set misses: status 1,
 * "cell <a> changes in this segment and is not in the set".  One host round trip carries the data (one more per further 8 MB;
 * with addresses == NULL the write set's size comes back in a small one of its own); the device's word count is checked against
 * cm_mem_set_plan's.  n_zero_only is the write set's.  Refusals are otherwise those of cm_input_open_memory_set: a NULL `in` or
 * `out`, n == 0 with addresses given, n > 2^20, addresses not strictly ascending or not below 2^28.  With addresses == NULL a
 * segment that changes nothing gives n == 0 and no words, and one that changes more than 2^20 cells is refused.  Without a GPU
 * the status is cm_init's (3).
 * cm_verify_memory_transition checks both roots on the GPU in ONE fold over two value planes (stream s; 0 = the calling thread's
 * own).  The set verifier's flag pass, scan and head scatter run once; k_fold_cells, one lane per cell, range-checks all eight
 * words and writes two nodes of depth 28; k_fold_level, one lane per parent while S_k is wider than 128 nodes, does the index
 * arithmetic and loads the sibling word once and compresses twice; k_fold_tail, one workgroup, finishes the remaining depths of
 * both planes in LDS, checks the count, compares both roots and writes the verdict and the roots; four words come back.  The
 * launches come from cm_mem_set_plan's records.  *ok = 1 when the statement is well formed and both folds match; computed (may be
 * NULL) receives the two roots it folds to when well formed (n == 0: root_before twice), else zeros.  Malformed input is a verdict
 * (*ok = 0), never a failed call; status 1 only for a NULL argument or n > 2^20.  The call keeps nothing.  Temporaries: the set
 * verifier's plus 24 bytes per cell.
 * cm_verify_memory_transition_host is the same check in host code, two runs of the set fold: 0 accepted, 11 rejected, 1 for a
 * NULL argument or n > 2^20.  cm_last_error() then reads "memory transition of <n> cells: " and the set verifier's own words for a
 * malformed record, with "old value word <j> of cell <a>" / "new value word ..." where a value is bad; for a well-formed record
 * "the old values hash to root <x>, not <y>", or, when that side passes, "the new values hash to root <x>, not <y>"; for n == 0
 * "no cell changes, and root <x> is not root <y>".
 * cm_prove_run_transitions is cm_prove_run with each segment's write-set transition opened on the adapting thread right after the
 * segment is adapted and before a worker proves it: the proofs are cm_prove_run's, byte for byte.  Error contract: cm_prove_run's;
 * transitions[i] is NULL for every segment that was not adapted, and the caller frees the others. */
typedef struct cm_mem_transition cm_mem_transition;
typedef struct {
  uint32_t struct_size;
  uint32_t root_before;
  uint32_t root_after;
  uint32_t n;
  uint32_t n_siblings;
  uint32_t n_zero_only;
  const uint32_t* addresses;    /* n */
  const uint32_t* old_values;   /* 4 n */
  const uint32_t* new_values;   /* 4 n */
  const uint32_t* siblings;     /* n_siblings */
} cm_mem_transition_view;       /* sizeof = 56 */
int32_t cm_input_write_set(const cm_device_input* in, uint32_t* addresses, uint64_t cap, uint64_t* n_total, uint64_t* n_zero_only);
int32_t cm_input_open_transition(const cm_device_input* in, const uint32_t* addresses, uint64_t n, cm_mem_transition** out);
int32_t cm_mem_transition_get(const cm_mem_transition* t, cm_mem_transition_view* out);
int32_t cm_mem_transition_free(cm_mem_transition* t);
int32_t cm_verify_memory_transition(uint32_t root_before, uint32_t root_after, const uint32_t* addresses, uint64_t n, const uint32_t* old_values,
                                    const uint32_t* new_values, const uint32_t* siblings, uint32_t n_siblings, uint8_t* ok, uint32_t computed[2],
                                    cm_stream_t s);
int32_t cm_verify_memory_transition_host(uint32_t root_before, uint32_t root_after, const uint32_t* addresses, uint64_t n, const uint32_t* old_values,
                                         const uint32_t* new_values, const uint32_t* siblings, uint32_t n_siblings);
int32_t cm_prove_run_transitions(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                                 cm_proof** outs, cm_mem_transition** transitions);
/* Composed transitions (additive to revision 10: one new function, no new struct).  cm_compose_transitions makes a chain of
 * transitions R0 -> R1 -> ... -> Rk into the ONE transition R0 -> Rk over the union U of their cells, from the records alone: no
 * memory image, no tree and no hash is needed, so a relay that holds only the records can do it.  parts[i] is a filled
 * cm_mem_transition_view (from cm_mem_transition_get, or built over bytes that arrived over a wire; struct_size set).  The result
 * is an ordinary transition: read it with cm_mem_transition_get, free it with cm_mem_transition_free, check it with
 * cm_verify_memory_transition or cm_verify_memory_transition_host; its wire format is the existing one.
 * The statement.  addresses = the strictly ascending union U of all parts' addresses; old_values[u] = the old value of u in the
 * first part that holds u; new_values[u] = the new value of u in the last part that holds u (a cell some part writes and a later
 * part writes back stays in U with old == new: a superset of the write set is valid, and dropping the cell would need hashes no
 * record holds); siblings = the canonical record of U (cm_mem_set_plan's order and counts); root_before = parts[0].root_before,
 * root_after = parts[n_parts - 1].root_after; n_zero_only = the sum of the parts'.  Parts with n == 0 take part in the chain and
 * add nothing; when every part is empty the result has n == 0 and no words; one part composes to itself, byte for byte.
 * Why the records suffice.  S_k(U) = the distinct u >> k.  The record of U needs node(28 - k, x ^ 1) exactly when x is in S_k(U)
 * and x ^ 1 is not.  Then no cell of U lies under x ^ 1, and since every part is valid the memories of the chain agree outside each
 * part's set: that subtree has the same hash under every root of the chain.  The first part r that holds the lowest address of U
 * under x has x in S_k(a_r) and not x ^ 1 (S_k(a_r) is a subset of S_k(U)), so its record holds that very word, and the word is
 * copied from there.  A word that a part holds for a subtree containing a cell of U may be stale; such a word is never needed.
 * The guarantee.  The call hashes nothing.  IF every part is a valid transition and the roots chain, the result is a valid
 * transition from parts[0].root_before to parts[n_parts - 1].root_after.  A caller that does not trust its source verifies the
 * result, or the parts.  The same call gives the same bytes, and device 0 and device 1 give the same bytes.
 * device == 0 composes in host code and needs no GPU: a stable merge of the sorted lists, then cm_mem_set_plan's walk over every
 * part and over U.  device == 1 composes on the GPU on the calling thread's stream and pool, which the call waits for: one upload
 * of the concatenated parts; a stable 28-bit radix sort of the N addresses (equal addresses stay in chain order); k_compose_heads
 * (head flags and the seam check), one scan for the ranks, one small round trip for |U|; k_compose_cells (U, the values, the source
 * part of every cell); the set opener's flag pass and scan over U, ONE segmented flag pass and ONE scan over the 28 N pairs of all
 * parts; k_compose_gather, one lane per pair of U, every word written by exactly one lane without atomics; one download (one more
 * trip per further 8 MB); the device's word count is checked against cm_mem_set_plan(U).  The number of launches and round trips
 * does not depend on n_parts.  Temporaries: flags and scans, 448 bytes per cell of N plus of |U|, dominate; with the sort's
 * buffers, the uploaded parts and the result the cap of 2^20 cells bounds a call near 1 GB (derived, not measured).  Every
 * device buffer is back in the pool when the call returns.
 * Refusals, the same status and message on both paths; *out is NULL on every failure.  device == 1 without a GPU: cm_init's
 * status (3), returned before any argument is looked at.  Status 1, cm_last_error() naming the cause: device > 1; a NULL `parts`
 * or `out`; n_parts == 0 or n_parts > 2^16; a part with a short struct_size; a part with a NULL array where n > 0 or n_siblings
 * > 0; the parts' n summing to more than 2^20 ("compose in groups": the operation is associative, so a caller can always split)
 * — all before any address is read.  Status 11 (rejected), parts in ascending order: "part <i>: " and the set verifier's own
 * words for addresses that are not strictly ascending or not below 2^28; "part <i>: <m> sibling words where the addresses need
 * <m'>" (established before any word of the part is read); "part <i> starts at root <x>, part <i-1> ended at root <y>"; then the
 * seam check: where a cell occurs in part j and next in part i > j, old_i must equal new_j, else "cell <a>: part <i> reads a value
 * part <j> did not leave" for the lowest such address and, for it, the lowest i. */
int32_t cm_compose_transitions(const cm_mem_transition_view* parts, uint32_t n_parts, uint32_t device, cm_mem_transition** out);
/* Batched verification of transitions and sets (additive to revision 10: three new functions and two structs, nothing moved).
 * cm_verify_memory_transitions / cm_verify_memory_sets check n_parts records in ONE fold: ok[i] and computed[2 i], computed[2 i + 1]
 * (sets: computed[i]) are exactly what cm_verify_memory_transition / cm_verify_memory_set gives for part i alone.  parts[i] is a
 * filled view (struct_size set); a set view is a transition view without the second plane.  Malformed input is a verdict —
 * ok[i] = 0 with zeros in `computed` — never a failed call, and a bad part does not disturb its neighbours' verdicts or roots (the
 * rule cm_program_ids states).  A transition part with n == 0 is accepted exactly when it has no words and its two roots are equal
 * (computed: root_before twice); it puts nothing into any launch, and a batch of only such parts launches nothing.  A set part with
 * n == 0 is rejected, as by the single call.
 * Host side: every part goes through the checks the single call makes before its first launch (addresses strictly ascending and
 * below 2^28, n_siblings = cm_mem_set_plan's); a part that fails them gets ok = 0 and is left out of the device batch, so only
 * well-shaped parts reach a kernel.  Device side (stream s; 0 = the calling thread's own): the parts' addresses, values and words go
 * up concatenated with their prefix tables in one copy; the segmented flag pass of cm_compose_transitions and ONE scan over the
 * 28 N pairs of all parts; a head scatter with ranks relative to each part's slice; one lane per cell of the concatenation; one
 * launch per depth with one lane per parent of ALL parts (a lane bisects that depth's prefix table for its part and works inside
 * the part's slice) while any part is wider than 128 nodes — a part that is already narrow rides along; then one tail launch with
 * one workgroup per part: the level in LDS, the remaining depths, the count, the root or roots compared, four words per part
 * written.  One upload, one download of 16 bytes per part, one wait.  The number of launches and round trips does not depend on
 * n_parts: it is that of the part with the most per-level steps plus a constant (cm_mem_batch_plan lists them).  Temporaries per
 * cell of the batch: the single call's (flags and scan 448 bytes, head lanes up to 112, values 16 per plane, address 4, two node
 * buffers 4 per plane each) plus 116 + 4 * planes + 16 bytes of tables per part.  The call keeps nothing: every device buffer is
 * back in the pool when it returns.
 * Status 1, cm_last_error() naming the part, all decided before any address is read: a NULL `parts` or `ok`; n_parts == 0 or
 * n_parts > 2^16; a part with a short struct_size; a NULL array in a part whose count is non-zero; a part with n > 2^20; the
 * parts' n summing to more than 2^20 ("verify in groups").  Without a GPU a call that passes these returns cm_init's status (3).
 * cm_mem_batch_plan lists, host code only and from the addresses alone, the launches the batch would make: none when no part
 * reaches the device (a part without cells or with bad addresses does not), else always 29 steps — steps[0] the cells (depth 28),
 * steps[k + 1] the step that hashes every part's S_k into S_{k+1}; n_nodes = the parents of all parts together, widest_part = the
 * most any one part has, `kernel` = 0 the per-cell kernel, 1 the per-level kernel (while any part's S_k is wider than 128 nodes), 2
 * the tail (consecutive tail steps are one launch).  The launch path runs the same host code.  Status 1: a NULL argument,
 * n_parts == 0 or > 2^16, a NULL address list with a count, a part or a sum over 2^20 cells, cap < *n_steps (which is still
 * written). */
typedef struct {
  uint32_t struct_size;
  uint32_t root;
  uint32_t n;
  uint32_t n_siblings;
  const uint32_t* addresses;    /* n */
  const uint32_t* values;       /* 4 n */
  const uint32_t* siblings;     /* n_siblings */
} cm_mem_set_view;              /* sizeof = 40 */
typedef struct {
  uint32_t depth;               /* the step produces nodes of this depth */
  uint32_t n_nodes;             /* in all parts together */
  uint32_t widest_part;         /* the most nodes any one part has at that depth */
  uint32_t kernel;              /* 0 cells, 1 level, 2 tail */
} cm_mem_batch_step;            /* sizeof = 16 */
int32_t cm_verify_memory_transitions(const cm_mem_transition_view* parts, uint32_t n_parts, uint8_t* ok, uint32_t* computed, cm_stream_t s);
int32_t cm_verify_memory_sets(const cm_mem_set_view* parts, uint32_t n_parts, uint8_t* ok, uint32_t* computed, cm_stream_t s);
int32_t cm_mem_batch_plan(const uint32_t* const* addresses, const uint32_t* n, uint32_t n_parts, cm_mem_batch_step* steps, uint32_t cap,
                          uint32_t* n_steps);
/* ---- followed memory (additive to revision 10: new symbols and one struct, nothing moved) --------------------------------------
 * The party between the prover and the light client: a follower (a bridge, an RPC node, a checkpoint service) that keeps its own
 * copy of a run's memory and answers openings under the run's latest root.  cm_mem_image is that copy: a memory image with its
 * partial Merkle tree, resident on the GPU (device == 1) or in host memory (device == 0, host code only, no GPU needed),
 * independent of any prover handle.  It absorbs a segment's writes by re-hashing only the dirty paths, checks itself against the
 * proof's roots, serves the three kinds of opening under its current root and re-emits a full transition from a bare update.
 *
 * The handle holds one list of cm_merkle_node records in the order every opener reads: depth 30 .. 1, ascending index inside a
 * depth.  Only the first five words of a record are contract (index, depth, left_value, right_value, parent_value); the three
 * multiplicity words enter no hash and are unspecified.  The cells are the list's depth-30 slice: a held cell a owns the
 * records 4a and 4a + 2 there and the record 2a of depth 29, whatever its value, so a cell written to (0, 0, 0, 0) stays held
 * with zeros, which hashes like an absent one.  Both modes give the same roots and the same node words 0 .. 4.
 *
 * cm_mem_image_create makes the image of n cells: addresses strictly ascending and below 2^28, value words below P, n at most
 * 2^22 (the device tree builder's transient block is 3840 bytes per cell: 15 GiB at the limit; a device image may grow beyond
 * it by updates).  n == 0 gives the empty image, whose root is default[0].  device == 1 builds the tree with the device tree
 * builder (the leaves of every cell, then one launch group per depth), on the calling thread's stream and pool; device == 0
 * folds the cells into the empty image in host code.  Status 1 for a bad argument, naming the first bad address or value word;
 * device == 1 without a GPU is cm_init's status (3), returned before any argument is looked at.
 * cm_mem_image_root, cm_mem_image_stats_get (set struct_size first) and cm_mem_image_free read and free the handle.
 * cm_mem_image_read gathers the values of n addresses in any order, repeats allowed, an absent cell as zeros (at most 2^24 a
 * call).  cm_mem_image_cells lists the whole image in ascending address order and cm_mem_image_nodes the node list: *n_total =
 * all there are; *n_total > cap means truncated and is not an error (cm_input_write_set's contract).
 *
 * cm_mem_image_apply writes new_values to `addresses` (strictly ascending, below 2^28, 0 < n <= 2^20, as for a set opening).
 * The checks run in this order, and the image is unchanged — root, nodes and cells byte for byte — unless all of them pass:
 *   1. bad arguments: status 1 (a NULL img, addresses, new_values or root_out; n == 0; n > 2^20; addresses not ascending);
 *   2. a new value word not below P: status 11, "memory image: new value word <j> of cell <a> is not below P";
 *   3. root_before given and not the image's root: 11, "the image is at root <x>, the update starts from <y>";
 *   4. old_values given and not the image's current values (an absent cell reads as zeros): 11, "cell <a> holds (..), the
 *      update's old value is (..)" for the lowest such address;
 *   5. the new root is computed;
 *   6. root_after given and different: 11, "the image would hash to root <x>, not <y>".
 * Then the new node list is committed: new addresses are inserted, held ones replaced.  *root_out receives the new root.
 * record_out (may be NULL) receives an ordinary cm_mem_transition over the addresses: its old values and sibling words are read
 * from the tree before the update, its new values are the given ones, its roots the ones seen; the transition verifiers accept
 * it unchanged, so a follower that received 20 n bytes can serve the 36 n + 4 m byte record to light clients.
 * The rule.  The update is the set fold with each sibling word taken from the image's own tree.  With S_k the distinct
 * a[i] >> k, the dirty nodes of depth 28 - k are exactly S_k and the dirty pair records of that depth one per node of S_{k+1}:
 * 3 n + sum_k |S_{k+1}| hashes, the set fold's count, whatever the size of the image.
 * On the GPU (the calling thread's stream and pool): k_img_check, one lane per cell half, bisects the depth-30 slice for the
 * current value and reports the lowest differing cell by an atomic minimum; k_img_cells, one lane per cell, writes the two
 * depth-30 records and the depth-29 record from the new value alone; the set verifier's flag pass, scan and head scatter; then
 * the steps of cm_mem_set_plan for the same addresses — k_fold_level, one lane per parent while S_k is wider than 128 nodes, and
 * k_fold_tail, one workgroup, for the rest — where a child in S_k takes its new hash from the level below and any other child
 * the old tree's word (the openers' lookup; a missing record is the depth's default hash).  The commit: k_img_rank bisects
 * every dirty record's place in the old slice of its depth, one exclusive scan counts the inserts, k_img_merge moves old and
 * dirty records into a new buffer in one launch and k_img_offsets updates the depth offsets.  Everything is enqueued before
 * the call's one host round trip (one more for a record); the handle swaps buffers only behind check 6.  The number of
 * launches does not depend on the size of the image.
 * cm_mem_image_apply_transition is cm_mem_image_apply with t's addresses, both value planes and both roots; t->siblings is
 * never read and may be NULL with n_siblings 0 (the "bare" transition: 20 n bytes and two roots).  t->n == 0 changes nothing
 * and still checks the roots: "no cell changes, and root <x> is not root <y>".
 * cm_mem_image_open_memory, _range and _set follow the contract of their cm_run_open_* twins (argument checks, an empty image
 * is refused, *root is written) and are thin calls into the same openers over the image's node list.  Device images only: a
 * host image refuses them with status 1 and says so.
 * Threading: calls on one image are serialised by a mutex in the handle, as for cm_run; every call waits for its GPU work, so
 * any thread may make the next one.  cm_mem_stats counts a device image while it lives. */
typedef struct cm_mem_image cm_mem_image;
typedef struct {
  uint32_t struct_size;
  uint32_t device;              /* 1: on the GPU, 0: in host memory */
  uint64_t n_cells;
  uint64_t n_nodes;
  uint64_t bytes;               /* held by the handle: pool blocks (device) or the node vector's capacity (host) */
} cm_mem_image_stats;           /* sizeof = 32 */
int32_t cm_mem_image_create(const uint32_t* addresses, const uint32_t* values, uint64_t n, uint32_t device, cm_mem_image** out);
int32_t cm_mem_image_free(cm_mem_image* img);
int32_t cm_mem_image_root(cm_mem_image* img, uint32_t* root);
int32_t cm_mem_image_stats_get(cm_mem_image* img, cm_mem_image_stats* out);
int32_t cm_mem_image_read(cm_mem_image* img, const uint32_t* addresses, uint64_t n, uint32_t* values);
int32_t cm_mem_image_cells(cm_mem_image* img, uint32_t* addresses, uint32_t* values, uint64_t cap, uint64_t* n_total);
int32_t cm_mem_image_nodes(cm_mem_image* img, cm_merkle_node* nodes, uint64_t cap, uint64_t* n_total);
int32_t cm_mem_image_apply(cm_mem_image* img, const uint32_t* addresses, const uint32_t* new_values, uint64_t n, const uint32_t* old_values,
                           const uint32_t* root_before, const uint32_t* root_after, uint32_t* root_out, cm_mem_transition** record_out);
int32_t cm_mem_image_apply_transition(cm_mem_image* img, const cm_mem_transition_view* t, cm_mem_transition** record_out);
int32_t cm_mem_image_open_memory(cm_mem_image* img, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root);
int32_t cm_mem_image_open_memory_range(cm_mem_image* img, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out,
                                       uint32_t* root);
int32_t cm_mem_image_open_memory_set(cm_mem_image* img, const uint32_t* addresses, uint64_t n, uint32_t* values, uint32_t* siblings,
                                     uint32_t cap_siblings, uint32_t* n_siblings, uint32_t* root);
/* ---- batched image updates (additive to revision 10: one new function and two structs, nothing moved) ------------------------
 * cm_mem_images_apply updates n_parts DIFFERENT device images in one call, one update each, through ONE ladder of launches: a
 * small update is bound by its chain of dependent launches, not by hashing, and independent images share that chain as the
 * records of cm_verify_memory_transitions do.  It is what a follower of many runs (a bridge, an RPC node, a checkpoint service)
 * calls once per round of segments.
 * Per part: parts[i] gets exactly the status, message, root and resulting image that
 * cm_mem_image_apply(img, addresses, new_values, n, old_values, root_before, root_after, &root, NULL) would give alone — nodes
 * and cells byte for byte.  results[i].status = 0 (applied), 1 (a bad part) or 11 (refused), .message the single call's words
 * ("" when applied), .root the image's root when the call returns.  A refused or bad part leaves its image byte-identical and
 * does not disturb its neighbours, which are applied (the rule cm_program_ids and the batch verifiers state).  The checks run in
 * the single call's order: 1 bad arguments; 2 a new value word not below P; 3 root_before; 4 old_values, naming the lowest
 * address; 5 - 6 root_after.  A part's own status 1, never a failed call: a host image ("device images only": it takes its
 * updates through cm_mem_image_apply), n == 0, n > 2^20, a NULL addresses or new_values, addresses not strictly ascending or not
 * below 2^28 (the single call's message).  Such a part, and one refused by check 2 or 3 — which read only what the host holds —
 * never reaches a kernel; the others run.
 * Returns 0 when every part has status 0, else the status of the lowest part that has another, with cm_last_error() =
 * "part <i>: <message>".
 * The call as a whole is refused with status 1, before any address is read and before the device is asked for: a NULL `parts` or
 * `results`; n_parts == 0 or n_parts > 2^16; a part with a short struct_size; a part with a NULL img; the parts' n summing to more
 * than 2^20 ("apply in groups"); one image named by two parts — updates of one image depend on each other and do not belong in
 * one fold; the message names both parts.  Nothing is written to `results` then.  A call that passes these asks for the device
 * whatever its parts hold: without a GPU it returns cm_init's status (3), with the host's own verdicts (status 1) in `results`
 * and cm_init's status and message in every other part.
 * The batch makes no record (cm_mem_image_apply's record_out): a follower that must re-emit the full transition of an update
 * uses the single call.
 * Device side (the calling thread's stream and pool, as the single call): one upload of one block — per part its result words
 * and a table entry (the image's node list and depth offsets, where its new list goes, its slice of the dirty records), the
 * prefix tables, then the addresses, new values and old values concatenated; k_imgs_check and k_imgs_cells on the concatenation
 * (a lane bisects the cells' prefix for its part and reads THAT part's image); the flag pass, ONE scan and the head scatter of
 * the batched verifier; k_imgs_level, one launch per depth with one lane per parent of ALL parts while any part is wider than 128
 * nodes — a narrow part rides along; k_imgs_tail, one workgroup per part, which writes the part's root; k_imgs_rank over the dirty
 * records of all parts, ONE exclusive scan of the insert flags with one sentinel per part, k_imgs_merge with one lane per old and
 * per dirty record of all parts into per-part new lists taken from the pool before the first launch, k_imgs_offsets with one
 * block per part; one download of 144 bytes per part, one wait (one more trip of 16 bytes per part whose old values differ, for
 * the value its message names).  The host then decides part by part: refuse and drop the new list, or swap.  The number of
 * launches and round trips does not depend on n_parts: it is that of the part with the most per-level steps, as
 * cm_mem_batch_plan lists for the parts' addresses, plus a constant.
 * Threading: the handles' mutexes are taken in one global order, by handle address, and are all held until the last swap. */
typedef struct {
  uint32_t struct_size;          /* sizeof(cm_mem_image_update) */
  uint32_t n;                    /* cells */
  cm_mem_image* img;
  const uint32_t* addresses;     /* n, strictly ascending, below 2^28 */
  const uint32_t* new_values;    /* 4 n */
  const uint32_t* old_values;    /* 4 n, or NULL: not compared */
  const uint32_t* root_before;   /* NULL: not compared */
  const uint32_t* root_after;    /* NULL: not compared */
} cm_mem_image_update;           /* sizeof = 56 */
typedef struct {
  int32_t status;                /* 0 applied, 1 bad part, 11 refused */
  uint32_t root;                 /* the image's root when the call returns */
  char message[248];             /* "" when applied */
} cm_mem_image_result;           /* sizeof = 256 */
int32_t cm_mem_images_apply(const cm_mem_image_update* parts, uint32_t n_parts, cm_mem_image_result* results);
/* ---- batched set openings (additive to revision 10: one new function and two structs, nothing moved) --------------------------
 * cm_mem_images_open_memory_sets opens n_parts sets in one call, each under the device image its part names, through ONE chain of
 * launches and one round trip: a small set opening is bound by its launches and its two copies, not by hashing or gathering, and
 * independent openings share that chain as the parts of cm_mem_images_apply do.  It is what a follower that serves clients (a
 * bridge, an RPC node, a checkpoint service) calls once per round of pending requests, and what produces in one call the records
 * cm_verify_memory_sets checks in one call.
 * Per part: parts[i] gets exactly what
 * cm_mem_image_open_memory_set(img, addresses, n, values, siblings, cap_siblings, &n_siblings, &root) would give alone —
 * results[i].status = 0 (opened) or 1 (a bad part), .message the single call's words ("" when opened), .n_siblings, .root, and
 * values[0 .. 4n) and siblings[0 .. n_siblings) byte for byte.  A bad part does not disturb its neighbours, which are opened, and
 * its `values` and `siblings` are not written.  A part's own status 1, never a failed call, in the single call's order: a NULL
 * addresses, values or siblings; n == 0; n > 2^20; addresses not strictly ascending or not below 2^28 (the single call's message);
 * a cap_siblings below the need (.n_siblings is cm_mem_set_plan's all the same); a host image; an empty image.  Such a part never
 * reaches a kernel; the others run.
 * Returns 0 when every part has status 0, else the status of the lowest part that has another, with cm_last_error() =
 * "part <i>: <message>".
 * The call as a whole is refused with status 1, before any address is read and before the device is asked for: a NULL `parts` or
 * `results`; n_parts == 0 or n_parts > 2^16; a part with a short struct_size; a part with a NULL img; the parts' n summing to more
 * than 2^20 ("open in groups").  Nothing is written to `results` then.  A call that passes these asks for the device whatever its
 * parts hold: without a GPU it returns cm_init's status (3), with the host's own verdicts (status 1) in `results` and cm_init's
 * status and message in every other part.
 * The one difference from cm_mem_images_apply: openings only read, so several parts MAY name one image — many clients under one
 * root is the common case.  Every part of one call that names an image is opened under the same root of it.
 * Nothing reaches any caller's array before EVERY part's device word count has been compared with the host plan (the single
 * call's rule, for the whole batch); a count that differs fails the call.
 * Device side (the calling thread's stream and pool, as the single call): one upload of one block — per part a table entry (the
 * image's node list, the depth offsets its handle already keeps, where its values and its words go in the output block), the
 * prefixes of the cells and of the words, the default hashes, then the addresses concatenated; the flag pass over the 28 N pairs of all parts and
 * ONE scan, as the batched verifier's; k_sets_gather, one launch over 28 N + 2 N lanes — a lane bisects the cells' prefix for its
 * part and reads THAT part's image; a sibling word lands in its part's slice at the scan's low word minus the scan at the part's
 * first pair, the last pair lane of a part stores the part's count, a lane behind the pairs stores one half of a cell's value;
 * every word is written by exactly one lane, no atomic; one download of one block (the counts, the values, the words) through
 * the pinned landing buffer, one trip per 8 MB, scattered to the callers' arrays.  The number of launches and round trips does
 * not depend on n_parts.
 * Threading: each DISTINCT handle's mutex is taken once, in one global order, by handle address (the order cm_mem_images_apply
 * takes them in), and all are held until the download has landed. */
typedef struct {
  uint32_t struct_size;        /* sizeof(cm_mem_set_request) */
  uint32_t n;                  /* cells */
  cm_mem_image* img;           /* a device image; several parts MAY name the same image */
  const uint32_t* addresses;   /* n, strictly ascending, below 2^28 */
  uint32_t* values;            /* out, 4 n */
  uint32_t* siblings;          /* out, room for cap_siblings words */
  uint32_t cap_siblings;
  uint32_t reserved;           /* 0 */
} cm_mem_set_request;          /* sizeof = 48 */
typedef struct {
  int32_t status;              /* 0 opened, 1 bad part */
  uint32_t root;               /* the image's root (written whenever img is usable) */
  uint32_t n_siblings;         /* the words the set needs = cm_mem_set_plan's, also when cap_siblings is short */
  uint32_t reserved;
  char message[240];           /* "" when opened */
} cm_mem_set_result;           /* sizeof = 256 */
int32_t cm_mem_images_open_memory_sets(const cm_mem_set_request* parts, uint32_t n_parts, cm_mem_set_result* results);
/* ---- program identity and the statement of a run (additive to revision 10) ---------------------------------------------------
 * Which program a proof is about, as one 31-bit word: Proof::program_id() of the reference (crates/prover/src/lib.rs:75-97), the
 * Poseidon2 root of the partial memory tree that holds only the proof's public program cells.  An "entry" is the seven-word record
 * of cm_proof_public_entries: present, address, value[4], clock.
 *
 * The statement.  The entries are present and their addresses are first, first + 1, .., first + n - 1 (first = entry 0's address).
 * Every cell becomes its node of depth 28, H(H(v0, v1), H(v2, v3)), as for ranges; the interval [first >> k, last >> k] of depth
 * 28 - k is hashed into the interval of depth 27 - k, a child outside the interval being the default hash of depth 28 - k (the
 * range fold of cm_mem_range_opening with every left[k] / right[k] the default); once the interval is one node the same step chains
 * it to depth 0.  About 4 n + 28 hashes.  Clocks do not enter.  A present cell whose value is (0, 0, 0, 0) hashes to the default
 * of depth 28, so it leaves no trace in the id: a property of the tree, as for the link diff's `zero only` cells.
 * cm_program_id_entries is host code, no device call.  Status 1, nothing written, cm_last_error() naming the entry and address:
 * NULL pointers; n == 0 (the reference returns None and unwraps it); more than 2^24 entries; an entry with present == 0 (the
 * reference's res.unwrap() panics there); "entry <i> has address <a>, not <first + i>"; "value word <j> of entry <i> (address <a>)
 * is not below P"; a range that ends beyond the address space of 2^28 cells.
 * cm_proof_program_id: the same computation over the proof's program entries.
 * cm_program_ids / cm_proofs_program_ids compute the ids of n programs on the GPU in one batch (stream s; 0 = the calling thread's
 * own): the host walks each item once, checking present flags and addresses and gathering the value words; one upload of all
 * values behind a table of offsets; two launches whatever n is — one lane per cell of the whole batch range-checks the four words
 * and writes the node of depth 28, then one workgroup of 1024 lanes per item folds its interval, through two global buffers while
 * it is wider than 1024 nodes and in LDS from there on; one download of ids and flags.  Every word is written by exactly one lane,
 * without atomics: the same call gives the same bytes.  status[i] is 0 or 1 by the rules of cm_program_id_entries, ids[i] the id
 * or 0; a bad item does not disturb its neighbours' ids.  Returns 0 when every status is 0, else 1 with cm_last_error() reading
 * "item <i>: ..." for the lowest bad i.  n == 0 (or more than 2^20 items, or more than 2^26 cells in all) or a NULL array:
 * status 1; a NULL entries[i] or proofs[i] is a bad item.  Without a GPU the status is cm_init's (3), returned before any argument
 * is looked at.  The call keeps nothing: its device buffers come from the calling thread's pool and are back there when it returns. */
int32_t cm_program_id_entries(const uint32_t* entries, uint64_t n, uint32_t* id);
int32_t cm_proof_program_id(const cm_proof* p, uint32_t* id);
int32_t cm_program_ids(const uint32_t* const* entries, const uint64_t* n_entries, uint32_t n, uint32_t* ids, int32_t* status, cm_stream_t s);
int32_t cm_proofs_program_ids(const cm_proof* const* proofs, uint32_t n, uint32_t* ids, int32_t* status, cm_stream_t s);
/* What a chain of proofs states: which program, from which registers and memory root to which.  Set struct_size =
 * sizeof(cm_run_statement) before the call (a NULL or short `out`, or device > 1: status 1).  In this order:
 * 1. cm_verify_run (device == 0) or cm_verify_run_device (device == 1); its status and message pass through unchanged.
 * 2. For every segment i > 0 the program entries equal segment 0's in present, address and value (clocks are not compared); else
 *    status 11 with "run: segment <i> program differs from segment 0 at address <a>" or "run: segment <i> has <k> program entries,
 *    segment 0 has <m>".
 * 3. The id is hashed once: through the batch path on the GPU when device == 1, in host code otherwise (a program that has no id
 *    is status 1 with cm_program_id_entries' words behind "run: program id: ").
 * 4. expected_program_id, when not NULL, must equal it: else status 11 with "run: program_id 0x%08x != expected 0x%08x".
 * On success the registers, initial_root and n_input are proof 0's, the final registers, final_root and n_output those of proof
 * n - 1; the entries themselves stay reachable through cm_proof_public_entries. */
typedef struct {
  uint32_t struct_size;
  uint32_t n_segments;
  uint32_t program_id;
  uint32_t program_start;
  uint32_t n_program;
  uint32_t initial_pc;
  uint32_t initial_fp;
  uint32_t final_pc;
  uint32_t final_fp;
  uint32_t initial_root;
  uint32_t final_root;
  uint32_t n_input;
  uint32_t n_output;
  uint32_t reserved0;
} cm_run_statement;             /* sizeof = 56 */
int32_t cm_run_statement_of(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, const uint32_t* expected_program_id,
                            uint32_t device, cm_run_statement* out);
/* AccumulationOps::accumulate: dst[k][i] += src[k][i] (4 coordinate columns of n words); generate_secure_powers:
 * out[i] = felt^i for i < n (host array of 4 * n words).  Column::zeros = cm_col_alloc + cm_col_zero. */
int32_t cm_accumulate(const cm_handle dst[4], const cm_handle src[4], uint64_t n, cm_stream_t s);
int32_t cm_generate_secure_powers(const uint32_t felt[4], uint64_t n, uint32_t* out);
int32_t cm_col_zero(cm_handle h, uint64_t n_u32, cm_stream_t s);
/* FriOps::decompose: lambda = (sum of the first half - sum of the second half) / 2^log_n of a bit-reversed secure
 * evaluation; g = f - lambda on the first half, f + lambda on the second.  In place; lambda_out = 4 words. */
int32_t cm_fri_decompose(const cm_handle f[4], uint32_t log_n, uint32_t lambda_out[4], cm_stream_t s);
/* Optional HIP-event kernel timing on the launch stream (bench.py `roofline`). */
int32_t cm_kprof_enable(int32_t on);
int32_t cm_kprof_report(char* buf, size_t buf_len);
/* Restrict the timing to one kernel class (a key of cm_kprof_report); NULL or "" = every class. */
int32_t cm_kprof_filter(const char* name);
/* cells = sum over committed columns of trees 0,1,2 of 2^log_size. */
int32_t cm_proof_stats(const cm_proof* p, uint64_t* cells, uint64_t* steps, double* phase_ms, uint32_t n_phases);

#ifdef __cplusplus
}
#endif
#endif /* CAIROM_HIP_H */
