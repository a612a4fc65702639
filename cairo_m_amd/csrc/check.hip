// PCS-free AIR check of a whole segment (reference: debug_tools::assert_constraints, crates/prover/src/debug_tools/
// assert_constraints.rs:24-60).  Of the reference's relation_tracker this file has the per-relation SUMS (which relation does not
// balance); the summary of the tuples that do not cancel is track.hip, which runs this check first and keeps its columns.
// The prover's own trace-generation, histogram, preprocessed-column and
// LogUp kernels on trace-domain buffers only — no twiddles, LDE, Merkle trees or FRI — then the check kernels of kernels_check.inc
// for all 34 components and the public data's LogUp contribution per relation.  One host round trip at the end (two when a lookup
// value was out of range).  Threading as cm_prove_device: the calling thread's main stream and device pool.
#include "../../include/cairom_hip.h"
#include "segment_input.hpp"
#include "handles.hpp"
#include "abi.hpp"
#include "air_kernels.hpp"
#include "check_kernels.hpp"
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

const char* const RELATION_NAMES[air::N_RELATIONS] = {"registers", "memory", "merkle", "poseidon2",
                                                      "range_check_8", "range_check_16", "range_check_20", "bitwise"};
const char* const TABLE_NAMES[4] = {"rc8", "rc16", "rc20", "bitwise"};

void host_relations(const DevRelations& w, HostRelations& h) {
  for (int r = 0; r < air::N_RELATIONS; r++) {
    h.z[r] = QM31::from_u32(w.z[r]);
    for (int i = 0; i < air::MAX_REL_SIZE; i++) h.alpha_pow[r][i] = QM31::from_u32(w.alpha_pow[r][i]);
  }
}
// 64-bit sums of canonical words (k_relsum) -> QM31
QM31 reduce_words(const unsigned long long* w) {
  return QM31(M31::reduce(w[0]), M31::reduce(w[1]), M31::reduce(w[2]), M31::reduce(w[3]));
}
void set_message(cm_check_report& rep, const std::string& m) {
  const size_t n = std::min(m.size(), sizeof(rep.message) - 1);
  memcpy(rep.message, m.data(), n);
  rep.message[n] = 0;
}

}  // namespace

void check_segment(const DeviceInput& din, const cm_relations* relations, cm_check_report& rep, CheckColumns* keep) {
  static_assert(CM_N_COMPONENTS == air::N_COMPONENTS && CM_N_RELATIONS == air::N_RELATIONS, "report dimensions");
  static_assert(sizeof(cm_check_report) % 8 == 0 && offsetof(cm_check_report, row) == 16, "cm_check_report: plain words");
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  const cm_prover_input& in = din.meta;
  constexpr int NC = air::N_COMPONENTS;
  CheckColumns own;
  CheckColumns& cols = keep ? *keep : own;
  uint32_t* const clog = cols.clog;
  component_logs(in, clog);
  for (int c = 0; c < NC; c++) CM_CHECK(clog[c] <= 26, "component too large");

  // ---- preprocessed columns, execution trace + lookup multiplicities (as SegmentProver::trace_commit, on one stream) ----
  ColumnSet& pp_evals = cols.pp;
  ColumnSet& tr_evals = cols.tr;
  ColumnSet it_evals;
  pp_evals.alloc(std::vector<uint32_t>(air::PREPROC_LOG, air::PREPROC_LOG + air::N_PREPROC), st);
  launch_preproc_all(pp_evals.ptrs.data(), st);
  std::vector<size_t>& tr0 = cols.tr0;
  std::vector<size_t> it0(NC);
  tr0.assign(NC, 0);
  {
    std::vector<uint32_t> tl, il;
    for (int c = 0; c < NC; c++) {
      tr0[c] = tl.size(); tl.insert(tl.end(), air::component_info(c).n_trace, clog[c]);
      it0[c] = il.size(); il.insert(il.end(), air::component_info(c).n_interaction, clog[c]);
    }
    tr_evals.alloc(tl, st);
    it_evals.alloc(il, st);
  }
  // results: [flag (u32) pad][failing rows: NC u64][first key: NC u64][relation sums: NC x 8 x 4 u64][claimed sums: NC x 4 u32]
  const size_t o_fail = 8, o_first = o_fail + 8 * NC, o_rel = o_first + 8 * NC, o_sums = o_rel + 8 * NC * 32;
  const size_t res_bytes = o_sums + 16 * NC;
  DevBuf res(res_bytes);
  uint8_t* const rp = res.as<uint8_t>();
  CM_HIP(hipMemsetAsync(rp, 0, o_first, st));
  CM_HIP(hipMemsetAsync(rp + o_first, 0xFF, o_rel - o_first, st));
  CM_HIP(hipMemsetAsync(rp + o_rel, 0, res_bytes - o_rel, st));
  unsigned long long* const d_fail = (unsigned long long*)(rp + o_fail);
  unsigned long long* const d_first = (unsigned long long*)(rp + o_first);
  unsigned long long* const d_rel = (unsigned long long*)(rp + o_rel);
  uint32_t* const d_sums = (uint32_t*)(rp + o_sums);
  HistPtrs h;
  h.rc8 = tr_evals.ptrs[tr0[air::C_RC8]]; h.rc16 = tr_evals.ptrs[tr0[air::C_RC16]];
  h.rc20 = tr_evals.ptrs[tr0[air::C_RC20]]; h.bitwise = tr_evals.ptrs[tr0[air::C_BITWISE]];
  h.error_flag = (uint32_t*)rp;
  CM_HIP(hipMemsetAsync(h.rc8, 0, 4u << 8, st));
  CM_HIP(hipMemsetAsync(h.rc16, 0, 4u << 16, st));
  CM_HIP(hipMemsetAsync(h.rc20, 0, 4u << 20, st));
  CM_HIP(hipMemsetAsync(h.bitwise, 0, 4u << 18, st));
  const auto small = [&](int c) { return clog[c] <= SMALL_COMPONENT_MAX_LOG; };
  {
    std::vector<SmallTraceJob> jobs;
    for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++)
      if (small(c)) jobs.push_back(SmallTraceJob{din.bundles[c].p, (uint32_t)in.n_bundles[c], tr_evals.dev(tr0[c]), clog[c], c});
    DevBuf d_jobs = upload(jobs, st);
    launch_trace_hist_small(d_jobs.as<SmallTraceJob>(), (uint32_t)jobs.size(), din.data_accesses.p, h, st);
    for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++)
      if (!small(c))
        launch_opcode_trace_hist(c, din.bundles[c].p, (uint32_t)in.n_bundles[c], din.data_accesses.p, clog[c], tr_evals.dev(tr0[c]), h, st);
    launch_memory_trace(din.init_mem.p, (uint32_t)in.n_initial_memory, din.fin_mem.p, (uint32_t)in.n_final_memory, in.initial_root,
                        in.final_root, clog[air::C_MEMORY], tr_evals.dev(tr0[air::C_MEMORY]), st);
    launch_merkle_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree, in.initial_root,
                        in.final_root, clog[air::C_MERKLE], tr_evals.dev(tr0[air::C_MERKLE]), st);
    launch_clock_update_trace(din.clock_updates.p, (uint32_t)in.n_clock_updates, clog[air::C_CLOCK_UPDATE],
                              tr_evals.dev(tr0[air::C_CLOCK_UPDATE]), st);
    launch_poseidon2_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree,
                           clog[air::C_POSEIDON2], tr_evals.dev(tr0[air::C_POSEIDON2]), st);
  }

  // ---- relations: the caller's, or drawn from a fresh default channel (assert_constraints.rs:42) ----
  DevRelations drel_h;
  HostRelations& hrel = cols.hrel;
  if (relations) {
    memcpy(&drel_h, relations, sizeof(DevRelations));
    host_relations(drel_h, hrel);
  } else {
    hostch::Channel ch;
    draw_relations(ch, hrel, drel_h);
  }
  memcpy(&rep.relations, &drel_h, sizeof(DevRelations));
  DevBuf& drel = cols.drel;
  drel.alloc(sizeof(DevRelations));
  stage_upload(drel.p, &drel_h, sizeof(DevRelations), st);
  const DevRelations* const d_rels = drel.as<DevRelations>();
  const uint32_t* const* const d_pp = (const uint32_t* const*)pp_evals.dev();

  // ---- interaction columns and claimed sums (as SegmentProver::interaction) ----
  {
    std::vector<SmallLogupJob> jobs;
    std::vector<LogupTailJob> tail(NC);
    uint32_t small_max = 0;
    for (int c = 0; c < NC; c++) {
      const air::ComponentInfo& info = air::component_info(c);
      for (int k = 0; k < 4; k++) tail[c].col[k] = it_evals.ptrs[it0[c] + info.n_interaction - 4 + k];
      tail[c].log_size = clog[c];
      if (small(c)) { jobs.push_back(SmallLogupJob{(const uint32_t* const*)tr_evals.dev(tr0[c]), it_evals.dev(it0[c]), clog[c], c}); small_max = std::max(small_max, clog[c]); }
    }
    DevBuf d_jobs = upload(jobs, st);
    launch_logup_small(d_jobs.as<SmallLogupJob>(), (uint32_t)jobs.size(), small_max, d_pp, d_rels, st);
    for (int c = 0; c < NC; c++)
      if (!small(c)) launch_logup(c, (const uint32_t* const*)tr_evals.dev(tr0[c]), d_pp, clog[c], d_rels, it_evals.dev(it0[c]), st);
    logup_finalize_all(tail, d_sums, st);
  }

  // ---- constraint check and relation sums of every component ----
  std::vector<CheckArgs> cargs(NC);
  std::vector<RelSumArgs> rargs(NC);
  for (int c = 0; c < NC; c++) {
    CheckArgs& a = cargs[c];
    a.tr = (const uint32_t* const*)tr_evals.dev(tr0[c]); a.it = (const uint32_t* const*)it_evals.dev(it0[c]); a.pp = d_pp;
    a.rels = d_rels; a.claimed_sum = d_sums + 4 * c; a.row_status = nullptr;
    a.failing_rows = d_fail + c; a.first = d_first + c;
    a.log_size = clog[c]; a.n_base = air::component_info(c).n_base_constraints;
    RelSumArgs& b = rargs[c];
    b.tr = a.tr; b.pp = d_pp; b.rels = d_rels; b.sums = d_rel + 32 * c; b.log_size = clog[c];
  }
  {
    std::vector<CheckArgs> sc;
    std::vector<RelSumArgs> sr;
    std::vector<int> ids;
    for (int c = 0; c < NC; c++)
      if (small(c)) { sc.push_back(cargs[c]); sr.push_back(rargs[c]); ids.push_back(c); }
    UploadBatch ub;
    CheckArgs* d_sc = nullptr; RelSumArgs* d_sr = nullptr; int* d_ids = nullptr;
    ub.add(sc, &d_sc); ub.add(sr, &d_sr); ub.add(ids, &d_ids);
    DevBuf tabs = ub.flush(st);
    launch_check_small(d_sc, d_ids, (uint32_t)ids.size(), st);
    launch_relsum_small(d_sr, d_ids, (uint32_t)ids.size(), st);
    for (int c = 0; c < NC; c++)
      if (!small(c)) { launch_check(c, cargs[c], st); launch_relsum(c, rargs[c], st); }
    std::vector<uint8_t> host(res_bytes);
    CM_HIP(hipMemcpyAsync(host.data(), rp, res_bytes, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));   // (also keeps every temporary above alive until the kernels have read it)

    // ---- report ----
    const uint32_t flag = *(const uint32_t*)host.data();
    const unsigned long long* fail = (const unsigned long long*)(host.data() + o_fail);
    const unsigned long long* first = (const unsigned long long*)(host.data() + o_first);
    const unsigned long long* rel = (const unsigned long long*)(host.data() + o_rel);
    const uint32_t* sums = (const uint32_t*)(host.data() + o_sums);
    QM31 total;
    for (int c = 0; c < NC; c++) {
      rep.failing_rows[c] = fail[c];
      rep.first_constraint[c] = fail[c] ? (int32_t)(first[c] & 0xffffu) : -1;
      rep.first_row[c] = fail[c] ? first[c] >> 16 : 0;
      memcpy(rep.claimed_sum[c], sums + 4 * c, 16);
      total += QM31::from_u32(sums + 4 * c);
      for (int r = 0; r < air::N_RELATIONS; r++) reduce_words(rel + 32 * c + 4 * r).to_u32(rep.relation_sum[c][r]);
    }
    QM31 pub[air::N_RELATIONS];
    total += public_logup_sum(din.public_data, hrel, pub);
    for (int r = 0; r < air::N_RELATIONS; r++) pub[r].to_u32(rep.public_sum[r]);
    total.to_u32(rep.total);
    rep.status = 0; rep.component = -1; rep.constraint = -1; rep.reserved = 0; rep.row = 0;
    set_message(rep, "");
    if (flag) {
      // which (component, row, table): a follow-up pass over the opcode components (the histogram kernels only raise a flag)
      DevBuf key(8);
      CM_HIP(hipMemsetAsync(key.p, 0xFF, 8, st));
      for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++)
        launch_lookup_diag(c, (const uint32_t* const*)tr_evals.dev(tr0[c]), clog[c], key.as<unsigned long long>(), st);
      unsigned long long k = ~0ull;
      CM_HIP(hipMemcpyAsync(&k, key.p, 8, hipMemcpyDeviceToHost, st));
      CM_HIP(hipStreamSynchronize(st));
      rep.status = 1;
      if (k != ~0ull) {
        rep.component = (int32_t)(k >> 40); rep.constraint = (int32_t)(k & 0xff); rep.row = (k >> 8) & 0xffffffffu;
        set_message(rep, std::string("lookup value out of range for ") + TABLE_NAMES[rep.constraint] + ": " + air::component_name(rep.component) +
                             " row " + std::to_string(rep.row));
      } else {
        set_message(rep, "lookup value out of range for an unidentified table");
      }
      return;
    }
    for (int c = 0; c < NC; c++)
      if (fail[c]) {
        rep.status = 2; rep.component = c; rep.constraint = rep.first_constraint[c]; rep.row = rep.first_row[c];
        set_message(rep, std::string(air::component_name(c)) + ": constraint " + std::to_string(rep.constraint) + " fails on row " +
                             std::to_string(rep.row));
        return;
      }
    if (!total.is_zero()) {
      std::string m = "LogUp sums do not cancel:";
      const char* sep = " ";
      for (int r = 0; r < air::N_RELATIONS; r++) {
        QM31 s = pub[r];
        for (int c = 0; c < NC; c++) s += QM31::from_u32(rep.relation_sum[c][r]);
        if (!s.is_zero()) { m += sep; m += RELATION_NAMES[r]; sep = ", "; }
      }
      rep.status = 3;
      set_message(rep, m);
    }
  }
}

}  // namespace cm

// ================================================================= C ABI
namespace {
std::vector<uint32_t*> column_handles(const cm_handle* h, int n) {
  CM_CHECK(h || n == 0, "null column array");
  return cm::handles(h, n);
}
}  // namespace

extern "C" {
int32_t cm_check_constraints(const cm_device_input* input, const cm_relations* relations, cm_check_report* out) {
  return cm::abi_guard([&] {
    CM_CHECK(input && input->d && out, "cm_check_constraints: null input / report");
    memset(out, 0, sizeof(*out));
    cm::check_segment(*input->d, relations, *out);
  });
}
int32_t cm_constraints_check(int32_t c, const cm_handle* trace_cols, const cm_handle* interaction_cols, const cm_handle* preprocessed,
                             uint32_t log_size, const cm_relations* relations, const uint32_t claimed_sum[4], cm_handle row_status,
                             uint64_t* failing_rows, int32_t* first_constraint, uint64_t* first_row, cm_stream_t s) {
  return cm::abi_guard([&] {
    using namespace cm;
    CM_CHECK(c >= 0 && c < air::N_COMPONENTS, "bad component id");
    CM_CHECK(log_size >= 4 && log_size <= 26, "cm_constraints_check: log_size must be in 4..26");
    CM_CHECK(relations && claimed_sum, "cm_constraints_check: null relations / claimed sum");
    bind_thread_to_library_device();
    const hipStream_t st = cm::as_stream(s);
    const air::ComponentInfo& info = air::component_info(c);
    UploadBatch ub;
    uint32_t** d_tr = nullptr; uint32_t** d_it = nullptr; uint32_t** d_pp = nullptr; uint32_t* d_cs = nullptr;
    ub.add(column_handles(trace_cols, info.n_trace), &d_tr);
    ub.add(column_handles(interaction_cols, info.n_interaction), &d_it);
    ub.add(column_handles(preprocessed, air::N_PREPROC), &d_pp);
    ub.add(std::vector<uint32_t>(claimed_sum, claimed_sum + 4), &d_cs);
    DevBuf tabs = ub.flush(st), drel(sizeof(DevRelations)), out(16);
    stage_upload(drel.p, relations, sizeof(DevRelations), st);
    CM_HIP(hipMemsetAsync(out.p, 0, 8, st));
    CM_HIP(hipMemsetAsync(out.as<uint8_t>() + 8, 0xFF, 8, st));
    CheckArgs a;
    a.tr = (const uint32_t* const*)d_tr; a.it = (const uint32_t* const*)d_it; a.pp = (const uint32_t* const*)d_pp;
    a.rels = drel.as<DevRelations>(); a.claimed_sum = d_cs; a.row_status = cm::as_words(row_status);
    a.failing_rows = out.as<unsigned long long>(); a.first = out.as<unsigned long long>() + 1;
    a.log_size = log_size; a.n_base = info.n_base_constraints;
    launch_check(c, a, st);
    unsigned long long r[2] = {0, 0};
    CM_HIP(hipMemcpyAsync(r, out.p, 16, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    if (failing_rows) *failing_rows = r[0];
    if (first_constraint) *first_constraint = r[0] ? (int32_t)(r[1] & 0xffffu) : -1;
    if (first_row) *first_row = r[0] ? r[1] >> 16 : 0;
  });
}
int32_t cm_relation_sums(int32_t c, const cm_handle* trace_cols, const cm_handle* preprocessed, uint32_t log_size,
                         const cm_relations* relations, uint32_t sums[CM_N_RELATIONS][4], cm_stream_t s) {
  return cm::abi_guard([&] {
    using namespace cm;
    CM_CHECK(c >= 0 && c < air::N_COMPONENTS, "bad component id");
    CM_CHECK(log_size >= 4 && log_size <= 26, "cm_relation_sums: log_size must be in 4..26");
    CM_CHECK(relations && sums, "cm_relation_sums: null relations / output");
    bind_thread_to_library_device();
    const hipStream_t st = cm::as_stream(s);
    UploadBatch ub;
    uint32_t** d_tr = nullptr; uint32_t** d_pp = nullptr;
    ub.add(column_handles(trace_cols, air::component_info(c).n_trace), &d_tr);
    ub.add(column_handles(preprocessed, air::N_PREPROC), &d_pp);
    DevBuf tabs = ub.flush(st), drel(sizeof(DevRelations)), out(8 * 32);
    stage_upload(drel.p, relations, sizeof(DevRelations), st);
    CM_HIP(hipMemsetAsync(out.p, 0, 8 * 32, st));
    RelSumArgs a;
    a.tr = (const uint32_t* const*)d_tr; a.pp = (const uint32_t* const*)d_pp; a.rels = drel.as<DevRelations>();
    a.sums = out.as<unsigned long long>(); a.log_size = log_size;
    launch_relsum(c, a, st);
    unsigned long long w[32];
    CM_HIP(hipMemcpyAsync(w, out.p, sizeof(w), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    for (int r = 0; r < CM_N_RELATIONS; r++) reduce_words(w + 4 * r).to_u32(sums[r]);
  });
}
}  // extern "C"
