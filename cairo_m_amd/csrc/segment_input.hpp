// Device-resident prover input and the input-level steps every whole-segment driver shares: the single-GPU and sharded provers
// (prover.hip) and the PCS-free AIR check (check.hip).
#pragma once
#include "../../include/cairom_hip.h"
#include "prover_common.hpp"
#include "gpu_air.hpp"
#include "point_eval.hpp"
#include <string>

namespace cm {

inline uint32_t log_size_for(uint64_t n) {  // max(LOG_N_LANES, ceil_log2(n))
  uint32_t l = 4;
  while ((1ull << l) < n) l++;
  return l;
}

// ---- device-resident prover input ------------------------------------------------------------------------
struct DeviceInput {
  cm_prover_input meta;  // scalar fields + counts; pointers are replaced by device pointers below
  DevBuf bundles[CM_N_OPCODE_COMPONENTS], data_accesses, init_mem, fin_mem, clock_updates, init_tree, fin_tree;
  PublicData public_data;
};

// bytes of the pool blocks a resident input occupies: every array at its size, pool-rounded (an empty array is a 4-byte block)
inline uint64_t device_input_bytes(const DeviceInput& d) {
  uint64_t n = 0;
  auto add = [&](const DevBuf& b) { if (b.p) n += pool_round(b.bytes); };
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) add(d.bundles[i]);
  add(d.data_accesses); add(d.init_mem); add(d.fin_mem); add(d.clock_updates); add(d.init_tree); add(d.fin_tree);
  return n;
}
// log2 rows of every component, known from the input lengths (Claim::log_sizes)
inline void component_logs(const cm_prover_input& in, uint32_t* clog) {
  uint64_t nrows[air::N_COMPONENTS] = {0};
  for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++) nrows[c] = in.n_bundles[c];
  nrows[air::C_MEMORY] = in.n_initial_memory + in.n_final_memory;
  nrows[air::C_MERKLE] = in.n_initial_tree + in.n_final_tree;
  nrows[air::C_CLOCK_UPDATE] = in.n_clock_updates;
  nrows[air::C_POSEIDON2] = in.n_initial_tree + in.n_final_tree;
  for (int c = 0; c <= air::C_POSEIDON2; c++) clog[c] = log_size_for(nrows[c]);
  clog[air::C_RC8] = 8; clog[air::C_RC16] = 16; clog[air::C_RC20] = 20; clog[air::C_BITWISE] = 18;
}
static_assert(sizeof(cm_relations) == sizeof(DevRelations), "cm_relations must mirror DevRelations");
// Relations::draw (prover.rs:94): (z, alpha) per relation, alpha powers for the device
inline void draw_relations(hostch::Channel& ch, HostRelations& hrel, DevRelations& drel_h) {
  for (int r = 0; r < air::N_RELATIONS; r++) {
    QM31 z, alpha;
    ch.draw_two_felts(z, alpha);
    hrel.z[r] = z;
    QM31 cur(M31(1));
    for (int i = 0; i < air::MAX_REL_SIZE; i++) { hrel.alpha_pow[r][i] = cur; cur = cur * alpha; }
    z.to_u32(drel_h.z[r]);
    for (int i = 0; i < air::MAX_REL_SIZE; i++) hrel.alpha_pow[r][i].to_u32(drel_h.alpha_pow[r][i]);
  }
}

// public_data.rs:291-394: the LogUp contribution of the public data (the verifier's initial_logup_sum); per_relation (optional)
// receives its part per relation (registers, merkle, memory; zero for the others).  verifier.hip
QM31 public_logup_sum(const PublicData& d, const HostRelations& rel, QM31* per_relation = nullptr);

// What the AIR check (check.hip) built and the relation tracker (track.hip) reads after it: the trace-domain columns of trees 0
// and 1, where each component's columns start, and the relations on both sides.
struct CheckColumns {
  ColumnSet pp, tr;
  std::vector<size_t> tr0;
  uint32_t clog[air::N_COMPONENTS];
  DevBuf drel;
  HostRelations hrel;
};
// The PCS-free AIR check of a whole segment; keep (optional) receives the columns instead of the check releasing them.
void check_segment(const DeviceInput& din, const cm_relations* relations, cm_check_report& rep, CheckColumns* keep = nullptr);

// Link diff of a run (link.hip): prev's final boundary memory against next's initial one.  rep.struct_size is kept; seg_index = the
// index of `next` in its run (the report's first sentence names it).  cells: room for `cap` records; n_total: all there are.
void link_diff(const DeviceInput& prev, const DeviceInput& next, uint32_t seg_index, cm_link_report& rep, cm_link_cell* cells, uint64_t cap,
               uint64_t& n_total);
// The diff's first half for any two row arrays in ascending address order (device pointers; `a` in the role of prev, `b` of next,
// n_a + n_b > 0): the classification of every row into its slot of the merged order, and with_scan the exclusive sum of the listed
// flags.  state[LS_*] = the totals.  Enqueued on st; the buffers live in `m`.  The segment write set (mem_transition.hip) runs it
// over one input's initial and final boundary memory.
enum : uint32_t { LS_CHANGED = 0, LS_ONLY_NEXT = 1, LS_ONLY_PREV = 2, LS_ZERO_ONLY = 3, LS_ERR = 4, LS_WORDS = 8 };
struct LinkMerge {
  DevBuf state, flag, pos, src, tmp;
  const uint32_t* prev = nullptr;
  const uint32_t* next = nullptr;
  uint32_t n_prev = 0, n_next = 0, n_slots = 0;
};
void link_merge_enqueue(const uint32_t* a, uint64_t n_a, const uint32_t* b, uint64_t n_b, bool with_scan, LinkMerge& m, hipStream_t st);
// out[p] = the address of the p-th listed cell, p < cap (ascending: the merged order is); needs the scan
void link_addresses_enqueue(const LinkMerge& m, uint32_t* out, uint32_t cap, hipStream_t st);
// *missing (device) = the lowest listed address that is not in the ascending device array set[0 .. n_set), or 0xffffffff
void link_missing_enqueue(const LinkMerge& m, const uint32_t* set, uint32_t n_set, uint32_t* missing, hipStream_t st);
// link i of a checked run into its record: cells + i * cap_per_link receive the cells
void check_link_into(const DeviceInput& prev, const DeviceInput& next, uint32_t i, cm_run_check& rec, cm_link_cell* cells, uint64_t cap_per_link);
// the line cm_check_run / cm_check_chain leave for cm_last_error(): the first bad link or segment, or empty
std::string run_check_summary(const cm_run_check* out, uint32_t n, bool with_air);

}  // namespace cm
