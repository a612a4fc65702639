// Device-memory estimate of one proof (cm_estimate_memory*, include/cairom_hip.h): host arithmetic only.
//
// The estimate walks the allocations of SegmentProver (prover.hip) in the order it makes them and charges every pool block at
// the capacity the pool may hand out for it: Pool::round of the request plus the 25 % a best-fit block may waste (Pool::get).
// Two points of a proof can be the widest one:
//   * the end of the interaction phase: twiddles, the constant columns, the trace-domain evaluations of tree 1 (tr_evals), trees
//     0 / 1 / 2 (coefficients, LDE, Merkle layers), the LogUp tail's scratch;
//   * the FRI commit phase: all of the above WITHOUT tr_evals (released when the claimed sums have been mixed), plus the
//     evaluation-domain copies of a blowup > 1, the composition accumulators and tree 3, the sampling scratch, the DEEP quotient
//     columns, the FRI layers with their trees, the decommitment gather (the coefficient columns are only given back under the
//     FRI kernels, after everything of FRI has been allocated).
// working_bytes is the larger of the two.  Every term is monotone in every component's log size and in the blowup: where the
// prover's real footprint depends on how many DISTINCT sizes there are (composition accumulators, quotient columns), the term is
// the geometric bound over all sizes below the largest, which no assignment of sizes exceeds.
// One rank of the sharded prover (world > 1) holds its own columns whole, then row slices of everybody's columns, exchange
// staging inside the pool's arena and the slices of split components; the bound charges the single-GPU sum of everything plus
// 1 / world of it again and does not yet credit what sharding saves — measured per-rank peaks are in DESIGN 3.5.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "gpu_air.hpp"
#include <algorithm>

namespace cm {

struct MemSwitches { bool pp_cache, tw_cache, defer_teardown; };

struct MemEstimator {
  uint64_t sum = 0;
  // one pool block: the capacity class of the request plus the best-fit slack
  static uint64_t blk(uint64_t bytes) {
    const uint64_t r = pool_round((size_t)std::max<uint64_t>(bytes, 4));
    return r + r / 4;
  }
  // the layers of a Merkle tree whose leaf layer has 2^top nodes: one block of 32 << k bytes per layer k
  static uint64_t merkle(uint32_t top) {
    uint64_t s = 0;
    for (uint32_t k = 0; k <= top; k++) s += blk((uint64_t)32 << k);
    return s;
  }
};

// blocks that are not enumerated below: pointer tables, argument arrays, transcript words, the per-launch job uploads — about
// 1500 requests per proof, none above a few hundred KiB and most of one 512-byte class
constexpr uint64_t MEM_SMALL_BLOCKS_ALLOWANCE = (uint64_t)32 << 20;

inline void estimate_memory(const uint32_t clog[air::N_COMPONENTS], const cm_pcs_config& cfg, uint32_t world, const MemSwitches& sw,
                            cm_mem_estimate& out) {
  using E = MemEstimator;
  const uint32_t B = cfg.log_blowup_factor;
  uint32_t L = 0;
  for (int c = 0; c < air::N_COMPONENTS; c++) L = std::max(L, clog[c]);
  const uint32_t comp_log = L + 1, R = comp_log + B;
  uint64_t n_pp = 0, n_tr = 0, n_it = 0, cols_tr = 0, cols_it = 0, n_constraints = 0;
  for (int i = 0; i < air::N_PREPROC; i++) n_pp += (uint64_t)1 << air::PREPROC_LOG[i];
  uint64_t logup_scratch = 0, slots = 0, eval_partials = 0;
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    n_tr += (uint64_t)info.n_trace << clog[c];
    n_it += (uint64_t)info.n_interaction << clog[c];
    cols_tr += info.n_trace; cols_it += info.n_interaction;
    n_constraints += info.n_constraints;
    // LogUp tail (logup_finalize_all): a linear-scan row buffer below 2^13 rows, two piece-total buffers above; the envelope of both
    logup_scratch += std::max<uint64_t>((uint64_t)16 << std::min<uint32_t>(clog[c], 12), clog[c] >= 13 ? (uint64_t)4096 << (clog[c] - 11) : 0);
    // private accumulator slots of the small evaluation sizes (composition(): SLOT_MAX_LOG = 15)
    slots += (uint64_t)16 << std::min<uint32_t>(clog[c] + 1, 15);
    // eval_at_point_multi: 16 bytes per column and group of 2^15 coefficients, once more for the previous-row mask of four columns
    eval_partials += (uint64_t)16 * (info.n_trace + info.n_interaction + 4) * std::max<uint64_t>(1, (uint64_t)1 << (clog[c] > 15 ? clog[c] - 15 : 0));
  }
  const uint64_t cols_all = cols_tr + cols_it + air::N_PREPROC + 4;

  // ---- alive from setup / trace_commit / interaction to the end of the proof ----
  uint64_t tw_bytes = 0;   // ProofTwiddles::build: x, ix (2^(R-1) words), y, iy (2^R words), the build scratch
  tw_bytes += 2 * E::blk((uint64_t)4 << (R - 1)) + 2 * E::blk((uint64_t)4 << R) + E::blk((uint64_t)twiddles_scratch_words(R) * 4);
  const uint64_t tw_cached = 2 * ((uint64_t)4 << (R - 1)) + 2 * ((uint64_t)4 << R) + (uint64_t)twiddles_scratch_words(R) * 4;   // hipMalloc, no pool
  const uint64_t pp_evals = E::blk(4 * n_pp);
  const uint64_t tree0 = E::blk(4 * n_pp) + E::blk((4 * n_pp) << B) + E::merkle(20 + B) + E::blk(64 * air::N_PREPROC);
  const uint64_t tr_evals = E::blk(4 * n_tr);
  const uint64_t tree1 = E::blk(4 * n_tr) + E::blk((4 * n_tr) << B) + E::merkle(L + B) + E::blk(64 * cols_tr);
  const uint64_t tree2 = E::blk(4 * n_it) + E::blk((4 * n_it) << B) + E::merkle(L + B) + E::blk(64 * cols_it);   // (coefficients = the evaluation arena)
  const uint64_t logup = E::blk(logup_scratch) * 2 + E::blk((uint64_t)air::N_COMPONENTS * 1024 * 16) + E::blk(32 * 64 * 2 * 16);
  uint64_t early = pp_evals + tree0 + tree1 + tree2 + logup;
  if (!sw.tw_cache) early += tw_bytes;

  // ---- allocated behind the interaction phase ----
  uint64_t late = 0;
  if (B > 1) late += E::blk(8 * n_pp) + E::blk(8 * n_tr) + E::blk(8 * n_it);       // evaluation-domain copies of trees 0..2
  late += E::blk(16 * n_constraints);                                              // coefficient powers
  late += 2 * E::blk((uint64_t)16 << comp_log);                                    // acc_top; acc_rest <= sum of all smaller sizes
  late += E::blk(slots + 32);
  const uint64_t tree3 = E::blk((uint64_t)16 << (comp_log + B)) + E::merkle(comp_log + B);   // (its coefficients are acc_top)
  late += tree3;
  late += E::blk(8 * cols_all * 2) + E::blk(16 * cols_all * 2);                    // sampling table, sampled values
  late += E::blk(eval_partials + 64 * (((uint64_t)16 << 10) + ((uint64_t)16 << (comp_log > 10 ? comp_log - 10 : 0))));
  const uint64_t quot_blob = E::blk(cols_all * 2 * 48 + 64 * 256);
  // DEEP quotient columns: four per distinct LDE size; the largest plus at most as much again for all smaller sizes together
  const uint64_t quot_cols = 2 * E::blk((uint64_t)16 << (comp_log + B));
  // FRI: the first-layer tree over the quotient columns, then per inner layer four columns and a tree (summed down to one row:
  // the layers below log_last_layer_degree_bound + blowup that a config leaves out are a rounding error)
  uint64_t fri = E::merkle(comp_log + B) + E::blk(4096);
  for (uint32_t l = 1; l < comp_log + B; l++) fri += E::blk((uint64_t)16 << l) + E::merkle(l);
  // decommitment gather (GatherBatch, the host-driven tail): address tables + results of every tree's walk
  const uint64_t Q = cfg.n_queries, D = comp_log + B;
  const uint64_t gather = E::blk(Q * D * (D + 5) * 2 * 40) + E::blk(Q * cols_all * 2 * 16) + E::blk(Q * D * 16 * 24);
  late += quot_blob + quot_cols + fri + gather;

  const uint64_t single = early + std::max(tr_evals, late) + MEM_SMALL_BLOCKS_ALLOWANCE;
  if (world <= 1) out.working_bytes = single;
  else {
    const uint64_t all = early + tr_evals + late + MEM_SMALL_BLOCKS_ALLOWANCE;
    out.working_bytes = all + all / world;
  }
  uint64_t cached = 0;
  if (sw.pp_cache) cached += pp_evals + tree0;
  if (sw.tw_cache) cached += tw_cached;
  if (sw.defer_teardown && world <= 1) cached += quot_blob + quot_cols + fri;
  out.cached_bytes = cached;
}

// the resident cm_device_input of a host input: every array at its struct size, pool-rounded (an empty array is a 4-byte block)
inline uint64_t estimate_input_bytes(const cm_prover_input& in) {
  uint64_t n = 0;
  auto add = [&](uint64_t count, size_t each) { n += pool_round((size_t)std::max<uint64_t>(count * each, 4)); };
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) add(in.n_bundles[i], sizeof(cm_bundle));
  add(in.n_data_accesses, sizeof(cm_data_access));
  add(in.n_initial_memory, sizeof(cm_memory_cell));
  add(in.n_final_memory, sizeof(cm_memory_cell));
  add(in.n_clock_updates, sizeof(cm_clock_update));
  add(in.n_initial_tree, sizeof(cm_merkle_node));
  add(in.n_final_tree, sizeof(cm_merkle_node));
  return n;
}

}  // namespace cm
