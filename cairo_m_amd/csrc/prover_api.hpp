// What the C-ABI files (api_prove.hip, api_run.hip, api_verify.hip) call in the prover, the run object and the verifiers, and the
// prototypes prover.hip needs of the translation units next to it.  CM_INTERNAL: what was file-local before this header existed.
#pragma once
#include "../../include/cairom_hip.h"
#include "abi.hpp"
#include "handles.hpp"
#include "segment_input.hpp"
#include "mem_estimate.hpp"
#include "verify_device.hpp"
#include <atomic>
#include <mutex>
#include <string>
#include <vector>

namespace cm {

// ---- inputs (prover.hip, adapter_device.hip) ---------------------------------------------------------------------------------
DeviceInput* upload_input(const cm_prover_input& in, hipStream_t st = nullptr);
DeviceInput* adapt_segment_device(const cm_runner_segment& seg);
void download_input(const DeviceInput& d, host::ProverInputOwned& o);   // back to the host (tests)

// ---- one proof (prover.hip, prover_sharded.inc) ------------------------------------------------------------------------------
ProofData* prove(const DeviceInput& din, const cm_pcs_config& cfg);
ProofData* prove_sharded(const DeviceInput& din, const cm_pcs_config& cfg, const cm_comm& comm_c);
// the ownership plan of a sharded proof (prover_sharded.inc says how it is packed)
struct ShardPlan {
  int owner[air::N_COMPONENTS];          // rank that owns the whole component; -1 = split over all ranks
  std::vector<int> tr_owner, it_owner;   // owner of every column of trees 1 / 2 (global column order)
  std::vector<size_t> tr0, it0;          // first column of every component in trees 1 / 2
  uint64_t load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool split(int c) const { return owner[c] < 0; }
  int cum_owner(int c) const { return it_owner[it0[c] + air::component_info(c).n_interaction - 4]; }   // the cumulative-sum columns
};
CM_INTERNAL ShardPlan make_shard_plan(const uint32_t* clog, uint32_t world, bool allow_split = true);
CM_INTERNAL uint64_t shard_staging_words(const uint32_t* clog, const ShardPlan& p, uint32_t world);

// ---- the pipelines (prover.hip): every item proved or given up on return; the first error of a worker or producer is thrown ----
CM_INTERNAL void prove_many(const cm_device_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs);
CM_INTERNAL void prove_many_host(const cm_prover_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs);
CM_INTERNAL void prove_many_segments(const cm_runner_segment* const* segments, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                                     cm_proof** outs);
CM_INTERNAL void check_run_segment(const cm_run_segment* seg, const char* who);
CM_INTERNAL void prove_run(const char* who, Run& run, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                           cm_proof** outs, cm_mem_transition** transitions);

// ---- process-wide switches of the prover and what the memory estimate reads of them (prover.hip) ------------------------------
CM_INTERNAL extern std::atomic<int> g_pp_cache, g_tw_cache;   // -1 = the environment decides, 0 / 1 = cm_set_*_cache
CM_INTERNAL MemSwitches mem_switches();

// ---- the run object (adapter_run.inc) and the openers under its image (mem_open.hip, mem_range.hip, mem_set.hip, mem_transition.hip) ----
Run* run_begin(const uint32_t* initial_memory, uint64_t n_initial_memory, const uint32_t* initial_heap, uint64_t n_initial_heap, const uint32_t ranges[6]);
DeviceInput* run_adapt_next(Run& run, const cm_run_segment& seg);
void run_memory(Run& r, uint32_t* locals, uint64_t cap_l, uint64_t* n_l, uint32_t* heap, uint64_t cap_h, uint64_t* n_h);
uint64_t run_image_bytes(const Run& r);
uint64_t run_rows_bound(const Run& r, uint64_t n_memory_trace);
std::mutex& run_mutex(Run& r);
void run_open_memory(Run& r, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root);
void open_require_device(const char* who);
void open_check_addresses(const char* who, const uint32_t* addresses, uint64_t n, const cm_mem_opening* out);
void run_open_memory_range(Run& r, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out, uint32_t* root);
void open_range_check(const char* who, uint32_t start, uint32_t n_cells, const uint32_t* values, const cm_mem_range_opening* out);
void run_open_memory_set(Run& r, const uint32_t* addresses, uint32_t n, uint32_t* values, uint32_t* siblings, uint32_t n_siblings, uint32_t* root);
void open_set_check(const char* who, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings, uint32_t cap_siblings,
                    uint32_t* n_siblings);
cm_mem_transition* open_transition(const DeviceInput& d, const uint32_t* addresses, uint64_t n);

// ---- the host verifier (verifier.hip); the device verifier is verify_device.hpp ------------------------------------------------
std::string verify_proof(const ProofData& pf, const cm_pcs_config& expected);
bool proof_from_words(const uint32_t* w, uint64_t n, ProofData& p, std::string& err);

}  // namespace cm
