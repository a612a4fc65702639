// What the single-GPU prover (prover.hip) and the sharded one (prover_sharded.inc) know about a proof in the same way: the input,
// the proof being written, component sizes and launch orders, column offsets of trees 1 / 2, relations, constraint offsets and
// powers, the OODS point — and the transcript snippets both use.
// ProofContext holds host state only.  The members that own device resources or streams (Prover P, the twiddles and their fork,
// drel, d_powers) stay declared in each prover, between that prover's own buffers and guards: members die in reverse declaration
// order, that order is behaviour (pool blocks go back in it, guards drain in front of the buffers they protect), and the two
// provers interleave those members differently.
#pragma once
#include "segment_input.hpp"

namespace cm {
// the PcsConfig ranges both provers accept (max_log: the largest trace column)
static void check_pcs_config(const cm_pcs_config& cfg, uint32_t max_log) {
  CM_CHECK(cfg.n_queries >= 1 && cfg.n_queries <= 4096, "PcsConfig: n_queries must be in 1..4096");
  CM_CHECK(cfg.pow_bits <= 64, "PcsConfig: pow_bits must be at most 64");
  CM_CHECK(cfg.log_last_layer_degree_bound <= max_log, "PcsConfig: log_last_layer_degree_bound exceeds the largest trace column");
}
struct ProofContext {
  const DeviceInput& din;
  const cm_prover_input& in;
  const cm_pcs_config cfg;
  std::unique_ptr<ProofData> out;
  ProofData& pf;
  uint32_t clog[air::N_COMPONENTS];          // log2 rows of every component
  uint32_t max_log = 0, comp_log = 0;        // largest component; composition polynomial = max_log + 1
  std::vector<int> by_size_all;              // launch order of the fork regions: all components by descending size (stable)
  std::vector<size_t> tr0, it0;              // first column of every component in trees 1 / 2
  std::vector<uint32_t> tr_logs, it_logs;    // log size of every column of trees 1 / 2
  HostRelations hrel;
  std::vector<size_t> coff;                  // first constraint of every component
  std::vector<QM31> powers;                  // random-coefficient powers, one per constraint (sized by column_offsets)
  CPoint<QM31> oods;
  ProofContext(const DeviceInput& din_, const cm_pcs_config& cfg_) : din(din_), in(din_.meta), cfg(cfg_), out(new ProofData()), pf(*out) {
    pf.config = cfg;
    bind_thread_to_library_device();
  }
  // the prover's driver state on the calling thread's main stream; the first phase event
  void start(Prover& P) {
    if (g_transcript_log.load()) P.ch.log.p = &pf.transcript;
    P.cfg = cfg;
    P.st = thread_main_stream();
    P.start();
  }
  // component log sizes (known from the input lengths), the config checks, launch order
  void size_components() {
    component_logs(in, clog);
    max_log = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) { max_log = std::max(max_log, clog[c]); CM_CHECK(clog[c] <= 26, "component too large"); }
    check_pcs_config(cfg, max_log);
    comp_log = max_log + 1;
    for (int c = 0; c < air::N_COMPONENTS; c++) by_size_all.push_back(c);
    std::stable_sort(by_size_all.begin(), by_size_all.end(), [&](int x, int y) { return clog[x] > clog[y]; });
  }
  // where every component's columns start in trees 1 / 2 (Claim::write_trace order) and its constraints among all constraints
  void column_offsets() {
    tr0.assign(air::N_COMPONENTS, 0); it0.assign(air::N_COMPONENTS, 0); coff.assign(air::N_COMPONENTS, 0);
    size_t n_constraints = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      const air::ComponentInfo& info = air::component_info(c);
      tr0[c] = tr_logs.size(); it0[c] = it_logs.size(); coff[c] = n_constraints;
      tr_logs.insert(tr_logs.end(), info.n_trace, clog[c]);
      it_logs.insert(it_logs.end(), info.n_interaction, clog[c]);
      n_constraints += info.n_constraints;
    }
    powers.assign(n_constraints, QM31());
  }
  // behind decommit(): phase times, the flag-join check, the memory report, the step count
  void finish_common(Prover& P) {
    P.finish();
    fork_join_check();
    pf.phase_ms = P.phase_ms;
    P.report_memory(pf, device_input_bytes(din));
    pf.steps = 0;
    for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) pf.steps += in.n_bundles[i];
  }
};
// Claim::mix_into (prover.rs:77-82): the component log sizes
inline void mix_claim(Channel& ch, ProofData& pf, const uint32_t* clog) {
  for (int c = 0; c < air::N_COMPONENTS; c++) { pf.claim_log_sizes.push_back(clog[c]); ch.mix_u64(clog[c]); }
}
// the channel state as the device transcript steps take it: {digest[8], n_sent}
inline void channel_words(const Channel& ch, uint32_t cw[9]) {
  memcpy(cw, ch.digest.data(), 32);
  cw[8] = ch.n_sent;
}
// An exception between a fork and its join must not hand buffers back to the pool under the side stream's kernels: declared BEHIND
// the buffers it protects, the guard drains the stream first.
struct DrainOnExit { hipStream_t s = nullptr; bool joined = false; ~DrainOnExit() { if (s && !joined) (void)hipStreamSynchronize(s); } };
}  // namespace cm
