// C ABI of the prover (include/cairom_hip.h): device inputs, one proof, the sharded plan and proof, the pipelines of
// cm_prove_many*, the memory estimate and the process-wide switches of the prover.  Argument checks, handle translation and result
// marshalling only: the provers and the pipelines' scheduling are prover.hip.
#include "../../include/cairom_hip.h"
#include "prover_api.hpp"
#include "tail_plan.hpp"
#include <algorithm>
#include <memory>
#include <string>

namespace {
void estimate_checked(const uint32_t* clog, const cm_pcs_config* config, uint32_t world, uint64_t input_bytes, cm_mem_estimate* out, const char* who) {
  const std::string w(who);
  CM_CHECK(clog && out, (w + ": null argument").c_str());
  CM_CHECK(out->struct_size >= sizeof(cm_mem_estimate), (w + ": struct_size does not cover cm_mem_estimate (set it to sizeof(cm_mem_estimate))").c_str());
  const cm_pcs_config cfg = config ? *config : cm::default_cfg();
  CM_CHECK(cfg.log_blowup_factor >= 1 && cfg.log_blowup_factor <= 4, (w + ": log_blowup_factor must be in 1..4").c_str());
  CM_CHECK(world == 1 || world == 2 || world == 4 || world == 8, (w + ": world must be 1, 2, 4 or 8").c_str());
  CM_CHECK(cfg.n_queries <= 4096, (w + ": n_queries must be at most 4096").c_str());
  for (int c = 0; c < air::N_COMPONENTS; c++) CM_CHECK(clog[c] <= 26, (w + ": a component's log size exceeds 26").c_str());
  cm_mem_estimate e;
  memset(&e, 0, sizeof(e));
  e.struct_size = sizeof(e);
  cm::estimate_memory(clog, cfg, world, cm::mem_switches(), e);
  e.input_bytes = input_bytes;
  memcpy(out, &e, sizeof(e));
}
}  // namespace

extern "C" {
int32_t cm_input_upload(const cm_prover_input* input, cm_device_input** out) {
  return cm::abi_guard([&] { std::unique_ptr<cm_device_input> h(new cm_device_input()); h->d = cm::upload_input(*input); *out = h.release(); });
}
int32_t cm_adapt_segment_device(const cm_runner_segment* seg, cm_device_input** out) {
  return cm::abi_guard([&] { std::unique_ptr<cm_device_input> h(new cm_device_input()); h->d = cm::adapt_segment_device(*seg); *out = h.release(); });
}
int32_t cm_device_input_download(const cm_device_input* in, cm_host_input** out) {
  return cm::abi_guard([&] {
    cm_host_input* h = new cm_host_input();
    cm::download_input(*in->d, h->owned);
    h->view = h->owned.view();
    *out = h;
  });
}
int32_t cm_input_free(cm_device_input* h) { delete h; return 0; }
int32_t cm_prove_device(const cm_device_input* input, const cm_pcs_config* config, cm_proof** out) {
  return cm::abi_guard([&] {
    cm_pcs_config cfg = config ? *config : cm::default_cfg();
    std::unique_ptr<cm_proof> p(new cm_proof());
    p->d = cm::prove(*input->d, cfg);
    *out = p.release();
  });
}
int32_t cm_prove_segment(const cm_prover_input* input, const cm_pcs_config* config, cm_proof** out) {
  cm_device_input* di = nullptr;
  int32_t rc = cm_input_upload(input, &di);
  if (rc) return rc;
  rc = cm_prove_device(di, config, out);
  cm_input_free(di);
  return rc;
}
int32_t cm_shard_plan(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, int32_t owner_out[CM_N_COMPONENTS],
                      uint64_t* staging_words) {
  return cm::abi_guard([&] {
    CM_CHECK(world >= 1 && world <= 8 && (world & (world - 1)) == 0, "cm_shard_plan: world must be 1, 2, 4 or 8");
    const cm_pcs_config cfg = config ? *config : cm::default_cfg();
    CM_CHECK(cfg.log_blowup_factor >= 1 && cfg.log_blowup_factor <= 4, "cm_shard_plan: log_blowup_factor");
    uint32_t clog[air::N_COMPONENTS];
    cm::component_logs(*input, clog);
    // the SAME plan cm_prove_sharded will run under this config (components are split only at log_blowup_factor 1)
    const cm::ShardPlan p = cm::make_shard_plan(clog, world, cfg.log_blowup_factor == 1);
    for (int c = 0; c < air::N_COMPONENTS; c++) if (owner_out) owner_out[c] = p.owner[c];
    // (the bound is computed for a blowup of 2; the LDE, and with it every exchange, grows by 2^(B - 1))
    if (staging_words) *staging_words = cm::shard_staging_words(clog, p, world) << (cfg.log_blowup_factor - 1);
  });
}
int32_t cm_shard_plan_columns(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, int32_t* trace_col_owner,
                              uint32_t* n_trace_cols, int32_t* interaction_col_owner, uint32_t* n_interaction_cols, uint64_t load_cells[8]) {
  return cm::abi_guard([&] {
    CM_CHECK(world >= 1 && world <= 8 && (world & (world - 1)) == 0, "cm_shard_plan_columns: world must be 1, 2, 4 or 8");
    const cm_pcs_config cfg = config ? *config : cm::default_cfg();
    uint32_t clog[air::N_COMPONENTS];
    cm::component_logs(*input, clog);
    const cm::ShardPlan p = cm::make_shard_plan(clog, world, cfg.log_blowup_factor == 1);
    // n_*_cols: capacity of the array on entry, the number of columns on return; an array that is too small is an error, never
    // an overrun
    if (trace_col_owner) {
      CM_CHECK(n_trace_cols && *n_trace_cols >= p.tr_owner.size(), "cm_shard_plan_columns: trace_col_owner is too small (set *n_trace_cols to its capacity)");
      for (size_t j = 0; j < p.tr_owner.size(); j++) trace_col_owner[j] = p.tr_owner[j];
    }
    if (interaction_col_owner) {
      CM_CHECK(n_interaction_cols && *n_interaction_cols >= p.it_owner.size(),
               "cm_shard_plan_columns: interaction_col_owner is too small (set *n_interaction_cols to its capacity)");
      for (size_t j = 0; j < p.it_owner.size(); j++) interaction_col_owner[j] = p.it_owner[j];
    }
    if (n_trace_cols) *n_trace_cols = (uint32_t)p.tr_owner.size();
    if (n_interaction_cols) *n_interaction_cols = (uint32_t)p.it_owner.size();
    if (load_cells) for (int k = 0; k < 8; k++) load_cells[k] = p.load[k];
  });
}
int32_t cm_prove_sharded(const cm_device_input* input, const cm_pcs_config* config, const cm_comm* comm, cm_proof** out) {
  return cm::abi_guard([&] {
    // the caller's struct may be older / shorter than this library's: copy what its struct_size covers, the rest stays zero
    CM_CHECK(comm && comm->struct_size >= offsetof(cm_comm, flags) && comm->struct_size <= 4096,
             "cm_prove_sharded: cm_comm.struct_size does not cover the required fields (set it to sizeof(cm_comm))");
    cm_comm cc;
    memset(&cc, 0, sizeof(cc));
    memcpy(&cc, comm, std::min<size_t>(comm->struct_size, sizeof(cm_comm)));
    CM_CHECK(cc.all_gather && cc.all_to_all_v && cc.send_buf && cc.recv_buf, "cm_prove_sharded: incomplete cm_comm");
    cm_pcs_config cfg = config ? *config : cm::default_cfg();
    std::unique_ptr<cm_proof> p(new cm_proof());
    try {
      p->d = cm::prove_sharded(*input->d, cfg, cc);
    } catch (...) {
      if (cc.abort) cc.abort(cc.ctx);   // the peers are heading for a collective this rank will never join
      throw;
    }
    *out = p.release();
  });
}
int32_t cm_prove_many(const cm_device_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                      cm_proof** outs) {
  return cm::abi_guard([&] { cm::prove_many(inputs, n, config, inflight, outs); });
}
// streaming ingest: the calling thread uploads (or adapts) item i + 1 while the workers prove the items before it (prover.hip)
int32_t cm_prove_many_host(const cm_prover_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs) {
  return cm::abi_guard([&] { cm::prove_many_host(inputs, n, config, inflight, outs); });
}
int32_t cm_prove_many_segments(const cm_runner_segment* const* segments, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                               cm_proof** outs) {
  return cm::abi_guard([&] { cm::prove_many_segments(segments, n, config, inflight, outs); });
}
int32_t cm_estimate_memory_logs(const uint32_t log_size[CM_N_COMPONENTS], const cm_pcs_config* config, uint32_t world, cm_mem_estimate* out) {
  return cm::abi_guard([&] { estimate_checked(log_size, config, world, 0, out, "cm_estimate_memory_logs"); });
}
int32_t cm_estimate_memory(const cm_prover_input* input, const cm_pcs_config* config, uint32_t world, cm_mem_estimate* out) {
  return cm::abi_guard([&] {
    CM_CHECK(input && out, "cm_estimate_memory: null argument");
    uint32_t clog[air::N_COMPONENTS];
    cm::component_logs(*input, clog);
    estimate_checked(clog, config, world, cm::estimate_input_bytes(*input), out, "cm_estimate_memory");
  });
}
int32_t cm_set_transcript_log(int32_t on) { cm::g_transcript_log.store(on ? 1 : 0); return 0; }
int32_t cm_set_preprocessed_cache(int32_t on) {
  cm::g_pp_cache.store(on ? 1 : 0, std::memory_order_relaxed);
  return 0;
}
int32_t cm_set_tuning(const char* key, int32_t value) {
  if (!key) return cm_set_last_error("cm_set_tuning: null key");
  for (int k = 0; k < cm::T_COUNT; k++)
    if (strcmp(cm::TUNE_TABLE[k].key, key) == 0) {
      if (value < cm::TUNE_TABLE[k].lo || value > cm::TUNE_TABLE[k].hi) return cm_set_last_error("cm_set_tuning: value out of the key's range");
      cm::tune_values()[k].store(value);
      return 0;
    }
  return cm_set_last_error("cm_set_tuning: unknown key");
}
int32_t cm_set_device_tail(int32_t on) {
  cm::g_device_tail.store(on ? 1 : 0);
  return 0;
}
int32_t cm_set_twiddle_cache(int32_t on) {
  cm::g_tw_cache.store(on ? 1 : 0, std::memory_order_relaxed);
  return 0;
}
int32_t cm_kprof_enable(int32_t on) {
  return cm::abi_guard([&] {
    cm::KProf::get().reset();
    cm::KProf::get().on = on != 0;
    cm::KProf::get().only.clear();
  });
}
// time only one kernel class (name as reported by cm_kprof_report); NULL / "" = all classes
int32_t cm_kprof_filter(const char* name) {
  return cm::abi_guard([&] { cm::KProf::get().only = name ? name : ""; });
}
// JSON: {"kernel": {"calls": n, "ms": total, "bytes": algorithmic bytes}, ...}; returns its length, or -1 with cm_last_error()
int32_t cm_kprof_report(char* buf, size_t buf_len) {
  int32_t len = -1;
  cm::abi_guard([&] {
    (void)hipDeviceSynchronize();
    cm::KProf& k = cm::KProf::get();
    k.flush();
    std::string s = "{";
    bool first = true;
    for (auto& kv : k.agg) {
      if (!first) s += ",";
      first = false;
      s += "\"" + kv.first + "\":{\"calls\":" + std::to_string(kv.second.calls) + ",\"ms\":" + std::to_string(kv.second.ms) +
           ",\"bytes\":" + std::to_string(kv.second.bytes) + ",\"work\":" + std::to_string(kv.second.work) + "}";
    }
    s += "}";
    if (buf && buf_len) { size_t n = s.size() < buf_len - 1 ? s.size() : buf_len - 1; memcpy(buf, s.data(), n); buf[n] = 0; }
    len = (int32_t)s.size();
  });
  return len;
}
}  // extern "C"
