// C ABI of the proof object (include/cairom_hip.h): its words, JSON and transcript, public data and entries, statistics and
// memory record.  Host code only.
#include "../../include/cairom_hip.h"
#include "abi.hpp"
#include "handles.hpp"
#include <algorithm>
#include <memory>
#include <string.h>

namespace cm {
bool proof_from_words(const uint32_t* w, uint64_t n, ProofData& p, std::string& err);   // verifier.hip
}  // namespace cm

namespace {
void public_entries_out(const cm::PublicData& d, uint32_t which, uint32_t* out, uint64_t cap_entries, uint64_t* n_entries, const char* too_small) {
  const std::vector<cm::PublicEntry>& v = which == 0 ? d.program : which == 1 ? d.input : d.output;
  *n_entries = v.size();
  if (!out) return;
  CM_CHECK(cap_entries >= v.size(), too_small);
  static_assert(sizeof(cm::PublicEntry) == 28, "seven words per public entry");
  if (!v.empty()) memcpy(out, v.data(), v.size() * sizeof(cm::PublicEntry));
}
}  // namespace

extern "C" {
int32_t cm_proof_public_data(const cm_proof* p, cm_public_data* out) {
  return cm::abi_guard([&] {
    CM_CHECK(p && p->d && out, "cm_proof_public_data: null argument");
    CM_CHECK(out->struct_size >= sizeof(cm_public_data), "cm_proof_public_data: struct_size does not cover cm_public_data (set it to sizeof(cm_public_data))");
    const cm::PublicData& d = p->d->public_data;
    cm_public_data o;
    memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.initial_pc = d.initial_pc; o.initial_fp = d.initial_fp; o.final_pc = d.final_pc; o.final_fp = d.final_fp; o.clock = d.clock;
    o.initial_root = d.initial_root; o.final_root = d.final_root;
    o.n_program = (uint32_t)d.program.size(); o.n_input = (uint32_t)d.input.size(); o.n_output = (uint32_t)d.output.size();
    memcpy(out, &o, sizeof(o));
  });
}
int32_t cm_proof_public_entries(const cm_proof* p, uint32_t which, uint32_t* out, uint64_t cap_entries, uint64_t* n_entries) {
  return cm::abi_guard([&] {
    CM_CHECK(p && p->d && n_entries && which <= 2, "cm_proof_public_entries: null argument, or `which` is not 0 (program), 1 (input) or 2 (output)");
    public_entries_out(p->d->public_data, which, out, cap_entries, n_entries, "cm_proof_public_entries: the output array is too small (the count is reported)");
  });
}
// the public data a device input already holds (host memory: no GPU work)
int32_t cm_device_input_public_entries(const cm_device_input* in, uint32_t which, uint32_t* out, uint64_t cap_entries, uint64_t* n_entries) {
  return cm::abi_guard([&] {
    CM_CHECK(in && in->d && n_entries && which <= 2, "cm_device_input_public_entries: null argument, or `which` is not 0 (program), 1 (input) or 2 (output)");
    public_entries_out(in->d->public_data, which, out, cap_entries, n_entries, "cm_device_input_public_entries: the output array is too small (the count is reported)");
  });
}
// proof object from its flat word stream (cm_proof_words format): host code, no GPU needed — lets a verifier-side process
// re-serialise a received proof (cm_proof_json) or hand it to cm_verify_proof
int32_t cm_proof_from_words(const uint32_t* words, uint64_t n_words, cm_proof** out) {
  return cm::abi_guard([&] {
    std::unique_ptr<cm_proof> p(new cm_proof());
    p->d = new cm::ProofData();
    std::string e;
    if (!cm::proof_from_words(words, n_words, *p->d, e)) throw cm::CmError(11, "cm_proof_from_words: " + e);
    *out = p.release();
  });
}
int32_t cm_proof_free(cm_proof* p) { delete p; return 0; }
int32_t cm_proof_json(const cm_proof* p, const char** json_out, size_t* len_out) {
  return cm::abi_guard([&] {
    cm_proof* q = const_cast<cm_proof*>(p);
    if (q->json.empty()) q->json = cm::proof_to_json(*p->d);
    *json_out = q->json.c_str();
    *len_out = q->json.size();
  });
}
int32_t cm_proof_transcript(const cm_proof* p, const char** json_out, size_t* len_out) {
  return cm::abi_guard([&] {
    cm_proof* q = const_cast<cm_proof*>(p);
    if (q->transcript_json.empty()) q->transcript_json = cm::transcript_to_json(p->d->transcript);
    *json_out = q->transcript_json.c_str();
    *len_out = q->transcript_json.size();
  });
}
int32_t cm_proof_words(const cm_proof* p, const uint32_t** words_out, uint64_t* n_out) {
  return cm::abi_guard([&] {
    cm_proof* q = const_cast<cm_proof*>(p);
    if (q->words.empty()) q->words = cm::proof_to_words(*p->d);
    *words_out = q->words.data();
    *n_out = q->words.size();
  });
}
int32_t cm_proof_commitments(const cm_proof* p, uint8_t roots[4][32]) {
  for (int t = 0; t < 4; t++) memcpy(roots[t], p->d->commitments[t].data(), 32);
  return 0;
}
int32_t cm_proof_memory(const cm_proof* p, cm_proof_mem* out) {
  return cm::abi_guard([&] {
    CM_CHECK(p && p->d && out, "cm_proof_memory: null argument");
    CM_CHECK(out->struct_size >= sizeof(cm_proof_mem), "cm_proof_memory: struct_size does not cover cm_proof_mem (set it to sizeof(cm_proof_mem))");
    cm_proof_mem m;
    memset(&m, 0, sizeof(m));
    m.struct_size = sizeof(m);
    const cm::ProofData& d = *p->d;
    m.n_phases = (uint32_t)std::min<size_t>(d.phase_peak_live.size(), 32);
    m.start_live_bytes = d.mem_start_live; m.peak_live_bytes = d.mem_peak_live; m.peak_reserved_bytes = d.mem_peak_reserved;
    m.input_bytes = d.mem_input_bytes; m.driver_allocs = d.mem_driver_allocs;
    for (uint32_t k = 0; k < m.n_phases; k++) m.phase_peak_live_bytes[k] = d.phase_peak_live[k];
    memcpy(out, &m, sizeof(m));
  });
}
int32_t cm_proof_stats(const cm_proof* p, uint64_t* cells, uint64_t* steps, double* phase_ms, uint32_t n_phases) {
  if (cells) *cells = p->d->cells;
  if (steps) *steps = p->d->steps;
  for (uint32_t i = 0; i < n_phases; i++) phase_ms[i] = i < p->d->phase_ms.size() ? p->d->phase_ms[i] : 0.0;
  return (int32_t)p->d->phase_ms.size();
}
}  // extern "C"
