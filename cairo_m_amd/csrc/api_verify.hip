// C ABI of the verifiers (include/cairom_hip.h): verify_cairo_m in host code (verifier.hip), the batched device verifier
// (verify_device.hip) and a run's continuity on top of either.  0 = accepted; status 11 + cm_last_error() = the failed check.
#include "../../include/cairom_hip.h"
#include "prover_api.hpp"
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

namespace {
// each segment starts where its predecessor stopped (crates/prover/tests/prover.rs:198-243; the registers are the execution
// boundary of public_data.rs:192-227)
void check_run_continuity(const cm_proof* const* proofs, uint32_t n) {
  for (uint32_t i = 1; i < n; i++) {
    const cm::PublicData &a = proofs[i - 1]->d->public_data, &b = proofs[i]->d->public_data;
    const char* field = b.initial_pc != a.final_pc ? "pc" : b.initial_fp != a.final_fp ? "fp" : b.initial_root != a.final_root ? "root" : nullptr;
    if (field)
      throw cm::CmError(11, "run: segment " + std::to_string(i) + " initial_" + field + " != segment " + std::to_string(i - 1) + " final_" + field);
  }
}
// The verdicts of the GPU for a whole batch (verify_device.hip): out[i] = what cm_verify_proof says about proofs[i]
void verify_many_impl(const char* who, const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, std::vector<cm::VerifyOutcome>& out,
                      cm_stream_t s, std::vector<std::vector<cm::VerifySlotDetail>>* detail = nullptr, uint32_t flags = 0) {
  CM_CHECK((flags & ~CM_VERIFY_ARITH_ON_DEVICE) == 0, std::string(who) + ": unknown flag bit");
  CM_CHECK(n >= 1 && proofs, std::string(who) + ": no proofs");
  std::vector<const cm::ProofData*> pd(n);
  for (uint32_t i = 0; i < n; i++) {
    CM_CHECK(proofs[i] && proofs[i]->d, std::string(who) + ": null proof");
    pd[i] = proofs[i]->d;
  }
  cm::verify_many_device(pd.data(), n, expected ? *expected : cm::default_cfg(), out, cm::as_stream(s), detail, flags);
}
// the verdicts of a batch as cm_verify_many reports them: results, and the first rejected proof as the call's error
void verify_many_report(const std::vector<cm::VerifyOutcome>& out, uint32_t n, cm_verify_result* results) {
  uint32_t first = n;
  for (uint32_t i = 0; i < n; i++) {
    const bool ok = out[i].message.empty();
    if (!ok && first == n) first = i;
    if (!results) continue;
    memset(&results[i], 0, sizeof(cm_verify_result));
    if (ok) continue;
    results[i].status = 11;
    results[i].check = out[i].check;
    snprintf(results[i].message, sizeof(results[i].message), "verification failed: %s", out[i].message.c_str());
  }
  if (first < n) throw cm::CmError(11, "proof " + std::to_string(first) + ": verification failed: " + out[first].message);
}
}  // namespace

extern "C" {
int32_t cm_verify_proof(const cm_proof* p, const cm_pcs_config* expected) {
  return cm::abi_guard([&] {
    std::string e = cm::verify_proof(*p->d, expected ? *expected : cm::default_cfg());
    if (!e.empty()) throw cm::CmError(11, "verification failed: " + e);
  });
}
int32_t cm_verify_proof_words(const uint32_t* words, uint64_t n_words, const cm_pcs_config* expected) {
  return cm::abi_guard([&] {
    cm::ProofData pd;
    std::string e;
    if (!cm::proof_from_words(words, n_words, pd, e)) throw cm::CmError(11, "verification failed: " + e);
    e = cm::verify_proof(pd, expected ? *expected : cm::default_cfg());
    if (!e.empty()) throw cm::CmError(11, "verification failed: " + e);
  });
}
// host code: every proof verifies, and the run is continuous
int32_t cm_verify_run(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected) {
  return cm::abi_guard([&] {
    CM_CHECK(n >= 1 && proofs, "cm_verify_run: no proofs");
    for (uint32_t i = 0; i < n; i++) {
      CM_CHECK(proofs[i] && proofs[i]->d, "cm_verify_run: null proof");
      const std::string e = cm::verify_proof(*proofs[i]->d, expected ? *expected : cm::default_cfg());
      if (!e.empty()) throw cm::CmError(11, "run: segment " + std::to_string(i) + ": verification failed: " + e);
    }
    check_run_continuity(proofs, n);
  });
}
int32_t cm_verify_many_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags, cm_verify_result* results,
                          cm_stream_t s) {
  return cm::abi_guard([&] {
    std::vector<cm::VerifyOutcome> out;
    verify_many_impl("cm_verify_many", proofs, n, expected, out, s, nullptr, flags);
    verify_many_report(out, n, results);
  });
}
int32_t cm_verify_many(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_result* results, cm_stream_t s) {
  return cm_verify_many_ex(proofs, n, expected, 0, results, s);
}
int32_t cm_verify_many_detail(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_result* results,
                              cm_verify_slot* slots, uint32_t cap_slots, uint32_t* slot_first, cm_stream_t s) {
  return cm_verify_many_detail_ex(proofs, n, expected, 0, results, slots, cap_slots, slot_first, s);
}
int32_t cm_verify_many_detail_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags, cm_verify_result* results,
                                 cm_verify_slot* slots, uint32_t cap_slots, uint32_t* slot_first, cm_stream_t s) {
  return cm::abi_guard([&] {
    CM_CHECK(slot_first && (slots || !cap_slots), "cm_verify_many_detail: null output");
    std::vector<cm::VerifyOutcome> out;
    std::vector<std::vector<cm::VerifySlotDetail>> detail;
    verify_many_impl("cm_verify_many_detail", proofs, n, expected, out, s, &detail, flags);
    slot_first[0] = 0;
    for (uint32_t i = 0; i < n; i++) slot_first[i + 1] = slot_first[i] + (uint32_t)detail[i].size();
    CM_CHECK(slot_first[n] <= cap_slots, "cm_verify_many_detail: the slot array is too small (the count is in slot_first[n])");
    for (uint32_t i = 0; i < n; i++)
      for (size_t k = 0; k < detail[i].size(); k++) {
        cm_verify_slot& o = slots[slot_first[i] + k];
        memset(&o, 0, sizeof(o));
        o.check = detail[i][k].check;
        o.on_device = detail[i][k].on_device ? 1u : 0u;
        o.raised = detail[i][k].raised ? 1u : 0u;
        snprintf(o.message, sizeof(o.message), "%s", detail[i][k].message.c_str());
      }
    verify_many_report(out, n, results);
  });
}
int32_t cm_verify_plan_stats(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, cm_verify_stats* out) {
  return cm::abi_guard([&] {
    CM_CHECK(n >= 1 && proofs && out, "cm_verify_plan_stats: no proofs, or null output");
    std::vector<const cm::ProofData*> pd(n);
    for (uint32_t i = 0; i < n; i++) {
      CM_CHECK(proofs[i] && proofs[i]->d, "cm_verify_plan_stats: null proof");
      CM_CHECK(out[i].struct_size >= sizeof(cm_verify_stats), "cm_verify_plan_stats: struct_size does not cover cm_verify_stats (set it to sizeof(cm_verify_stats))");
      pd[i] = proofs[i]->d;
    }
    std::vector<cm_verify_stats> st(n);
    cm::verify_plan_stats(pd.data(), n, expected ? *expected : cm::default_cfg(), st.data());
    for (uint32_t i = 0; i < n; i++) { const uint32_t keep = out[i].struct_size; out[i] = st[i]; out[i].struct_size = keep; }
  });
}
int32_t cm_verify_run_device(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected) {
  return cm_verify_run_device_ex(proofs, n, expected, 0);
}
// the same verdicts from the GPU, then the run's continuity
int32_t cm_verify_run_device_ex(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, uint32_t flags) {
  return cm::abi_guard([&] {
    std::vector<cm::VerifyOutcome> out;
    verify_many_impl("cm_verify_run_device", proofs, n, expected, out, 0, nullptr, flags);
    for (uint32_t i = 0; i < n; i++)
      if (!out[i].message.empty()) throw cm::CmError(11, "run: segment " + std::to_string(i) + ": verification failed: " + out[i].message);
    check_run_continuity(proofs, n);
  });
}
int32_t cm_verify_many_timing(double ms[4]) {
  return cm::abi_guard([&] { CM_CHECK(ms, "cm_verify_many_timing: null output"); cm::verify_many_timing(ms); });
}
}  // extern "C"
