// C ABI of a whole run (include/cairom_hip.h, header revision 10): memory carried on the device, chained segment proofs, the
// openings under the image's root, and the PCS-free check of a run.  The run object is adapter_run.inc, the ingest loop prover.hip.
#include "../../include/cairom_hip.h"
#include "prover_api.hpp"
#include <memory>
#include <mutex>
#include <string.h>

extern "C" {
int32_t cm_run_begin(const uint32_t* initial_memory, uint64_t n_initial_memory, const uint32_t* initial_heap, uint64_t n_initial_heap,
                     const uint32_t ranges[6], cm_run** out) {
  return cm::abi_guard([&] {
    CM_CHECK(out, "cm_run_begin: null output");
    std::unique_ptr<cm_run> h(new cm_run());
    h->r = cm::run_begin(initial_memory, n_initial_memory, initial_heap, n_initial_heap, ranges);
    *out = h.release();
  });
}
int32_t cm_run_adapt_next(cm_run* r, const cm_run_segment* seg, cm_device_input** out) {
  return cm::abi_guard([&] {
    CM_CHECK(r && r->r && out, "cm_run_adapt_next: null argument");
    cm::check_run_segment(seg, "cm_run_adapt_next");
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    std::unique_ptr<cm_device_input> h(new cm_device_input());
    h->d = cm::run_adapt_next(*r->r, *seg);
    *out = h.release();
  });
}
int32_t cm_run_memory(const cm_run* r, uint32_t* locals, uint64_t cap_l, uint64_t* n_l, uint32_t* heap, uint64_t cap_h, uint64_t* n_h) {
  return cm::abi_guard([&] {
    CM_CHECK(r && r->r, "cm_run_memory: null run");
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    cm::run_memory(*r->r, locals, cap_l, n_l, heap, cap_h, n_h);
  });
}
// openings under the root of the image as it is now (mem_open.hip, adapter_run.inc); every refusal comes before the first write
int32_t cm_run_open_memory(cm_run* r, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_run_open_memory");
    CM_CHECK(r && r->r && root, "cm_run_open_memory: null argument");
    cm::open_check_addresses("cm_run_open_memory", addresses, n, out);
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    cm::run_open_memory(*r->r, addresses, n, out, root);
  });
}
// a range under the same root (mem_range.hip); every refusal comes before the first write
int32_t cm_run_open_memory_range(cm_run* r, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_run_open_memory_range");
    CM_CHECK(r && r->r && root, "cm_run_open_memory_range: null argument");
    cm::open_range_check("cm_run_open_memory_range", start, n_cells, values, out);
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    cm::run_open_memory_range(*r->r, start, n_cells, values, out, root);
  });
}
// a set of cells under the same root (mem_set.hip); every refusal comes before the first write to values or siblings
int32_t cm_run_open_memory_set(cm_run* r, const uint32_t* addresses, uint64_t n, uint32_t* values, uint32_t* siblings, uint32_t cap_siblings,
                               uint32_t* n_siblings, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_run_open_memory_set");
    CM_CHECK(r && r->r && root, "cm_run_open_memory_set: null argument");
    cm::open_set_check("cm_run_open_memory_set", addresses, n, values, siblings, cap_siblings, n_siblings);
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    cm::run_open_memory_set(*r->r, addresses, (uint32_t)n, values, siblings, *n_siblings, root);
  });
}
int32_t cm_run_free(cm_run* r) { delete r; return 0; }
int32_t cm_prove_run(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs) {
  return cm::abi_guard([&] {
    CM_CHECK(r && r->r && (!n || (segs && outs)), "cm_prove_run: null argument");
    cm::prove_run("cm_prove_run", *r->r, segs, n, config, inflight, outs, nullptr);
  });
}
// the same with every adapted segment's write-set transition (mem_transition.hip) opened before a worker takes the input
int32_t cm_prove_run_transitions(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                                 cm_proof** outs, cm_mem_transition** transitions) {
  return cm::abi_guard([&] {
    CM_CHECK(r && r->r && (!n || (segs && outs && transitions)), "cm_prove_run_transitions: null argument");
    for (uint32_t i = 0; i < n; i++) transitions[i] = nullptr;
    cm::prove_run("cm_prove_run_transitions", *r->r, segs, n, config, inflight, outs, transitions);
  });
}
// The same walk with the PCS-free check (check.hip) and the link diff (link.hip) in the place of the proof: every verdict is
// collected, only a segment that cannot be adapted ends the call.  Segment i - 1's input lives until link i has been looked at.
int32_t cm_check_run(cm_run* r, const cm_run_segment* const* segs, uint32_t n, const cm_relations* relations, cm_run_check* out,
                     cm_link_cell* cells, uint64_t cap_per_link) {
  return cm::abi_guard([&] {
    CM_CHECK(r && r->r && (!n || (segs && out)), "cm_check_run: null argument");
    CM_CHECK(cells || cap_per_link == 0, "cm_check_run: null cells with a capacity");
    std::lock_guard<std::mutex> lk(cm::run_mutex(*r->r));
    if (n) memset(out, 0, (size_t)n * sizeof(cm_run_check));
    std::unique_ptr<cm::DeviceInput> prev;
    for (uint32_t i = 0; i < n; i++) {
      cm::check_run_segment(segs[i], "cm_check_run");
      std::unique_ptr<cm::DeviceInput> cur(cm::run_adapt_next(*r->r, *segs[i]));
      cm::check_segment(*cur, relations, out[i].check);
      if (prev) cm::check_link_into(*prev, *cur, i, out[i], cells, cap_per_link);
      prev = std::move(cur);
    }
    cm_set_last_error(cm::run_check_summary(out, n, true).c_str());
  });
}
}  // extern "C"
