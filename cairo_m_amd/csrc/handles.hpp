// The opaque handle structs of include/cairom_hip.h, each defined once.  (cm_mem_image stays in mem_image.hip: it is built from
// that file's own constants and nothing outside it looks inside; cm_rccl_comm likewise in comm_rccl.hip.)
#pragma once
#include "../../include/cairom_hip.h"
#include "host_adapter.hpp"
#include "proof.hpp"
#include "segment_input.hpp"
#include <string>
#include <vector>

namespace cm {
struct Run;             // adapter_run.inc
void run_free(Run* r);
}  // namespace cm

struct cm_host_input {
  cm::host::ProverInputOwned owned;
  cm_prover_input view;
};
struct cm_host_segment {
  cm::host::Segment seg;
  std::vector<uint32_t> trace, mem, init, heap;
  cm_runner_segment view;
};
struct cm_device_input { cm::DeviceInput* d = nullptr; ~cm_device_input() { delete d; } };
struct cm_proof {   // owns its ProofData: every failure path (parse error, exception mid-proof) releases it with the wrapper
  cm::ProofData* d = nullptr; std::string json, transcript_json; std::vector<uint32_t> words;
  ~cm_proof() { delete d; }
};
struct cm_run { cm::Run* r = nullptr; ~cm_run() { cm::run_free(r); } };
// what cm_input_open_transition hands out; cm_mem_transition_get points into the vectors
struct cm_mem_transition {
  std::vector<uint32_t> addresses, old_values, new_values, siblings;
  uint32_t root_before = 0, root_after = 0, n_zero_only = 0;
};
