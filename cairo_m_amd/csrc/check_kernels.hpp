// Host-visible declarations of the PCS-free AIR check kernels (kernels_check.inc; driver: check.hip).
#pragma once
#include "engine.hpp"

namespace cm {

struct DevRelations;

// One component's trace-domain check: every constraint of every row tested for zero.
struct CheckArgs {
  const uint32_t* const* tr;       // tree-1 trace-domain columns of the component (device array)
  const uint32_t* const* it;       // tree-2 trace-domain columns
  const uint32_t* const* pp;       // preprocessed trace-domain columns by PreprocId
  const DevRelations* rels;
  const uint32_t* claimed_sum;     // 4 words on the device (cumsum shift = claimed_sum / 2^log_size)
  uint32_t* row_status;            // optional (null): lowest failing constraint of every row, 0xFFFFFFFF = none
  unsigned long long* failing_rows;   // += rows with a failing constraint (one atomic per wave that saw one)
  unsigned long long* first;          // atomicMin of (row << 16) | constraint; the caller sets it to ~0
  uint32_t log_size;
  int n_base;
};
// One component's relation sums: sums[r * 4 + k] += coordinate k of sum_rows sum_{entries of r} mult / combine_r(values), as
// 64-bit sums of canonical words (one atomic per block and word); the caller zeroes them and reduces modulo P.
struct RelSumArgs {
  const uint32_t* const* tr;
  const uint32_t* const* pp;
  const DevRelations* rels;
  unsigned long long* sums;        // [N_RELATIONS][4]
  uint32_t log_size;
};
constexpr uint32_t CHECK_KEY_NONE = 0xffffffffu;

void launch_check(int cid, const CheckArgs& a, hipStream_t st);
void launch_relsum(int cid, const RelSumArgs& a, hipStream_t st);
// every component of at most SMALL_COMPONENT_MAX_LOG (256) rows in one launch each (blockIdx.y = job)
void launch_check_small(const CheckArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st);
void launch_relsum_small(const RelSumArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st);
// After the lookup histograms flagged an out-of-range value: *key = min over the opcode component's rows of
// (cid << 40) | (row << 8) | table of the row's first out-of-range entry (table 0 rc8, 1 rc16, 2 rc20, 3 bitwise).
void launch_lookup_diag(int cid, const uint32_t* const* d_cols, uint32_t log_size, unsigned long long* key, hipStream_t st);

}  // namespace cm
