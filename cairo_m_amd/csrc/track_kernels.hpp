// Host-visible declarations of the relation tracker's kernels (kernels_track.inc; driver: track.hip).
#pragma once
#include "engine.hpp"

namespace cm {

struct DevRelations;

// One record per (entry ordinal, row) of the selected relation, entry-major: slot = base + ordinal * 2^log_size + row.
//   key_hi / key_lo : the entry's LogUp denominator sum_i alpha^i v_i - z as (w0 << 32 | w1), (w2 << 32 | w3), canonical words
//   mult            : canonical multiplicity;  loc : TRACK_LOC(component, row, ordinal)
// An entry whose multiplicity is zero gets the sentinel key (TRACK_KEY_NONE in both halves: P is no canonical word), mult 0.
struct TrackRecords {
  unsigned long long* key_hi;
  unsigned long long* key_lo;
  unsigned long long* loc;
  uint32_t* mult;
};
constexpr unsigned long long TRACK_KEY_NONE = 0x7fffffff7fffffffull;
constexpr unsigned long long TRACK_LOC(unsigned long long cid, unsigned long long row, unsigned long long ord) {
  return (cid << 56) | (row << 24) | ord;
}
constexpr uint32_t TRACK_ORD_BITS = 24;

struct TrackEmitArgs {
  const uint32_t* const* tr;     // trace-domain columns of the component
  const uint32_t* const* pp;     // preprocessed trace-domain columns by PreprocId
  const DevRelations* rels;
  TrackRecords rec;
  unsigned long long base;       // first slot of the component
  uint32_t log_size;
  int relation;                  // the selected relation
  int cid;                       // component id (for the locator)
};
// One survivor: re-evaluate row `row` of component `cid` and capture entry `ordinal` of relation `relation`:
// out[17 * i] = number of values, out[17 * i + 1 ..] = the values
struct TrackRecoverJob {
  const uint32_t* const* tr;
  int cid, relation;
  uint32_t row, ordinal;
};
constexpr int TRACK_RECOVER_WORDS = 17;

void launch_track_emit(int cid, const TrackEmitArgs& a, hipStream_t st);
// every component of at most SMALL_COMPONENT_MAX_LOG (256) rows in one launch (blockIdx.y = job)
void launch_track_emit_small(const TrackEmitArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st);
void launch_track_recover(const TrackRecoverJob* d_jobs, uint32_t n_jobs, const uint32_t* const* d_pp, uint32_t* d_out, hipStream_t st);

}  // namespace cm
