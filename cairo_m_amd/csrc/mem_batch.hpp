// Batched set folds (mem_batch.hip: cm_verify_memory_transitions, cm_verify_memory_sets, cm_mem_batch_plan): many records, each a
// set of its own (mem_set.hpp), folded by ONE ladder of launches.  What the batch shares with the composition of transitions
// (mem_compose.hip) and the host plan both the launch path and cm_mem_batch_plan run.
//
// Layout.  The parts that pass the host checks are concatenated: cells, values (one or two planes) and sibling words, part after
// part.  lvl[k * (B + 1) + b], k = 0 .. 28, is the number of nodes of S_k in the parts before b (lvl[0 ..] = the cells' prefix
// `off`), woff[b] the number of words before part b.  The flags and their scan run over the 28 N pairs part-major: pair t of part
// p lies in [28 off[p], 28 off[p + 1]), depth-major inside that slice, as mem_compose.hip lays them out.  A node buffer keeps part
// p's level at off[p] + (rank inside the part) at every depth: |S_k| never exceeds the part's cells.
#pragma once
#include "mem_set.hpp"
#include <vector>

namespace cm {

constexpr uint32_t BATCH_MAX_PARTS = 1u << 16;
// the four device words of a part: the malformed flag of its hashing lanes, the verdict, the computed root of either plane
enum : uint32_t { BATCH_FLAG = 0, BATCH_VERDICT = 1, BATCH_ROOT = 2, BATCH_WORDS = 4 };

static_assert(sizeof(cm_mem_batch_step) == 16, "plain words, size as the header states it");

// the last part p with off[p] <= e (off[0] = 0, so there is one): the part of element e, empty parts skipped
CM_HD uint32_t compose_part_of(const uint32_t* off, uint32_t n_parts, uint32_t e) {
  uint32_t lo = 0, hi = n_parts;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (off[mid] <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// flag[t] and scan[t] of the 28 n pairs of all parts (k_compose_flags of mem_compose.hip and ONE scan), enqueued on st: set_lane on
// each part's own addresses, every part non-empty or skipped by `off`.  The scan's temporary lives in `tmp` until the stream has run.
void parts_flags_and_scan(const uint32_t* d_addr, const uint32_t* d_off, uint32_t n_parts, uint32_t n, DevBuf& flag, DevBuf& scan, DevBuf& tmp,
                          hipStream_t st);

// ---- the host plan ---------------------------------------------------------------------------------------------------------
// Which parts reach the device and what is launched for them.  A part is taken when it has cells, its addresses are strictly
// ascending and below 2^28 and (where the caller states one) its word count is mem_set_plan's: `part` lists the caller's indices of
// those B parts, in order.  steps: none when B == 0, else always 29 as mem_set_plan's — the cells, the per-level steps while ANY
// part's S_k is wider than SET_TAIL (k < k_tail; a part that is already narrow rides along), then the tail's steps (one launch, one
// workgroup per part).  n_nodes = the parents of all parts together, widest_part = the most any one part has.
struct BatchPlan {
  uint32_t B = 0, N = 0, W = 0, k_tail = 0;
  uint64_t n_heads = 0;                  // nodes of S_0 .. S_27 of all parts: the head lanes
  std::vector<uint32_t> part, lvl, woff;
  std::vector<cm_mem_batch_step> steps;
  const uint32_t* level(uint32_t k) const { return lvl.data() + (size_t)k * (B + 1); }
};
inline void batch_plan(const uint32_t* const* addresses, const uint32_t* n, const uint32_t* n_siblings, uint32_t n_parts, BatchPlan& bp) {
  std::vector<uint32_t> widths;          // SET_STEPS per taken part
  cm_mem_set_step steps[SET_STEPS];
  for (uint32_t i = 0; i < n_parts; i++) {
    if (n[i] == 0 || set_first_bad_address(addresses[i], n[i]) < n[i]) continue;
    const uint32_t need = mem_set_plan(addresses[i], n[i], steps);
    if (n_siblings && n_siblings[i] != need) continue;
    bp.part.push_back(i);
    bp.woff.push_back(bp.W);
    bp.W += need;
    bp.N += n[i];
    for (uint32_t s = 0; s < SET_STEPS; s++) widths.push_back(steps[s].n_nodes);
  }
  const uint32_t B = bp.B = (uint32_t)bp.part.size();
  if (B == 0) return;
  bp.woff.push_back(bp.W);
  bp.lvl.assign((size_t)SET_STEPS * (B + 1), 0u);
  uint32_t widest[SET_STEPS];
  for (uint32_t k = 0; k < SET_STEPS; k++) {
    uint32_t* const row = bp.lvl.data() + (size_t)k * (B + 1);
    widest[k] = 0;
    for (uint32_t b = 0; b < B; b++) {
      const uint32_t w = widths[(size_t)b * SET_STEPS + k];
      row[b + 1] = row[b] + w;
      widest[k] = w > widest[k] ? w : widest[k];
    }
    if (k < SET_DEPTHS) bp.n_heads += row[B];
  }
  while (bp.k_tail < SET_DEPTHS && widest[bp.k_tail] > SET_TAIL) bp.k_tail++;
  bp.steps.push_back(cm_mem_batch_step{28, bp.N, widest[0], SET_K_CELLS});
  for (uint32_t k = 0; k < SET_DEPTHS; k++)
    bp.steps.push_back(cm_mem_batch_step{27 - k, bp.level(k + 1)[B], widest[k + 1], k < bp.k_tail ? SET_K_LEVEL : SET_K_TAIL});
}

// ---- what the lanes of every batched fold read (mem_batch.hip, the batched image update of mem_image.hip), device only -------------
// Internal linkage, as set_fold.hpp's: every translation unit instantiates its own.
namespace {

// what the lanes of a batch read
struct BatchView {
  const uint32_t* lvl;    // SET_STEPS rows of B + 1
  const uint32_t* woff;   // B + 1
  const uint32_t* roots;  // PLANES per part
  const uint32_t* a;
  const unsigned long long* flag;
  const unsigned long long* scan;
  const uint32_t* heads;
  const uint32_t* words;
  uint32_t B, n_heads;
  __device__ __forceinline__ const uint32_t* level(uint32_t k) const { return lvl + (size_t)k * (B + 1); }
};
// part p's own view for set_parent_from: its slice of the addresses, of the pairs and of the words; the head lanes stay the
// batch's (the scan's high word counts the heads of the parts in front).  at = off[p], q0 = the word position at the slice's start
struct BatchPart { SetView s; uint32_t at, q0; };
__device__ __forceinline__ BatchPart batch_part(const BatchView& v, uint32_t p) {
  BatchPart bp;
  bp.at = v.lvl[p];
  const size_t slice = (size_t)SET_DEPTHS * bp.at;
  bp.q0 = (uint32_t)v.scan[slice];
  bp.s = SetView{v.a + bp.at, v.flag + slice, v.scan + slice, v.heads, v.words + v.woff[p], v.lvl[p + 1] - bp.at, v.woff[p + 1] - v.woff[p]};
  return bp;
}
// lane t with the head flag stores its lane index INSIDE its part at heads[scan[t] >> 32]
__global__ void __launch_bounds__(SET_BLOCK)
k_batch_heads(BatchView v, uint32_t n, uint32_t* __restrict__ heads) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= SET_DEPTHS * n || !(v.flag[t] >> 32)) return;
  const uint32_t p = compose_part_of(v.lvl, v.B, t / SET_DEPTHS), at = v.lvl[p], np = v.lvl[p + 1] - at;
  const uint32_t rank = (uint32_t)(v.scan[t] >> 32);
  if (rank < v.n_heads) heads[rank] = (t - SET_DEPTHS * at) % np;
}

}  // namespace

}  // namespace cm
