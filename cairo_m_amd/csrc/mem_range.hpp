// Range openings (mem_range.hip): the record's layout, the plan of its verification and the pieces the host verifier and the
// kernels share.  A range [start, start + n_cells) with last = start + n_cells - 1 covers the nodes [start >> k, last >> k] of
// depth 28 - k; hashing that interval up one depth needs the node left of it exactly when start >> k is odd (left[k]) and the
// node right of it exactly when last >> k is even (right[k]).  Host code except where CM_HD says otherwise.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "host_adapter.hpp"

namespace cm {

constexpr uint32_t RANGE_SPACE = host::MAX_ADDRESS + 1;   // 2^28 cells
constexpr uint32_t RANGE_MAX_CELLS = 1u << 24;            // one call: 256 MB of values
constexpr uint32_t RANGE_SLOTS = 28;                      // left[k], right[k]: k = 0 .. 27
constexpr uint32_t RANGE_STEPS = 1 + RANGE_SLOTS;         // the cells, then one step per depth 27 .. 0
// The single-workgroup tail takes an interval of at most this many nodes.  128: of the shapes the tests pin, (777, 4099) and
// (1000, 2048) then run six and five per-level launches, (1000, 2048) meets a level step that uses both siblings (125 .. 380 at
// depth 25, 256 nodes) and both enter the tail at 65 nodes, above half its width; a single cell enters it at width 1.
constexpr uint32_t RANGE_TAIL = 128;
// record words: 0 start, 1 n_cells, 2..29 left, 30..57 right
enum : uint32_t { RW_START = 0, RW_NCELLS = 1, RW_LEFT = 2, RW_RIGHT = RW_LEFT + RANGE_SLOTS, RANGE_WORDS = RW_RIGHT + RANGE_SLOTS };
enum : uint32_t { RANGE_K_CELLS = 0, RANGE_K_LEVEL = 1, RANGE_K_TAIL = 2 };

static_assert(sizeof(cm_mem_range_opening) == 4 * RANGE_WORDS && sizeof(cm_mem_range_step) == 24, "plain words, sizes as the header states them");

// ---- well-formedness and the fold, host and device --------------------------------------------------------------------------
CM_HD bool range_header_bad(uint32_t start, uint32_t n_cells) { return n_cells == 0 || start >= RANGE_SPACE || n_cells > RANGE_SPACE - start; }
CM_HD bool range_uses_left(uint32_t start, uint32_t k) { return (start >> k) & 1u; }
CM_HD bool range_uses_right(uint32_t last, uint32_t k) { return !((last >> k) & 1u); }
// slot s < 56 (left[s], or right[s - 28]) of a record whose header is good: 0 = fine, 1 = used and not below P, 2 = unused and not 0
CM_HD uint32_t range_slot_malformed(const uint32_t* w, uint32_t s) {
  const uint32_t k = s < RANGE_SLOTS ? s : s - RANGE_SLOTS;
  const bool used = s < RANGE_SLOTS ? range_uses_left(w[RW_START], k) : range_uses_right(w[RW_START] + w[RW_NCELLS] - 1, k);
  const uint32_t x = w[RW_LEFT + s];
  return used ? (x >= P ? 1u : 0u) : (x ? 2u : 0u);
}
// the node of depth 28 of a cell with the value v[0..3] (one call site of the permutation: the loop is not unrolled)
CM_HD uint32_t range_cell_node(const uint32_t* v) {
  uint32_t h = 0, h29_0 = 0;
#pragma unroll 1
  for (uint32_t i = 0; i < 3; i++) {
    const uint32_t l = i == 0 ? v[0] : i == 1 ? v[2] : h29_0;
    const uint32_t r = i == 0 ? v[1] : i == 1 ? v[3] : h;
    if (i == 1) h29_0 = h;
    h = host::poseidon2_hash(l, r);
  }
  return h;
}
// the children of parent p, lo >> 1 <= p <= hi >> 1, where in[i] = node lo + i of the interval [lo, hi] one depth below: two nodes
// of the interval, or at its ends a node and the record's left / right word of that depth
CM_HD void range_children(const uint32_t* in, uint32_t lo, uint32_t hi, uint32_t left, uint32_t right, uint32_t p, uint32_t& l, uint32_t& r) {
  const uint32_t c = 2u * p;   // (c == lo - 1 only when lo is odd, c + 1 == hi + 1 only when hi is even)
  l = c < lo ? left : in[c - lo];
  r = c + 1 > hi ? right : in[c + 1 - lo];
}

// ---- the lookup in a tree's node list, device only ------------------------------------------------------------------------------
constexpr uint32_t RANGE_NODE_WORDS = 8;   // a cm_merkle_node in words: index, depth, left_value, right_value, ...
// the record of `depth` that holds the pair `index` (even), or nullptr: bisection over the depth's slice, as k_open_paths (shared with
// the set openings of mem_set.hip, so the three kinds of opening read one tree alike)
__device__ __forceinline__ const uint32_t* range_find(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, uint32_t depth,
                                                      uint32_t index) {
  const uint32_t end = off[air::TREE_HEIGHT + 1 - depth];
  uint32_t lo = off[air::TREE_HEIGHT - depth], hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (nodes[RANGE_NODE_WORDS * (size_t)mid] < index) lo = mid + 1; else hi = mid;
  }
  const uint32_t* const nd = nodes + RANGE_NODE_WORDS * (size_t)lo;
  return lo < end && nd[0] == index ? nd : nullptr;
}

// ---- the plan: one record per hashing step, consumed by the device verifier and handed out by cm_mem_range_plan -------------
// steps[0]: the cells -> the nodes [start, last] of depth 28.  steps[k + 1]: the interval of depth 28 - k -> [lo, hi] of depth
// 27 - k, with left[k] / right[k] where uses_left / uses_right say so; the per-level kernel while the interval it reads is wider
// than RANGE_TAIL, the tail from there on (consecutive tail steps are one launch).  The header is good (the caller checked).
inline void mem_range_plan(uint32_t start, uint32_t n_cells, cm_mem_range_step steps[RANGE_STEPS]) {
  const uint32_t last = start + n_cells - 1;
  steps[0] = cm_mem_range_step{28, start, last, RANGE_K_CELLS, 0, 0};
  for (uint32_t k = 0; k < RANGE_SLOTS; k++) {
    const uint32_t width_in = (last >> k) - (start >> k) + 1;
    steps[k + 1] = cm_mem_range_step{27 - k, start >> (k + 1), last >> (k + 1), width_in > RANGE_TAIL ? RANGE_K_LEVEL : RANGE_K_TAIL,
                                     range_uses_left(start, k) ? 1u : 0u, range_uses_right(last, k) ? 1u : 0u};
  }
}

// ---- what the run adapter (adapter_run.inc) and the C ABI need --------------------------------------------------------------
// values[4 * n_cells] and *out = the opening of [start, start + n_cells) under the tree whose node list is `nodes`: three launches
// and one round trip on `st` (one more per further 2^19 cells of values).  The range is good (the caller checked).
void open_range(const cm_merkle_node* nodes, uint64_t n_nodes, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out,
                hipStream_t st);
// status 1 unless the range is good and at most 2^24 cells and the outputs are not NULL
void open_range_check(const char* who, uint32_t start, uint32_t n_cells, const uint32_t* values, const cm_mem_range_opening* out);

}  // namespace cm
