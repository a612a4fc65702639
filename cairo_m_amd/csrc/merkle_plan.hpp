// Which kernel hashes which layers of a mixed-degree Merkle commitment: decided here, on the host, without a HIP call or an
// allocation.  MerkleTree::plan_commit (merkle_tree.hpp) consumes the records — it allocates the layers, fills the argument
// structs and pushes the launches — and cm_merkle_plan hands them to the tests, so what they read is what runs.  The predicates
// the kernels evaluate on the device (the LDS-streaming "wide" paths) and the one merkle_layer() evaluates at launch (narrow or
// layer, chunks per wave) live here too and are called from both sides: the plan reports them, it does not restate them.
#pragma once
#include "engine.hpp"
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#if defined(__HIPCC__)
#define CM_PLAN_HD __host__ __device__ __forceinline__
#else
#define CM_PLAN_HD inline
#endif

namespace cm {

// ---- the wide path: a block streams a layer's columns through LDS (merkle_wide_quad, merkle_kernels.hpp) ------------------------
constexpr uint32_t WIDE_PTR_CAP = 2048;   // columns whose pointers fit the LDS table (16 KiB)
constexpr uint32_t WIDE_MIN_COLS = 48;    // below this a layer pays its one or two loads directly
template <int NT, int R>
CM_PLAN_HD bool wide_layer_ok(uint32_t ncols, uint32_t log_n) {
  return ncols >= WIDE_MIN_COLS && ncols <= WIDE_PTR_CAP && (16u << log_n) <= (uint32_t)(NT * R) && (4u << log_n) <= (uint32_t)NT;
}
// k_merkle_layer_quad: full blocks of 64 nodes (256 threads, 16 words each)
CM_PLAN_HD bool merkle_quad_wide(uint32_t log_size, uint32_t ncols) { return log_size >= 6 && wide_layer_ok<256, 16>(ncols, 6u); }
// k_merkle_tail: layer 2^l of its one 1024-thread block (4 words each)
CM_PLAN_HD bool merkle_tail_wide(uint32_t ncols, uint32_t l) { return wide_layer_ok<1024, 4>(ncols, l); }
// k_merkle_top, phase 2: layer 2^l of the last block (256 threads, 16 words each)
CM_PLAN_HD bool merkle_top_wide(uint32_t ncols, uint32_t l) { return wide_layer_ok<256, 16>(ncols, l); }

// ---- merkle_layer(): k_merkle_narrow or k_merkle_layer ------------------------------------------------------------------------
// Narrow layers (no columns or one SecureColumn, 2^14 nodes and more): a wave walks several 64-node chunks with the next chunk's
// loads in flight.  Returns the chunks per wave — as many as still leave >= 2 waves per wave slot of the chip (256 CUs x 32 slots),
// halved until they divide the grid — or 0 for k_merkle_layer.  Tuning key "merkle_npw" (CM_MERKLE_NPW): 0 restores
// k_merkle_layer for these layers, 1..8 force a chunk count, -1 (default) sizes it by the layer.
constexpr uint32_t MERKLE_NARROW_MIN_LOG = 14;
inline uint32_t merkle_narrow_npw(uint32_t log_size, bool has_prev, uint32_t ncols) {
  const int npw_env = tune(T_MERKLE_NPW);
  if (npw_env == 0 || !(ncols == 0 || ncols == 4) || !(has_prev || ncols) || log_size < MERKLE_NARROW_MIN_LOG) return 0;
  const uint32_t n = 1u << log_size;
  uint32_t npw = npw_env > 0 ? (uint32_t)npw_env : std::min(8u, std::max(1u, n >> 20));
  while (npw > 1 && (n % (256u * npw)) != 0) npw >>= 1;
  return npw;
}

// CM_NO_MERKLE_TOP (A/B switch, read once per process): no k_merkle_top launch, fused groups and the tail instead
inline bool merkle_use_top() {
  static const bool use_top = getenv("CM_NO_MERKLE_TOP") == nullptr;
  return use_top;
}

// ---- one record per launch, in launch order (largest layer first) ---------------------------------------------------------------
enum MerklePlanKind : uint32_t { MP_LAYER = 0, MP_NARROW = 1, MP_QUAD = 2, MP_MULTI = 3, MP_TOP = 4, MP_TAIL = 5 };
constexpr uint32_t MERKLE_PLAN_MAX_LAYERS = MERKLE_TOP_MAX_LOG + 1;   // the layers of the longest launch (k_merkle_top from 2^16)
constexpr uint32_t MERKLE_PLAN_MAX_LAUNCHES = 33;                     // one per layer of a 2^31 tree, plus the tail
struct MerkleLaunchPlan {
  uint32_t kind;                       // MerklePlanKind
  uint32_t hi, lo;                     // the launch produces the layers 2^hi .. 2^lo
  uint32_t has_prev;                   // layer hi + 1 exists (its hashes are the children of layer hi)
  uint32_t narrow_prev, narrow_nc;     // MP_NARROW: the <PREV, NC> instantiation
  uint32_t npw;                        // MP_NARROW: chunks per wave
  uint32_t wide_mask;                  // bit l: layer 2^l takes the wide LDS path (MP_QUAD: bit hi; MP_TOP: phase-2 layers; MP_TAIL)
  uint32_t col_begin;                  // first column of the launch in the sorted column list
  uint32_t ncols[MERKLE_PLAN_MAX_LAYERS];   // ncols[k]: columns of layer hi - k, k <= hi - lo
};

// `logs`: the column logs sorted by size descending (MerkleTree::prepare).  Fills out[0 .. return value).
inline uint32_t merkle_plan(const uint32_t* logs, size_t n_cols, MerkleLaunchPlan out[MERKLE_PLAN_MAX_LAUNCHES]) {
  uint32_t n_out = 0;
  const uint32_t max_log = n_cols ? logs[0] : 0;
  size_t ci = 0;
  const int tail_top = (int)std::min<uint32_t>(max_log, MERKLE_TAIL_LOG);
  const bool use_top = merkle_use_top();
  auto count_at = [&](size_t from, int l) {
    size_t cnt = 0;
    while (from + cnt < n_cols && logs[from + cnt] == (uint32_t)l) cnt++;
    return cnt;
  };
  // a launch of the layers hi .. lo that starts at column ci: counts the columns per layer and moves ci past them
  auto open = [&](uint32_t kind, int hi, int lo) -> MerkleLaunchPlan& {
    MerkleLaunchPlan& r = out[n_out++];
    r.kind = kind; r.hi = (uint32_t)hi; r.lo = (uint32_t)lo;
    r.has_prev = hi < (int)max_log ? 1u : 0u;
    r.narrow_prev = r.narrow_nc = r.npw = r.wide_mask = 0;
    r.col_begin = (uint32_t)ci;
    for (int l = hi; l >= lo; l--) {
      const size_t cnt = count_at(ci, l);
      r.ncols[hi - l] = (uint32_t)cnt;
      ci += cnt;
    }
    return r;
  };
  for (int log = (int)max_log; log > tail_top;) {
    // the whole top of the tree in one launch once no wide layer is left among the per-lane levels
    if (use_top && log <= (int)MERKLE_TOP_MAX_LOG && log >= 9) {
      bool wide_inside = false;
      size_t cj = ci;
      for (int l = log; l >= log - 8; l--) {
        const size_t cnt = count_at(cj, l);
        if (cnt >= MERKLE_QUAD_MIN_COLS) wide_inside = true;
        cj += cnt;
      }
      if (!wide_inside) {
        MerkleLaunchPlan& r = open(MP_TOP, log, 0);
        for (int l = log - 9; l >= 0; l--)
          if (merkle_top_wide(r.ncols[log - l], (uint32_t)l)) r.wide_mask |= 1u << l;
        return n_out;
      }
    }
    // group of up to MERKLE_MULTI_LEVELS layers per launch (the top layer of a group needs >= 256 nodes)
    int levels = std::min<int>((int)MERKLE_MULTI_LEVELS, log - tail_top);
    if (log < 8) levels = 1;
    // big layers are throughput-bound: one node per thread with every lane busy beats the fused kernel
    // (whose parent levels run on half / quarter of the block); fusion pays only once launches are latency-bound
    if (log >= tune(T_MERKLE_MULTI_TOP)) levels = 1;   // (default MERKLE_MULTI_MAX_TOP = 19; A/B: "merkle_multi_top")
    // a mid-size layer carrying many columns is one long compression chain per node: quad-lane kernel
    const size_t n_here = count_at(ci, log);
    const bool wide = log <= (int)MERKLE_QUAD_MAX_LOG && n_here >= MERKLE_QUAD_MIN_COLS;
    if (!wide && levels > 1) {  // a fused group must stop in front of a wide layer further down
      size_t cj = ci + n_here;
      for (int lv = 1; lv < levels; lv++) {
        const size_t cnt = count_at(cj, log - lv);
        if (log - lv <= (int)MERKLE_QUAD_MAX_LOG && cnt >= MERKLE_QUAD_MIN_COLS) { levels = lv; break; }
        cj += cnt;
      }
    }
    if (wide) {
      MerkleLaunchPlan& r = open(MP_QUAD, log, log);
      if (merkle_quad_wide((uint32_t)log, r.ncols[0])) r.wide_mask = 1u << log;
      log--;
    } else if (levels == 1) {
      MerkleLaunchPlan& r = open(MP_LAYER, log, log);
      if (const uint32_t npw = merkle_narrow_npw((uint32_t)log, r.has_prev != 0, r.ncols[0])) {
        r.kind = MP_NARROW;
        r.narrow_prev = r.has_prev;
        r.narrow_nc = r.ncols[0];
        r.npw = npw;
      }
      log--;
    } else {
      open(MP_MULTI, log, log - levels + 1);
      log -= levels;
    }
  }
  // layers 2^tail_top .. 2^0: one fused launch
  MerkleLaunchPlan& r = open(MP_TAIL, tail_top, 0);
  for (int l = tail_top; l >= 0; l--)
    if (merkle_tail_wide(r.ncols[tail_top - l], (uint32_t)l)) r.wide_mask |= 1u << l;
  return n_out;
}

}  // namespace cm
