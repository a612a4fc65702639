// Range openings (cm_input_open_memory_range, cm_run_open_memory_range, cm_verify_memory_range, cm_verify_memory_range_host,
// cm_mem_range_plan): a contiguous run of cells under a 31-bit Poseidon2 memory root — the values, and per depth at most the node
// left and the node right of the interval the range covers (mem_range.hpp) — built on the GPU from a partial Merkle tree's node
// list, checked on the GPU level by level and in host code by the same fold.
//
// The tree, the node records and the depth offsets are those of mem_open.hip.  Opening:
//   k_range_open     2 * n_cells + 56 lanes.  Lane t < 2 * n_cells bisects depth 30 for the pair 4a + 2 * (t & 1) of cell
//                    a = start + t / 2 and stores that half of the cell's value (a missing record: zeros).  Lane 2 * n_cells + s
//                    bisects depth 28 - k's slice for the pair that holds left[k] (s = k) or right[k] (s = 28 + k), a missing record
//                    being default[28 - k], or stores 0 for a slot the range does not use.  The lookup rule of k_open_paths; every
//                    word is written by exactly one lane: no atomic, the same bytes every time.
// Verification (launched from the records of mem_range_plan, which cm_mem_range_plan hands out):
//   k_fold_cells     the set verifier's (set_cells_enqueue of mem_set.hip): one lane per cell, its four words range-checked,
//                    three Poseidon2 calls -> the node of depth 28.
//   k_range_level    one lane per parent of the next depth: its children are two nodes of the interval, or at the ends a node and
//                    the record's left[k] / right[k]; from one ping-pong buffer into the other.
//   k_range_tail     one workgroup, once the interval is at most RANGE_TAIL nodes: the level in LDS, a barrier between depths, every
//                    remaining depth; it checks the record's own words, compares with the root and writes the verdict.
// A malformed word raises a flag word with a plain store (every writer stores 1).  Each kernel has one call site of the
// permutation.
#include "../../include/cairom_hip.h"
#include "mem_range.hpp"
#include "mem_set.hpp"
#include "mem_open.hpp"
#include "segment_input.hpp"
#include "handles.hpp"
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

constexpr uint32_t RANGE_BLOCK = 256;
constexpr uint32_t RANGE_LAND_CELLS = 1u << 19;   // 8 MB of values per trip through the pinned landing buffer
// device words behind the record: the malformed flag of the cells kernel, the verdict of k_range_tail
enum : uint32_t { RW_FLAG = RANGE_WORDS, RW_VERDICT = RANGE_WORDS + 1, RANGE_DEV_WORDS = RANGE_WORDS + 2 };

static_assert(RANGE_TAIL <= 1024 && RANGE_TAIL >= 2 && 2 * RANGE_SLOTS <= RANGE_TAIL, "one workgroup holds a level and checks the 56 slots");

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(RANGE_BLOCK)
k_range_open(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, uint32_t start, uint32_t n_cells, TreeDefaults dflt,
             uint32_t* __restrict__ values, uint32_t* __restrict__ slots) {
  const uint32_t t = blockIdx.x * RANGE_BLOCK + threadIdx.x;   // (2 * 2^24 + 56 lanes at the most)
  if (t < 2u * n_cells) {
    const uint32_t* const nd = range_find(nodes, off, air::TREE_HEIGHT, 4u * (start + (t >> 1)) + 2u * (t & 1u));
    values[2 * (size_t)t] = nd ? nd[2] : 0u;
    values[2 * (size_t)t + 1] = nd ? nd[3] : 0u;
    return;
  }
  const uint32_t s = t - 2u * n_cells;
  if (s >= 2 * RANGE_SLOTS) return;
  const bool is_left = s < RANGE_SLOTS;
  const uint32_t k = is_left ? s : s - RANGE_SLOTS, depth = RANGE_SLOTS - k, last = start + n_cells - 1;
  uint32_t word = 0;
  if (is_left ? range_uses_left(start, k) : range_uses_right(last, k)) {
    // left[k] = node (start >> k) - 1, the left half of its pair; right[k] = node (last >> k) + 1, the right half of its pair
    const uint32_t* const nd = range_find(nodes, off, depth, is_left ? (start >> k) - 1 : last >> k);
    word = nd ? (is_left ? nd[2] : nd[3]) : dflt.h[depth];
  }
  slots[s] = word;
}

// in[i] = node lo + i of the interval [lo, hi]; out[j] = node (lo >> 1) + j of the depth above, j < n_out
__global__ void __launch_bounds__(RANGE_BLOCK)
k_range_level(const uint32_t* __restrict__ in, uint32_t lo, uint32_t hi, const uint32_t* __restrict__ rec, uint32_t k, uint32_t n_out,
              uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * RANGE_BLOCK + threadIdx.x;
  if (t >= n_out) return;
  uint32_t l, r;
  range_children(in, lo, hi, rec[RW_LEFT + k], rec[RW_RIGHT + k], (lo >> 1) + t, l, r);
  out[t] = host::poseidon2_hash(l, r);
}

// the interval [lo, hi] of depth 28 - k0, at most RANGE_TAIL nodes, up to the root; rec[RW_FLAG] in, rec[RW_VERDICT] out
__global__ void __launch_bounds__(RANGE_TAIL)
k_range_tail(const uint32_t* __restrict__ in, uint32_t lo, uint32_t hi, uint32_t* __restrict__ rec, uint32_t k0, uint32_t root) {
  __shared__ uint32_t level[2][RANGE_TAIL];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) bad = (rec[RW_FLAG] || range_header_bad(rec[RW_START], rec[RW_NCELLS])) ? 1u : 0u;
  if (t <= hi - lo) level[0][t] = in[t];
  __syncthreads();
  if (t < 2 * RANGE_SLOTS && !range_header_bad(rec[RW_START], rec[RW_NCELLS]) && range_slot_malformed(rec, t)) bad = 1u;
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < RANGE_SLOTS; k++) {
    const uint32_t plo = lo >> 1, phi = hi >> 1;
    if (t <= phi - plo) {
      uint32_t l, r;
      range_children(level[cur], lo, hi, rec[RW_LEFT + k], rec[RW_RIGHT + k], plo + t, l, r);
      level[cur ^ 1][t] = host::poseidon2_hash(l, r);
    }
    __syncthreads();
    lo = plo; hi = phi; cur ^= 1;
  }
  if (t == 0) rec[RW_VERDICT] = (!bad && level[cur][0] == root) ? 1u : 0u;
}

}  // namespace

void open_range_check(const char* who, uint32_t start, uint32_t n_cells, const uint32_t* values, const cm_mem_range_opening* out) {
  CM_CHECK(values && out, std::string(who) + ": null values or null output");
  CM_CHECK(n_cells > 0, std::string(who) + ": a range of no cells");
  CM_CHECK(!range_header_bad(start, n_cells), std::string(who) + ": the range [" + std::to_string(start) + ", " +
                                                  std::to_string((uint64_t)start + n_cells) + ") ends beyond the address space of 2^28 cells");
  CM_CHECK(n_cells <= RANGE_MAX_CELLS, std::string(who) + ": more than 2^24 cells in one call: split the range");
}

void open_range(const cm_merkle_node* nodes, uint64_t n_nodes, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out,
                hipStream_t st) {
  CM_CHECK(!range_header_bad(start, n_cells) && n_cells <= RANGE_MAX_CELLS, "memory range: a bad range reached the device path");
  const TreeDefaults dflt = tree_defaults();
  constexpr size_t SLOT_BYTES = 2 * RANGE_SLOTS * 4;
  DevBuf d_off((air::TREE_HEIGHT + 1) * 4), d_vals((size_t)n_cells * 16), d_slots(SLOT_BYTES);
  open_depth_offsets_enqueue(nodes, n_nodes, d_off.u32(), st);
  hipLaunchKernelGGL(k_range_open, blocks_for(2ull * n_cells + 2 * RANGE_SLOTS, RANGE_BLOCK), dim3(RANGE_BLOCK), 0, st,
                     reinterpret_cast<const uint32_t*>(nodes), (const uint32_t*)d_off.u32(), start, n_cells, dflt, d_vals.u32(), d_slots.u32());
  CM_HIP(hipGetLastError());
  // the first trip carries the slots behind its values; a longer range takes one more trip per RANGE_LAND_CELLS
  for (uint32_t done = 0; done < n_cells;) {
    const uint32_t m = std::min(n_cells - done, RANGE_LAND_CELLS);
    const size_t bytes = (size_t)m * 16;
    uint8_t* const land = (uint8_t*)stage_landing(bytes + SLOT_BYTES, st);
    CM_HIP(hipMemcpyAsync(land, d_vals.as<uint8_t>() + (size_t)done * 16, bytes, hipMemcpyDeviceToHost, st));
    if (!done) CM_HIP(hipMemcpyAsync(land + bytes, d_slots.p, SLOT_BYTES, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));   // (also keeps the temporaries alive until the kernels have run)
    memcpy(values + 4 * (size_t)done, land, bytes);
    if (!done) {
      out->start = start; out->n_cells = n_cells;
      memcpy(out->left, land + bytes, SLOT_BYTES);   // left[28] and right[28] lie back to back
    }
    done += m;
  }
}

namespace {
void verify_range_device(uint32_t root, const cm_mem_range_opening* opening, const uint32_t* values, uint8_t* ok, hipStream_t st) {
  const uint32_t start = opening->start, n_cells = opening->n_cells;
  if (range_header_bad(start, n_cells)) { *ok = 0; return; }   // nothing to launch from: the verdict needs no GPU
  cm_mem_range_step steps[RANGE_STEPS];
  mem_range_plan(start, n_cells, steps);
  uint32_t words[RANGE_DEV_WORDS];
  memcpy(words, opening, sizeof(*opening));
  words[RW_FLAG] = 0; words[RW_VERDICT] = 0;
  DevBuf d_rec(sizeof(words)), d_vals((size_t)n_cells * 16), d_a((size_t)n_cells * 4), d_b(((size_t)n_cells / 2 + 1) * 4);
  stage_upload(d_rec.p, words, sizeof(words), st);
  stage_upload(d_vals.p, values, (size_t)n_cells * 16, st);
  uint32_t* in = d_a.u32();
  uint32_t* out = d_b.u32();
  set_cells_enqueue(d_vals.u32(), n_cells, in, d_rec.u32() + RW_FLAG, st);
  uint32_t s = 1;
  for (; s < RANGE_STEPS && steps[s].kernel == RANGE_K_LEVEL; s++) {
    const uint32_t n_out = steps[s].hi - steps[s].lo + 1;   // (<= n_cells / 2 + 1: the size of the second buffer)
    hipLaunchKernelGGL(k_range_level, blocks_for(n_out, RANGE_BLOCK), dim3(RANGE_BLOCK), 0, st, (const uint32_t*)in, steps[s - 1].lo, steps[s - 1].hi,
                       (const uint32_t*)d_rec.u32(), s - 1, n_out, out);
    std::swap(in, out);
  }
  CM_CHECK(s < RANGE_STEPS && steps[s].kernel == RANGE_K_TAIL && steps[s - 1].hi - steps[s - 1].lo < RANGE_TAIL, "memory range: the plan has no tail");
  hipLaunchKernelGGL(k_range_tail, dim3(1), dim3(RANGE_TAIL), 0, st, (const uint32_t*)in, steps[s - 1].lo, steps[s - 1].hi, d_rec.u32(), s - 1, root);
  CM_HIP(hipGetLastError());
  const uint32_t* land = (const uint32_t*)stage_download_async(d_rec.u32() + RW_VERDICT, 4, st);
  CM_HIP(hipStreamSynchronize(st));   // the buffers go back to the pool behind this wait
  *ok = land[0] == 1 ? 1 : 0;
}
}  // namespace

}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_input_open_memory_range(const cm_device_input* in, uint32_t which, uint32_t start, uint32_t n_cells, uint32_t* values,
                                   cm_mem_range_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_input_open_memory_range");
    CM_CHECK(in && in->d && root, "cm_input_open_memory_range: null argument");
    CM_CHECK(which <= 1, "cm_input_open_memory_range: `which` is not 0 (the initial tree) or 1 (the final tree)");
    cm::open_range_check("cm_input_open_memory_range", start, n_cells, values, out);
    const cm::DeviceInput& d = *in->d;
    cm::bind_thread_to_library_device();
    cm::open_range((which ? d.fin_tree : d.init_tree).as<cm_merkle_node>(), which ? d.meta.n_final_tree : d.meta.n_initial_tree, start, n_cells, values,
                   out, cm::thread_main_stream());
    *root = which ? d.meta.final_root : d.meta.initial_root;
  });
}
int32_t cm_verify_memory_range(uint32_t root, const cm_mem_range_opening* opening, const uint32_t* values, uint8_t* ok, cm_stream_t s) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_verify_memory_range");
    CM_CHECK(opening && values && ok, "cm_verify_memory_range: null argument");
    CM_CHECK(opening->n_cells <= cm::RANGE_MAX_CELLS, "cm_verify_memory_range: more than 2^24 cells in one call: split the range");
    cm::bind_thread_to_library_device();
    cm::verify_range_device(root, opening, values, ok, cm::stream_or_own(s));
  });
}
// host code: no device call on this path
int32_t cm_verify_memory_range_host(uint32_t root, const cm_mem_range_opening* opening, const uint32_t* values) {
  return cm::abi_guard([&]() -> int32_t {
    if (!opening || !values) return cm_set_last_error("cm_verify_memory_range_host: null argument");
    const uint32_t* const w = reinterpret_cast<const uint32_t*>(opening);
    const uint32_t start = w[cm::RW_START], n = w[cm::RW_NCELLS];
    if (n > cm::RANGE_MAX_CELLS) return cm_set_last_error("cm_verify_memory_range_host: more than 2^24 cells in one call: split the range");
    const std::string who = "memory range [" + std::to_string(start) + ", " + std::to_string((uint64_t)start + n) + "): ";
    auto reject = [&](const std::string& why) { cm_set_last_error((who + why).c_str()); return 11; };
    if (n == 0) return reject("n_cells is 0");
    if (cm::range_header_bad(start, n)) return reject("the range ends beyond the address space of 2^28 cells");
    for (uint64_t i = 0; i < 4ull * n; i++)
      if (values[i] >= cm::P) return reject("value word " + std::to_string(i % 4) + " of cell " + std::to_string(start + i / 4) + " is not below P");
    for (uint32_t s = 0; s < 2 * cm::RANGE_SLOTS; s++) {
      const uint32_t bad = cm::range_slot_malformed(w, s);
      if (!bad) continue;
      const std::string side = s < cm::RANGE_SLOTS ? "left" : "right", depth = std::to_string(cm::RANGE_SLOTS - s % cm::RANGE_SLOTS);
      return reject(bad == 1 ? "the " + side + " sibling at depth " + depth + " is not below P" : "unused " + side + " slot at depth " + depth + " is not zero");
    }
    // the fold of the device path, step by step of the same plan
    cm_mem_range_step steps[cm::RANGE_STEPS];
    cm::mem_range_plan(start, n, steps);
    std::vector<uint32_t> a(n), b(n / 2 + 1);
    for (uint32_t i = 0; i < n; i++) a[i] = cm::range_cell_node(values + 4 * (size_t)i);
    for (uint32_t s = 1; s < cm::RANGE_STEPS; s++) {
      const uint32_t n_out = steps[s].hi - steps[s].lo + 1;
  #pragma unroll 1
      for (uint32_t j = 0; j < n_out; j++) {
        uint32_t l, r;
        cm::range_children(a.data(), steps[s - 1].lo, steps[s - 1].hi, w[cm::RW_LEFT + s - 1], w[cm::RW_RIGHT + s - 1], steps[s].lo + j, l, r);
        b[j] = cm::host::poseidon2_hash(l, r);
      }
      a.swap(b);
    }
    if (a[0] == root) return 0;
    return reject("the range hashes to root " + std::to_string(a[0]) + ", not " + std::to_string(root));
  });
}
int32_t cm_mem_range_plan(uint32_t start, uint32_t n_cells, cm_mem_range_step* steps, uint32_t cap, uint32_t* n_steps) {
  return cm::abi_guard([&] {
    CM_CHECK(steps && n_steps, "cm_mem_range_plan: null argument");
    CM_CHECK(n_cells > 0 && !cm::range_header_bad(start, n_cells), "cm_mem_range_plan: no cells, or the range ends beyond the address space of 2^28 cells");
    CM_CHECK(cap >= cm::RANGE_STEPS, "cm_mem_range_plan: output buffer too small (29 steps)");
    cm::mem_range_plan(start, n_cells, steps);
    *n_steps = cm::RANGE_STEPS;
  });
}
}  // extern "C"
