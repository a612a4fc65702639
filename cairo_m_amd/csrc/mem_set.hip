// Set openings (cm_input_open_memory_set, cm_run_open_memory_set, cm_verify_memory_set, cm_memory_set_root_host,
// cm_verify_memory_set_host, cm_mem_set_plan): any set of cells under a 31-bit Poseidon2 memory root — the values, and depth by
// depth one sibling word per node of the set's paths whose sibling is not on a path itself (mem_set.hpp) — built on the GPU from a
// partial Merkle tree's node list, checked on the GPU with one hashing lane per parent and in host code by the same fold.
//
// The tree, the node records and the depth offsets are those of mem_open.hip; the lookup is range_find of mem_range.hpp.
// Both paths start from one pass over the 28 n pairs (shift k, address lane i), depth-major, t = k * n + i:
//   k_set_flags      lane t applies set_lane — the one rule, set_lane_given_next, behind a bisection for the next node's first
//                    lane, which the host plan knows from its walk: flag[t] = (head << 32) | needs.
//   ExclusiveSum     one scan of the 64-bit flags: the low word of scan[t] = the position of lane t's sibling word in the canonical
//                    order, the high word = the number of heads in front of it (minus that of t = k * n: the node's rank in S_k).
// Opening:
//   k_set_gather     28 n + 2 n lanes.  A lane t < 28 n with the needs flag bisects depth 28 - k's slice for the pair of
//                    x ^ 1, x = a[i] >> k, takes that half or default[28 - k] and stores it at its scanned position; the last of
//                    them also stores the total.  Lane 28 n + u bisects depth 30 for the pair 4a + 2 * (u & 1) of cell a[u / 2] and
//                    stores that half of the value (a missing record: zeros), as k_range_open.  Every word is written by exactly
//                    one lane: no atomic, the same bytes every time.
// Verification (launched from the records of mem_set_plan, which cm_mem_set_plan hands out):
//   k_set_heads      lane t with the head flag stores i at heads[scan[t] >> 32]: the head lane of every node, depth-major.
// and then the shared ladder of set_fold.hpp with the one-plane verifier policy, VerifyFold<1>:
//   k_fold_cells     one lane per cell: its four words range-checked, three Poseidon2 calls -> the node of depth 28.
//   k_fold_level     one lane per PARENT r of S_{k+1}: its head lane i (heads) is also the head of its first child in S_k, whose rank
//                    and flags say where the two children are: the node and the next sibling word (left or right by the node's
//                    parity), or two neighbouring nodes of S_k.  From one ping-pong buffer into the other.  No lane idles on an
//                    address that shares its parent with another, so the upper depths keep their waves as full as the set allows.
//   k_fold_tail      one workgroup, once S_k is at most SET_TAIL nodes: the level in LDS, a barrier between depths, every remaining
//                    depth; it checks the count of sibling words, compares with the root and writes the verdict and the root.
// A malformed word raises a flag word with a plain store (every writer stores 1).  Each kernel has one call site of the
// permutation.  Temporaries: flags and scan 2 * 8 * 28 = 448 bytes per cell on both paths; the verifier adds the head lanes (4 bytes
// per node of every S_k, at most 112 per cell), the values, the addresses and two node buffers of n words.
#include "../../include/cairom_hip.h"
#include "set_fold.hpp"
#include "mem_open.hpp"
#include "segment_input.hpp"
#include "handles.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

static_assert((uint64_t)SET_DEPTHS * SET_MAX_CELLS + 2ull * SET_MAX_CELLS < (1ull << 32), "the lanes of a launch fit 32 bits");

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SET_BLOCK)
k_set_flags(const uint32_t* __restrict__ a, uint32_t n, unsigned long long* __restrict__ flag) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= SET_DEPTHS * n) return;
  const uint32_t f = set_lane(a, n, t % n, t / n);
  flag[t] = ((unsigned long long)(f & SET_HEAD ? 1u : 0u) << 32) | (f & SET_NEEDS ? 1u : 0u);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_set_gather(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a, uint32_t n,
             const unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ scan, TreeDefaults dflt, uint32_t cap_words,
             uint32_t* __restrict__ values, uint32_t* __restrict__ words, uint32_t* __restrict__ count) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x, n_pairs = SET_DEPTHS * n;
  if (t >= n_pairs) {
    const uint32_t u = t - n_pairs;
    if (u >= 2u * n) return;
    set_gather_half(nodes, off, a, u, values);
    return;
  }
  const uint32_t needs = (uint32_t)flag[t] & 1u, pos = (uint32_t)scan[t];
  if (t == n_pairs - 1) *count = pos + needs;
  if (!needs || pos >= cap_words) return;   // (the host compares *count with its plan before it reads a word)
  words[pos] = set_gather_word(nodes, off, a, n, t, dflt);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_set_heads(const unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ scan, uint32_t n, uint32_t cap_heads,
            uint32_t* __restrict__ heads) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= SET_DEPTHS * n || !(flag[t] >> 32)) return;
  const uint32_t rank = (uint32_t)(scan[t] >> 32);
  if (rank < cap_heads) heads[rank] = t % n;
}

}  // namespace

void set_cells_enqueue(const uint32_t* values, uint32_t n, uint32_t* out, uint32_t* bad, hipStream_t st) {
  hipLaunchKernelGGL(k_fold_cells<1>, blocks_for(n, SET_BLOCK), dim3(SET_BLOCK), 0, st, FoldValues<1>{{reinterpret_cast<const uint4*>(values)}}, n, out, bad);
}

void set_fold_prepare(SetFold& f, const uint32_t* d_addr, uint32_t n, const cm_mem_set_step steps[SET_STEPS], const uint32_t* words, uint32_t n_words,
                      hipStream_t st) {
  uint64_t n_heads = 0;
  for (uint32_t s = 0; s < SET_STEPS; s++) { f.w.w[s] = steps[s].n_nodes; if (s < SET_DEPTHS) n_heads += f.w.w[s]; }
  f.heads.alloc(n_heads * 4);
  set_flags_and_scan(d_addr, n, f.flag, f.scan, f.tmp, st);
  set_heads_enqueue(f.flag, f.scan, n, (uint32_t)n_heads, f.heads.u32(), st);
  f.view = SetView{d_addr, f.flag.as<unsigned long long>(), f.scan.as<unsigned long long>(), f.heads.u32(), words, n, n_words};
}

// flag[t] and scan[t] of the 28 n pairs, enqueued on st (the scan's temporary lives in `tmp` until the stream has run)
void set_flags_and_scan(const uint32_t* d_addr, uint32_t n, DevBuf& flag, DevBuf& scan, DevBuf& tmp, hipStream_t st) {
  const uint32_t n_pairs = SET_DEPTHS * n;
  flag.alloc((size_t)n_pairs * 8);
  scan.alloc((size_t)n_pairs * 8);
  hipLaunchKernelGGL(k_set_flags, blocks_for(n_pairs, SET_BLOCK), dim3(SET_BLOCK), 0, st, d_addr, n, flag.as<unsigned long long>());
  size_t tmp_bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, flag.as<unsigned long long>(), scan.as<unsigned long long>(), (int)n_pairs, st));
  tmp.alloc(tmp_bytes ? tmp_bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, tmp_bytes, flag.as<unsigned long long>(), scan.as<unsigned long long>(), (int)n_pairs, st));
}
void set_heads_enqueue(const DevBuf& flag, const DevBuf& scan, uint32_t n, uint32_t n_heads, uint32_t* heads, hipStream_t st) {
  hipLaunchKernelGGL(k_set_heads, blocks_for((uint64_t)SET_DEPTHS * n, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const unsigned long long*)flag.as<unsigned long long>(),
                     (const unsigned long long*)scan.as<unsigned long long>(), n, n_heads, heads);
}

// what is wrong with address `bad` = set_first_bad_address(a, n) < n
std::string set_address_complaint(const uint32_t* a, uint64_t bad) {
  if (a[bad] >= RANGE_SPACE) return "address " + std::to_string(bad) + " is beyond the address space of 2^28 cells";
  return "address " + std::to_string(bad) + " is not above address " + std::to_string(bad - 1);
}

void open_set_check(const char* who, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings, uint32_t cap_siblings,
                    uint32_t* n_siblings) {
  CM_CHECK(addresses && values && siblings && n_siblings, std::string(who) + ": null argument");
  CM_CHECK(n > 0, std::string(who) + ": a set of no cells");
  CM_CHECK(n <= SET_MAX_CELLS, std::string(who) + ": more than 2^20 cells in one call: split the set");
  const uint64_t bad = set_first_bad_address(addresses, n);
  CM_CHECK(bad == n, std::string(who) + ": " + set_address_complaint(addresses, bad) + " (" + std::to_string(addresses[bad]) +
                         "): the addresses must be strictly ascending and below 2^28");
  cm_mem_set_step steps[SET_STEPS];
  const uint32_t need = mem_set_plan(addresses, (uint32_t)n, steps);
  *n_siblings = need;
  CM_CHECK(cap_siblings >= need, std::string(who) + ": room for " + std::to_string(cap_siblings) + " sibling words where the set needs " +
                                     std::to_string(need));
}

void open_set(const cm_merkle_node* nodes, uint64_t n_nodes, const uint32_t* addresses, uint32_t n, uint32_t* values, uint32_t* siblings,
              uint32_t n_siblings, hipStream_t st) {
  CM_CHECK(n > 0 && n <= SET_MAX_CELLS && n_siblings <= SET_DEPTHS * n, "memory set: a bad set reached the device path");
  const TreeDefaults dflt = tree_defaults();
  // one block behind the other: the count, the values, the words — what the trips through the landing buffer carry
  const size_t val_bytes = (size_t)n * 16, word_bytes = (size_t)n_siblings * 4, out_bytes = 16 + val_bytes + word_bytes;
  DevBuf d_addr((size_t)n * 4), d_off((air::TREE_HEIGHT + 1) * 4), d_out(out_bytes), flag, scan, tmp;
  uint32_t* const d_count = d_out.u32();
  uint32_t* const d_vals = d_out.u32() + 4;
  uint32_t* const d_words = d_vals + 4 * (size_t)n;
  stage_upload(d_addr.p, addresses, (size_t)n * 4, st);
  open_depth_offsets_enqueue(nodes, n_nodes, d_off.u32(), st);
  set_flags_and_scan(d_addr.u32(), n, flag, scan, tmp, st);
  hipLaunchKernelGGL(k_set_gather, blocks_for((uint64_t)(SET_DEPTHS + 2) * n, SET_BLOCK), dim3(SET_BLOCK), 0, st, reinterpret_cast<const uint32_t*>(nodes),
                     (const uint32_t*)d_off.u32(), (const uint32_t*)d_addr.u32(), n, (const unsigned long long*)flag.as<unsigned long long>(),
                     (const unsigned long long*)scan.as<unsigned long long>(), dflt, n_siblings, d_vals, d_words, d_count);
  CM_HIP(hipGetLastError());
  std::vector<uint8_t> words_first;   // nothing reaches the caller's arrays before the count has been compared
  for (size_t done = 0; done < out_bytes;) {
    const size_t m = std::min(out_bytes - done, TREE_LAND_BYTES);
    const uint8_t* const land = (const uint8_t*)stage_download_async(d_out.as<uint8_t>() + done, m, st);
    CM_HIP(hipStreamSynchronize(st));   // (also keeps the temporaries alive until the kernels have run)
    if (!done) {
      const uint32_t got = *(const uint32_t*)land;
      CM_CHECK(got == n_siblings, "memory set: the device counts " + std::to_string(got) + " sibling words where the host plan has " +
                                      std::to_string(n_siblings));
    }
    // bytes [done, done + m) of the block: the part of the values and the part of the words among them
    const size_t lo = std::max(done, (size_t)16), hi = done + m, split = 16 + val_bytes;
    if (lo < std::min(hi, split)) memcpy((uint8_t*)values + (lo - 16), land + (lo - done), std::min(hi, split) - lo);
    if (std::max(lo, split) < hi) memcpy((uint8_t*)siblings + (std::max(lo, split) - split), land + (std::max(lo, split) - done), hi - std::max(lo, split));
    done += m;
  }
}

namespace {
void verify_set_device(uint32_t root, const uint32_t* addresses, uint32_t n, const uint32_t* values, const uint32_t* siblings, uint32_t n_siblings,
                       uint8_t* ok, uint32_t* computed_root, hipStream_t st) {
  *ok = 0;
  if (computed_root) *computed_root = 0;
  if (n == 0) return;   // nothing to launch from: the verdict needs no GPU
  verify_fold_device<1>("memory set", {root}, addresses, n, {values}, siblings, n_siblings, ok, computed_root, st);
}
}  // namespace

}  // namespace cm

// ================================================================= C ABI
namespace cm {
int32_t set_root_host(const char* who, const uint32_t* a, uint64_t n64, const uint32_t* values, const uint32_t* words, uint32_t n_words, uint32_t* root_out,
                      const char* noun, const char* value_word) {
  if (!a || !values || !words || !root_out) return cm_set_last_error((std::string(who) + ": null argument").c_str());
  if (n64 > SET_MAX_CELLS) return cm_set_last_error((std::string(who) + ": more than 2^20 cells in one call: split the set").c_str());
  const uint32_t n = (uint32_t)n64;
  const std::string head = std::string(noun) + " of " + std::to_string(n) + " cells: ";
  auto reject = [&](const std::string& why) { cm_set_last_error((head + why).c_str()); return 11; };
  if (n == 0) return reject("no cells");
  const uint64_t bad = set_first_bad_address(a, n);
  if (bad < n) return reject(set_address_complaint(a, bad));
  for (uint64_t i = 0; i < 4ull * n; i++)
    if (values[i] >= P) return reject(std::string(value_word) + " " + std::to_string(i % 4) + " of cell " + std::to_string(a[i / 4]) + " is not below P");
  cm_mem_set_step steps[SET_STEPS];
  const uint32_t need = mem_set_plan(a, n, steps);
  if (need != n_words) return reject(std::to_string(n_words) + " sibling words where the addresses need " + std::to_string(need));
  for (uint32_t s = 1, q = 0; s < SET_STEPS; s++)
    for (uint32_t j = 0; j < steps[s].n_siblings; j++, q++)
      if (words[q] >= P) return reject("sibling " + std::to_string(q) + " (depth " + std::to_string(steps[s].depth + 1) + ") is not below P");
  // the fold as the statement words it: walk S_k in order, pair neighbours, else take the next unread word
  std::vector<uint32_t> x(a, a + n), h(n), px, ph;
  for (uint32_t i = 0; i < n; i++) h[i] = range_cell_node(values + 4 * (size_t)i);
  uint32_t q = 0;
  auto word = [&] { const uint32_t w = q < n_words ? words[q] : 0u; q++; return w; };   // (q ends at n_words: checked below)
  for (uint32_t k = 0; k < SET_DEPTHS; k++) {
    px.clear(); ph.clear();
#pragma unroll 1
    for (size_t j = 0; j < x.size(); j++) {
      uint32_t l, r;
      if (!(x[j] & 1u) && j + 1 < x.size() && x[j + 1] == x[j] + 1) { l = h[j]; r = h[j + 1]; j++; }
      else if (x[j] & 1u) { l = word(); r = h[j]; }
      else { l = h[j]; r = word(); }
      px.push_back(x[j] >> 1);
      ph.push_back(host::poseidon2_hash(l, r));
    }
    x.swap(px); h.swap(ph);
  }
  if (q != n_words || x.size() != 1) return reject("the fold read " + std::to_string(q) + " of " + std::to_string(n_words) + " sibling words");
  *root_out = h[0];
  return 0;
}
}  // namespace cm

extern "C" {
int32_t cm_mem_set_plan(const uint32_t* addresses, uint64_t n, cm_mem_set_step* steps, uint32_t cap, uint32_t* n_steps, uint32_t* n_siblings) {
  return cm::abi_guard([&] {
    CM_CHECK(addresses && steps && n_steps && n_siblings, "cm_mem_set_plan: null argument");
    CM_CHECK(n > 0 && n <= cm::SET_MAX_CELLS, "cm_mem_set_plan: no cells, or more than 2^20 cells in one call: split the set");
    const uint64_t bad = cm::set_first_bad_address(addresses, n);
    CM_CHECK(bad == n, "cm_mem_set_plan: " + cm::set_address_complaint(addresses, bad));
    CM_CHECK(cap >= cm::SET_STEPS, "cm_mem_set_plan: output buffer too small (29 steps)");
    *n_siblings = cm::mem_set_plan(addresses, (uint32_t)n, steps);
    *n_steps = cm::SET_STEPS;
  });
}
int32_t cm_input_open_memory_set(const cm_device_input* in, uint32_t which, const uint32_t* addresses, uint64_t n, uint32_t* values,
                                 uint32_t* siblings, uint32_t cap_siblings, uint32_t* n_siblings, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_input_open_memory_set");
    CM_CHECK(in && in->d && root, "cm_input_open_memory_set: null argument");
    CM_CHECK(which <= 1, "cm_input_open_memory_set: `which` is not 0 (the initial tree) or 1 (the final tree)");
    cm::open_set_check("cm_input_open_memory_set", addresses, n, values, siblings, cap_siblings, n_siblings);
    const cm::DeviceInput& d = *in->d;
    cm::bind_thread_to_library_device();
    cm::open_set((which ? d.fin_tree : d.init_tree).as<cm_merkle_node>(), which ? d.meta.n_final_tree : d.meta.n_initial_tree, addresses, (uint32_t)n,
                 values, siblings, *n_siblings, cm::thread_main_stream());
    *root = which ? d.meta.final_root : d.meta.initial_root;
  });
}
int32_t cm_verify_memory_set(uint32_t root, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings,
                             uint32_t n_siblings, uint8_t* ok, uint32_t* computed_root, cm_stream_t s) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_verify_memory_set");
    CM_CHECK(addresses && values && siblings && ok, "cm_verify_memory_set: null argument");
    CM_CHECK(n <= cm::SET_MAX_CELLS, "cm_verify_memory_set: more than 2^20 cells in one call: split the set");
    cm::bind_thread_to_library_device();
    cm::verify_set_device(root, addresses, (uint32_t)n, values, siblings, n_siblings, ok, computed_root, cm::stream_or_own(s));
  });
}
// host code: no device call on these paths
int32_t cm_memory_set_root_host(const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings, uint32_t n_siblings,
                                uint32_t* root_out) {
  return cm::abi_guard([&] { return cm::set_root_host("cm_memory_set_root_host", addresses, n, values, siblings, n_siblings, root_out); });
}
int32_t cm_verify_memory_set_host(uint32_t root, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings,
                                  uint32_t n_siblings) {
  return cm::abi_guard([&]() -> int32_t {
    uint32_t got = 0;
    const int32_t rc = cm::set_root_host("cm_verify_memory_set_host", addresses, n, values, siblings, n_siblings, &got);
    if (rc || got == root) return rc;
    cm_set_last_error(("memory set of " + std::to_string(n) + " cells: the set hashes to root " + std::to_string(got) + ", not " + std::to_string(root)).c_str());
    return 11;
  });
}
}  // extern "C"
