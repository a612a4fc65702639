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
//   k_set_cells      one lane per cell: its four words range-checked, three Poseidon2 calls -> the node of depth 28.
//   k_set_level      one lane per PARENT r of S_{k+1}: its head lane i (heads) is also the head of its first child in S_k, whose rank
//                    and flags say where the two children are: the node and the next sibling word (left or right by the node's
//                    parity), or two neighbouring nodes of S_k.  From one ping-pong buffer into the other.  No lane idles on an
//                    address that shares its parent with another, so the upper depths keep their waves as full as the set allows.
//   k_set_tail       one workgroup, once S_k is at most SET_TAIL nodes: the level in LDS, a barrier between depths, every remaining
//                    depth; it checks the count of sibling words, compares with the root and writes the verdict and the root.
// A malformed word raises a flag word with a plain store (every writer stores 1).  Each kernel has one call site of the
// permutation.  Temporaries: flags and scan 2 * 8 * 28 = 448 bytes per cell on both paths; the verifier adds the head lanes (4 bytes
// per node of every S_k, at most 112 per cell), the values, the addresses and two node buffers of n words.
#include "../../include/cairom_hip.h"
#include "mem_set.hpp"
#include "mem_open.hpp"
#include "segment_input.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

// device words of the verifier: the malformed flag of the hashing kernels, the verdict and the root of k_set_tail
enum : uint32_t { SW_FLAG = 0, SW_VERDICT = 1, SW_ROOT = 2, SET_DEV_WORDS = 3 };

static_assert(SET_TAIL <= 1024 && SET_TAIL >= 2, "one workgroup holds a level");
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
             const unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ scan, SetDefaults dflt, uint32_t cap_words,
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

__global__ void __launch_bounds__(SET_BLOCK)
k_set_cells(const uint4* __restrict__ values, uint32_t n, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint4 q = values[t];
  const uint32_t v[4] = {q.x, q.y, q.z, q.w};
  if (v[0] >= P || v[1] >= P || v[2] >= P || v[3] >= P) *bad = 1u;
  out[t] = range_cell_node(v);
}

// the children of parent r of S_{k+1}, where in[c] = node c of S_k; false when the sibling word it needs is missing or not below P
__device__ __forceinline__ bool set_children(const SetView& s, const uint32_t* in, uint32_t k, uint32_t r, uint32_t& l, uint32_t& rr) {
  const SetParent p = set_parent(s, k, r);
  const uint32_t me = in[p.c];
  if (p.paired) { l = me; rr = in[p.c + 1]; return true; }
  l = p.odd ? p.w : me; rr = p.odd ? me : p.w;
  return p.w < P;
}

// in = S_k, out = S_{k+1} (n_out nodes)
__global__ void __launch_bounds__(SET_BLOCK)
k_set_level(SetView s, const uint32_t* __restrict__ in, uint32_t k, uint32_t n_out, uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint32_t r = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (r >= n_out) return;
  uint32_t l, rr;
  if (!set_children(s, in, k, r, l, rr)) *bad = 1u;
  out[r] = host::poseidon2_hash(l, rr);
}

// S_k0 (w.w[k0] <= SET_TAIL nodes) up to the root; dev[SW_FLAG] in, dev[SW_VERDICT] and dev[SW_ROOT] out
__global__ void __launch_bounds__(SET_TAIL)
k_set_tail(SetView s, const uint32_t* __restrict__ in, SetWidths w, uint32_t k0, uint32_t root, uint32_t* __restrict__ dev) {
  __shared__ uint32_t level[2][SET_TAIL];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    // the count of the addresses' own flags against the record's
    const size_t last = (size_t)SET_DEPTHS * s.n - 1;
    const uint32_t need = (uint32_t)s.scan[last] + ((uint32_t)s.flag[last] & 1u);
    bad = (dev[SW_FLAG] || need != s.n_words) ? 1u : 0u;
  }
  if (t < w.w[k0]) level[0][t] = in[t];
  __syncthreads();
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < SET_DEPTHS; k++) {
    if (t < w.w[k + 1]) {
      uint32_t l, rr;
      if (!set_children(s, level[cur], k, t, l, rr)) bad = 1u;
      level[cur ^ 1][t] = host::poseidon2_hash(l, rr);
    }
    __syncthreads();
    cur ^= 1;
  }
  if (t == 0) {
    dev[SW_VERDICT] = (!bad && level[cur][0] == root) ? 1u : 0u;
    dev[SW_ROOT] = bad ? 0u : level[cur][0];
  }
}

inline dim3 blocks_for(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }
inline hipStream_t stream_or_own(cm_stream_t s) { return s ? (hipStream_t)(uintptr_t)s : thread_main_stream(); }

}  // namespace

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
  SetDefaults dflt;
  const std::vector<uint32_t>& dh = host::poseidon2_default_hashes();
  for (uint32_t d = 0; d <= air::TREE_HEIGHT; d++) dflt.h[d] = dh[d];
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
    const size_t m = std::min(out_bytes - done, SET_LAND_BYTES);
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
  // nothing to launch from: these verdicts need no GPU
  if (n == 0 || set_first_bad_address(addresses, n) < n) return;
  cm_mem_set_step steps[SET_STEPS];
  if (mem_set_plan(addresses, n, steps) != n_siblings) return;
  SetWidths w;
  uint64_t n_heads = 0;
  for (uint32_t s = 0; s < SET_STEPS; s++) { w.w[s] = steps[s].n_nodes; if (s < SET_DEPTHS) n_heads += w.w[s]; }
  const uint32_t words0[SET_DEV_WORDS] = {0, 0, 0};
  DevBuf d_dev(sizeof(words0)), d_addr((size_t)n * 4), d_vals((size_t)n * 16), d_words((size_t)n_siblings * 4), d_heads(n_heads * 4),
      d_a((size_t)n * 4), d_b((size_t)n * 4), flag, scan, tmp;
  stage_upload(d_dev.p, words0, sizeof(words0), st);
  stage_upload(d_addr.p, addresses, (size_t)n * 4, st);
  stage_upload(d_vals.p, values, (size_t)n * 16, st);
  stage_upload(d_words.p, siblings, (size_t)n_siblings * 4, st);
  set_flags_and_scan(d_addr.u32(), n, flag, scan, tmp, st);
  set_heads_enqueue(flag, scan, n, (uint32_t)n_heads, d_heads.u32(), st);
  uint32_t* in = d_a.u32();
  uint32_t* out = d_b.u32();
  hipLaunchKernelGGL(k_set_cells, blocks_for(n, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint4*)d_vals.as<uint4>(), n, in, d_dev.u32() + SW_FLAG);
  const SetView view{d_addr.u32(), flag.as<unsigned long long>(), scan.as<unsigned long long>(), d_heads.u32(), d_words.u32(), n, n_siblings};
  uint32_t s = 1;
  for (; s < SET_STEPS && steps[s].kernel == SET_K_LEVEL; s++) {
    hipLaunchKernelGGL(k_set_level, blocks_for(steps[s].n_nodes, SET_BLOCK), dim3(SET_BLOCK), 0, st, view, (const uint32_t*)in, s - 1, steps[s].n_nodes, out,
                       d_dev.u32() + SW_FLAG);
    std::swap(in, out);
  }
  CM_CHECK(s < SET_STEPS && steps[s].kernel == SET_K_TAIL && w.w[s - 1] <= SET_TAIL, "memory set: the plan has no tail");
  hipLaunchKernelGGL(k_set_tail, dim3(1), dim3(SET_TAIL), 0, st, view, (const uint32_t*)in, w, s - 1, root, d_dev.u32());
  CM_HIP(hipGetLastError());
  const uint32_t* land = (const uint32_t*)stage_download_async(d_dev.p, sizeof(words0), st);
  CM_HIP(hipStreamSynchronize(st));   // the buffers go back to the pool behind this wait
  *ok = land[SW_VERDICT] == 1 ? 1 : 0;
  if (computed_root) *computed_root = land[SW_ROOT];
}
}  // namespace

}  // namespace cm

// ================================================================= C ABI
extern "C" int32_t cm_set_last_error(const char* msg);
namespace {
template <class F>
int32_t set_guard(F&& f) {
  try { f(); return 0; }
  catch (const cm::CmError& e) { cm_set_last_error(e.what()); return e.code ? e.code : 1; }
  catch (const std::exception& e) { cm_set_last_error(e.what()); return 1; }
}
}  // namespace

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
  return set_guard([&] {
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
  return set_guard([&] {
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
  return set_guard([&] {
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
  return cm::set_root_host("cm_memory_set_root_host", addresses, n, values, siblings, n_siblings, root_out);
}
int32_t cm_verify_memory_set_host(uint32_t root, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings,
                                  uint32_t n_siblings) {
  uint32_t got = 0;
  const int32_t rc = cm::set_root_host("cm_verify_memory_set_host", addresses, n, values, siblings, n_siblings, &got);
  if (rc || got == root) return rc;
  cm_set_last_error(("memory set of " + std::to_string(n) + " cells: the set hashes to root " + std::to_string(got) + ", not " + std::to_string(root)).c_str());
  return 11;
}
}  // extern "C"
