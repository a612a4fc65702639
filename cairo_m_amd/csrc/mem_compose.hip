// Composed transitions (cm_compose_transitions): a chain of memory transitions R0 -> R1 -> ... -> Rk (mem_transition.hpp) made
// into the ONE transition R0 -> Rk over the union U of their addresses, from the records alone — no tree, no memory image, no hash.
//
// Why the records suffice.  S_k(U) = the distinct u >> k.  The composed record needs the word node(28 - k, x ^ 1) exactly when x is
// in S_k(U) and x ^ 1 is not.  Then no cell of U lies under x ^ 1; every part is valid, so the memories of the chain agree outside
// each part's set, and that subtree has the same hash under every root of the chain.  Let u be the lowest address of U under x and
// r the first part that holds u: x is in S_k(a_r), x ^ 1 is not (S_k(a_r) is a subset of S_k(U)), so part r's record holds that
// very word, at the position of the lane of u at shift k — u is also the lowest address of a_r under x, the head lane of x in
// part r, so no search is needed.  A word some part holds for a subtree that contains a cell of U may be stale (hashed before or
// after another part's write); such a word is never needed.
//
// Both paths validate on the host, part by part (addresses, the word count of mem_set_plan, the root chain), and concatenate the
// parts into one block: two tables of offsets, the addresses, the old values, the new values, the words.
// Host path (device == 0): a stable sort of the concatenation (equal addresses stay in chain order), one walk for U, the values
// and the seam check, then mem_set_plan's walk depth by depth over every part and over U to copy the words.
// GPU path (device == 1), the same launches whatever the number of parts:
//   one upload of the block; a stable radix sort (28 key bits) of the N addresses with the element index as the value;
//   k_compose_heads  one lane per sorted slot: the head flag, and on a non-head the seam check (the four old words of this element
//                    against the four new words of the slot before), atomicMin on the slot — a minimum, so no order decides it;
//   ExclusiveSum     of the head flags: the rank of each address in U; |U| and the seam slot come back in one small round trip;
//   k_compose_cells  one lane per slot: heads store U[rank], the old value and src[rank] = (part, index in part), the last slot of
//                    an address stores the new value;
//   set_flags_and_scan over U (the one rule), k_compose_flags + ONE ExclusiveSum over the 28 N pairs of all parts, each part
//                    depth-major inside its own slice (the scan at the slice start is subtracted);
//   k_compose_gather one lane per pair (k, i) of U: a head that needs a word takes (r, j) = src[i], reads the scan position of lane
//                    (k, j) of part r, bounds-checks it against the part's word count and copies the word.  Every word is written
//                    by exactly one lane, without atomics: the same call gives the same bytes;
//   one download (one more trip per further 8 MB); the device's count is compared with mem_set_plan(U) before the handle leaves.
// Temporaries on the GPU: flags and scan 448 bytes per cell of N plus of |U| (mem_set.hip's figure), the sort's buffers 16 N,
// head flags and ranks 8 N, the uploaded block (36 N + 4 per word) and the result (36 |U| + 112 |U| reserved for words): the cap
// of 2^20 cells bounds a call near 1 GB (derived from the layout, not measured).
// Two deviations from the obvious shape, both for less work: the gather does not search part r for the head lane (see above), and
// no tail flag is stored — k_compose_cells reads the successor's address itself.
#include "../../include/cairom_hip.h"
#include "mem_transition.hpp"
#include "mem_batch.hpp"
#include "mem_open.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

namespace cm {
namespace {

constexpr uint32_t COMPOSE_MAX_PARTS = 1u << 16;
constexpr uint32_t NO_SLOT = 0xffffffffu;
// the words of the small round trip, behind the N + 1 ranks: |U| is rank[N]
enum : uint32_t { CR_CELLS = 0, CR_SEAM = 1, COMPOSE_TRIP_WORDS = 2 };
// header words of the result block: the device's count of sibling words, the gather's error flag
enum : uint32_t { CH_COUNT = 0, CH_ERR = 1, COMPOSE_HEAD_WORDS = 4 };

static_assert((uint64_t)SET_DEPTHS * SET_MAX_CELLS < (1ull << 32), "the lanes of a launch fit 32 bits");

inline uint32_t round4(uint32_t x) { return (x + 3u) & ~3u; }

// (compose_part_of, the part of an element, is mem_batch.hpp's: the batched verifiers bisect the same tables)

// A validated chain as one block of words, every array on a 16-byte boundary:
// off[n_parts + 1] | woff[n_parts + 1] | addresses[N] | old[4 N] | new[4 N] | words[W]
struct Chain {
  uint32_t n_parts = 0, N = 0, W = 0, root_before = 0, root_after = 0, n_zero_only = 0;
  std::vector<uint32_t> block;
  size_t at_woff() const { return round4(n_parts + 1); }
  size_t at_addr() const { return 2 * at_woff(); }
  size_t at_old() const { return at_addr() + round4(N); }
  size_t at_new() const { return at_old() + 4 * (size_t)N; }
  size_t at_words() const { return at_new() + 4 * (size_t)N; }
  size_t size() const { return at_words() + W; }
  const uint32_t* off() const { return block.data(); }
  const uint32_t* woff() const { return block.data() + at_woff(); }
  const uint32_t* addr() const { return block.data() + at_addr(); }
  const uint32_t* old_values() const { return block.data() + at_old(); }
  const uint32_t* new_values() const { return block.data() + at_new(); }
  const uint32_t* words() const { return block.data() + at_words(); }
};

[[noreturn]] void reject(const std::string& why) { throw CmError(11, why); }

std::string seam_complaint(const Chain& c, uint32_t e, uint32_t e_before) {
  return "cell " + std::to_string(c.addr()[e]) + ": part " + std::to_string(compose_part_of(c.off(), c.n_parts, e)) + " reads a value part " +
         std::to_string(compose_part_of(c.off(), c.n_parts, e_before)) + " did not leave";
}

// every refusal that needs no hash, in this order: the arguments of every part and the total (status 1), then part by part its
// addresses, its word count and its place in the chain (status 11).  A part's words are not read before its count is established.
Chain chain_of(const cm_mem_transition_view* parts, uint32_t n_parts) {
  const std::string who = "cm_compose_transitions: ";
  uint64_t cells = 0, zero_only = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const cm_mem_transition_view& p = parts[i];
    const std::string part = who + "part " + std::to_string(i);
    CM_CHECK(p.struct_size >= sizeof(cm_mem_transition_view),
             part + ": struct_size does not cover cm_mem_transition_view (set it to sizeof(cm_mem_transition_view))");
    CM_CHECK((p.n == 0 || (p.addresses && p.old_values && p.new_values)) && (p.n_siblings == 0 || p.siblings), part + ": null array");
    cells += p.n;
    zero_only += p.n_zero_only;
  }
  CM_CHECK(cells <= SET_MAX_CELLS, who + "the parts hold " + std::to_string(cells) +
                                       " cells, more than 2^20 in one call: compose in groups (the operation is associative)");
  Chain c;
  c.n_parts = n_parts;
  c.N = (uint32_t)cells;
  c.n_zero_only = (uint32_t)zero_only;
  c.root_before = parts[0].root_before;
  c.root_after = parts[n_parts - 1].root_after;
  uint64_t words = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const cm_mem_transition_view& p = parts[i];
    const std::string part = "part " + std::to_string(i);
    const uint64_t bad = set_first_bad_address(p.addresses, p.n);
    if (bad < p.n) reject(part + ": " + set_address_complaint(p.addresses, bad));
    cm_mem_set_step steps[SET_STEPS];
    const uint32_t need = p.n ? mem_set_plan(p.addresses, p.n, steps) : 0u;
    if (need != p.n_siblings) reject(part + ": " + std::to_string(p.n_siblings) + " sibling words where the addresses need " + std::to_string(need));
    if (i && p.root_before != parts[i - 1].root_after)
      reject(part + " starts at root " + std::to_string(p.root_before) + ", part " + std::to_string(i - 1) + " ended at root " +
             std::to_string(parts[i - 1].root_after));
    words += need;
  }
  c.W = (uint32_t)words;   // (at most 28 N)
  c.block.assign(c.size(), 0u);
  uint32_t* const b = c.block.data();
  uint32_t at = 0, wat = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const cm_mem_transition_view& p = parts[i];
    b[i] = at;
    b[c.at_woff() + i] = wat;
    if (p.n) {
      memcpy(b + c.at_addr() + at, p.addresses, (size_t)p.n * 4);
      memcpy(b + c.at_old() + 4 * (size_t)at, p.old_values, (size_t)p.n * 16);
      memcpy(b + c.at_new() + 4 * (size_t)at, p.new_values, (size_t)p.n * 16);
    }
    if (p.n_siblings) memcpy(b + c.at_words() + wat, p.siblings, (size_t)p.n_siblings * 4);
    at += p.n;
    wat += p.n_siblings;
  }
  b[n_parts] = at;
  b[c.at_woff() + n_parts] = wat;
  return c;
}

std::unique_ptr<cm_mem_transition> result_of(const Chain& c) {
  std::unique_ptr<cm_mem_transition> tr(new cm_mem_transition());
  tr->root_before = c.root_before;
  tr->root_after = c.root_after;
  tr->n_zero_only = c.n_zero_only;
  return tr;
}

// ---- host path ---------------------------------------------------------------------------------------------------------
// One depth of mem_set_plan's walk: h[0 .. cnt) = the head lanes of a[0 .. n) at shift k; on_needs(j) for every head that needs a
// word, in record order; h then holds the heads of shift k + 1, whose count is returned.
template <class F>
uint32_t walk_depth(const uint32_t* a, uint32_t n, uint32_t k, uint32_t* h, uint32_t cnt, F&& on_needs) {
  uint32_t m = 0;
  for (uint32_t jj = 0; jj < cnt; jj++) {
    const uint32_t j = h[jj], next = jj + 1 < cnt ? h[jj + 1] : n;
    if (set_lane_given_next(a, n, j, k, next) & SET_NEEDS) on_needs(j);
    if (j == 0 || (a[j - 1] >> (k + 1)) != (a[j] >> (k + 1))) h[m++] = j;   // (m <= jj: behind what is still to be read)
  }
  return m;
}

cm_mem_transition* compose_host(const Chain& c) {
  std::unique_ptr<cm_mem_transition> tr = result_of(c);
  const uint32_t N = c.N, n_parts = c.n_parts;
  if (N == 0) return tr.release();
  const uint32_t* const addr = c.addr();
  const uint32_t* const off = c.off();
  const uint32_t* const woff = c.woff();
  // the merge: the parts are ascending runs in chain order, and the sort is stable
  std::vector<uint32_t> order(N), src;
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return addr[x] < addr[y]; });
  for (uint32_t s = 0; s < N; s++) {
    const uint32_t e = order[s];
    if (s && addr[order[s - 1]] == addr[e]) {
      if (memcmp(c.old_values() + 4 * (size_t)e, c.new_values() + 4 * (size_t)order[s - 1], 16)) reject(seam_complaint(c, e, order[s - 1]));
    } else {
      tr->addresses.push_back(addr[e]);
      tr->old_values.insert(tr->old_values.end(), c.old_values() + 4 * (size_t)e, c.old_values() + 4 * (size_t)e + 4);
      src.push_back(e);
    }
    if (s + 1 == N || addr[order[s + 1]] != addr[e])
      tr->new_values.insert(tr->new_values.end(), c.new_values() + 4 * (size_t)e, c.new_values() + 4 * (size_t)e + 4);
  }
  // the words, depth by depth: where each part's record holds the word of each of its heads, then U's heads take theirs
  const uint32_t nu = (uint32_t)tr->addresses.size();
  const uint32_t* const u = tr->addresses.data();
  std::vector<uint32_t> heads(N), n_heads(n_parts), base(n_parts, 0u), pos(N), uheads(nu);
  for (uint32_t r = 0; r < n_parts; r++) {
    n_heads[r] = off[r + 1] - off[r];
    std::iota(heads.begin() + off[r], heads.begin() + off[r + 1], 0u);
  }
  std::iota(uheads.begin(), uheads.end(), 0u);
  uint32_t n_uheads = nu;
  for (uint32_t k = 0; k < SET_DEPTHS; k++) {
    std::fill(pos.begin(), pos.end(), NO_SLOT);
    for (uint32_t r = 0; r < n_parts; r++)
      n_heads[r] = walk_depth(addr + off[r], off[r + 1] - off[r], k, heads.data() + off[r], n_heads[r], [&](uint32_t j) { pos[off[r] + j] = base[r]++; });
    n_uheads = walk_depth(u, nu, k, uheads.data(), n_uheads, [&](uint32_t i) {
      const uint32_t e = src[i], r = compose_part_of(off, n_parts, e), q = pos[e];
      CM_CHECK(q != NO_SLOT && q < woff[r + 1] - woff[r], "composed transition: part " + std::to_string(r) + " holds no word for cell " +
                                                              std::to_string(u[i]) + " at depth " + std::to_string(SET_DEPTHS - k));
      tr->siblings.push_back(c.words()[woff[r] + q]);
    });
  }
  return tr.release();
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SET_BLOCK)
k_compose_iota(uint32_t* __restrict__ v, uint32_t n) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t < n) v[t] = t;
}

// head[s] for the N sorted slots and head[N] = 0 (so that the exclusive scan ends in |U|); the seam check on every non-head
__global__ void __launch_bounds__(SET_BLOCK)
k_compose_heads(const uint32_t* __restrict__ saddr, const uint32_t* __restrict__ se, uint32_t n, const uint4* __restrict__ old_values,
                const uint4* __restrict__ new_values, uint32_t* __restrict__ head, uint32_t* __restrict__ seam) {
  const uint32_t s = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (s > n) return;
  if (s == n) { head[s] = 0u; return; }
  const bool h = s == 0 || saddr[s - 1] != saddr[s];
  head[s] = h ? 1u : 0u;
  if (h) return;
  const uint4 o = old_values[se[s]], w = new_values[se[s - 1]];
  if (o.x != w.x || o.y != w.y || o.z != w.z || o.w != w.w) atomicMin(seam, s);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_compose_cells(const uint32_t* __restrict__ saddr, const uint32_t* __restrict__ se, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank,
                uint32_t n, const uint32_t* __restrict__ off, uint32_t n_parts, const uint4* __restrict__ old_values, const uint4* __restrict__ new_values,
                uint32_t n_cells, uint32_t* __restrict__ u, uint4* __restrict__ u_old, uint4* __restrict__ u_new, uint2* __restrict__ src) {
  const uint32_t s = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (s >= n) return;
  const uint32_t a = saddr[s], h = head[s], e = se[s], r = rank[s] + h - 1u;   // (a non-head has a head in front of it)
  if (r >= n_cells) return;
  if (h) {
    const uint32_t p = compose_part_of(off, n_parts, e);
    u[r] = a;
    u_old[r] = old_values[e];
    src[r] = make_uint2(p, e - off[p]);
  }
  if (s + 1 == n || saddr[s + 1] != a) u_new[r] = new_values[e];
}

// the flags of every part, set_lane on its own addresses: pair t lies in the slice [28 off[p], 28 off[p + 1]) of its part, depth-major
__global__ void __launch_bounds__(SET_BLOCK)
k_compose_flags(const uint32_t* __restrict__ addr, const uint32_t* __restrict__ off, uint32_t n_parts, uint32_t n, unsigned long long* __restrict__ flag) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= SET_DEPTHS * n) return;
  const uint32_t p = compose_part_of(off, n_parts, t / SET_DEPTHS), at = off[p], np = off[p + 1] - at, tl = t - SET_DEPTHS * at;
  const uint32_t f = set_lane(addr + at, np, tl % np, tl / np);
  flag[t] = ((unsigned long long)(f & SET_HEAD ? 1u : 0u) << 32) | (f & SET_NEEDS ? 1u : 0u);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_compose_gather(uint32_t n_cells, const unsigned long long* __restrict__ uflag, const unsigned long long* __restrict__ uscan, const uint2* __restrict__ src,
                 const uint32_t* __restrict__ off, uint32_t n_parts, const uint32_t* __restrict__ woff, const uint32_t* __restrict__ words, uint32_t n,
                 const unsigned long long* __restrict__ pflag, const unsigned long long* __restrict__ pscan, uint32_t cap_words,
                 uint32_t* __restrict__ out, uint32_t* __restrict__ head) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x, n_pairs = SET_DEPTHS * n_cells;
  if (t >= n_pairs) return;
  const uint32_t needs = (uint32_t)uflag[t] & 1u, pos = (uint32_t)uscan[t];
  if (t == n_pairs - 1) head[CH_COUNT] = pos + needs;
  if (!needs || pos >= cap_words) return;   // (the host compares the count with its plan before it reads a word)
  const uint32_t k = t / n_cells;
  const uint2 rj = src[t % n_cells];
  if (rj.x >= n_parts) { head[CH_ERR] = 1u; return; }
  const uint32_t at = off[rj.x], np = off[rj.x + 1] - at, n_words = woff[rj.x + 1] - woff[rj.x];
  const uint32_t slice = SET_DEPTHS * at, tp = slice + k * np + rj.y;
  if (rj.y >= np || tp >= SET_DEPTHS * n) { head[CH_ERR] = 1u; return; }
  const uint32_t q = (uint32_t)pscan[tp] - (uint32_t)pscan[slice];
  if (!((uint32_t)pflag[tp] & 1u) || q >= n_words) { head[CH_ERR] = 1u; return; }
  out[pos] = words[woff[rj.x] + q];
}

// ---- GPU path ----------------------------------------------------------------------------------------------------------
cm_mem_transition* compose_device(const Chain& c) {
  std::unique_ptr<cm_mem_transition> tr = result_of(c);
  const uint32_t N = c.N, n_parts = c.n_parts;
  if (N == 0) return tr.release();   // nothing to launch from
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  DevBuf d_in, d_iota, d_saddr, d_se, d_head, d_rank, d_src, d_out, tmp_sort, tmp_rank, tmp_parts, tmp_u, pflag, pscan, uflag, uscan;
  const StreamWait wait{st};
  // 1. one upload
  d_in.alloc(c.size() * 4);
  stage_upload(d_in.p, c.block.data(), c.size() * 4, st);
  const uint32_t* const d_off = d_in.u32();
  const uint32_t* const d_woff = d_in.u32() + c.at_woff();
  const uint32_t* const d_addr = d_in.u32() + c.at_addr();
  const uint4* const d_old = (const uint4*)(d_in.u32() + c.at_old());
  const uint4* const d_new = (const uint4*)(d_in.u32() + c.at_new());
  const uint32_t* const d_words = d_in.u32() + c.at_words();
  // 2. the merge: equal addresses come out in chain order
  d_iota.alloc((size_t)N * 4); d_saddr.alloc((size_t)N * 4); d_se.alloc((size_t)N * 4);
  hipLaunchKernelGGL(k_compose_iota, blocks_for(N, SET_BLOCK), dim3(SET_BLOCK), 0, st, d_iota.u32(), N);
  size_t bytes = 0;
  CM_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, d_addr, d_saddr.u32(), (const uint32_t*)d_iota.u32(), d_se.u32(), (int)N, 0, 28, st));
  tmp_sort.alloc(bytes ? bytes : 4);
  CM_HIP(hipcub::DeviceRadixSort::SortPairs(tmp_sort.p, bytes, d_addr, d_saddr.u32(), (const uint32_t*)d_iota.u32(), d_se.u32(), (int)N, 0, 28, st));
  // 3. heads, the seam check, the ranks; rank[N] = |U| and the seam slot behind it come back together
  d_head.alloc((size_t)(N + 1) * 4);
  d_rank.alloc((size_t)(N + 1 + COMPOSE_TRIP_WORDS) * 4);
  uint32_t* const d_trip = d_rank.u32() + N;
  const uint32_t no_seam = NO_SLOT;
  stage_upload(d_trip + CR_SEAM, &no_seam, 4, st);
  hipLaunchKernelGGL(k_compose_heads, blocks_for((uint64_t)N + 1, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint32_t*)d_saddr.u32(), (const uint32_t*)d_se.u32(), N, d_old,
                     d_new, d_head.u32(), d_trip + CR_SEAM);
  bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_head.u32(), d_rank.u32(), (int)(N + 1), st));
  tmp_rank.alloc(bytes ? bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp_rank.p, bytes, d_head.u32(), d_rank.u32(), (int)(N + 1), st));
  CM_HIP(hipGetLastError());
  uint32_t trip[COMPOSE_TRIP_WORDS];
  {
    const void* land = stage_download_async(d_trip, sizeof(trip), st);
    CM_HIP(hipStreamSynchronize(st));
    memcpy(trip, land, sizeof(trip));
  }
  if (trip[CR_SEAM] != NO_SLOT) {
    const uint32_t s = trip[CR_SEAM];
    CM_CHECK(s >= 1 && s < N, "composed transition: the device names a seam slot outside the chain");
    uint32_t e[2];
    const void* land = stage_download_async(d_se.u32() + (s - 1), sizeof(e), st);
    CM_HIP(hipStreamSynchronize(st));
    memcpy(e, land, sizeof(e));
    CM_CHECK(e[0] < N && e[1] < N, "composed transition: the device names an element outside the chain");
    reject(seam_complaint(c, e[1], e[0]));
  }
  const uint32_t nu = trip[CR_CELLS];
  CM_CHECK(nu >= 1 && nu <= N, "composed transition: the device counts " + std::to_string(nu) + " cells in the union of " + std::to_string(N));
  // 4. the cells of U; the result block: the header, the old values, the new values, the addresses, the words
  const uint32_t cap_words = SET_DEPTHS * nu;
  const size_t head_bytes = COMPOSE_HEAD_WORDS * 4, val_bytes = (size_t)nu * 16, addr_bytes = (size_t)nu * 4;
  d_out.alloc(head_bytes + 2 * val_bytes + addr_bytes + (size_t)cap_words * 4);
  d_src.alloc((size_t)nu * 8);
  uint32_t* const o_head = d_out.u32();
  uint4* const o_old = (uint4*)(o_head + COMPOSE_HEAD_WORDS);
  uint4* const o_new = o_old + nu;
  uint32_t* const o_addr = (uint32_t*)(o_new + nu);
  uint32_t* const o_words = o_addr + nu;
  const uint32_t head0[COMPOSE_HEAD_WORDS] = {0, 0, 0, 0};
  stage_upload(o_head, head0, sizeof(head0), st);
  hipLaunchKernelGGL(k_compose_cells, blocks_for(N, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint32_t*)d_saddr.u32(), (const uint32_t*)d_se.u32(),
                     (const uint32_t*)d_head.u32(), (const uint32_t*)d_rank.u32(), N, d_off, n_parts, d_old, d_new, nu, o_addr, o_old, o_new, d_src.as<uint2>());
  // 5. the flags of U by the one rule, the flags of all parts in one pass and one scan
  set_flags_and_scan(o_addr, nu, uflag, uscan, tmp_u, st);
  parts_flags_and_scan(d_addr, d_off, n_parts, N, pflag, pscan, tmp_parts, st);
  // 6. the words
  hipLaunchKernelGGL(k_compose_gather, blocks_for((uint64_t)SET_DEPTHS * nu, SET_BLOCK), dim3(SET_BLOCK), 0, st, nu, (const unsigned long long*)uflag.as<unsigned long long>(),
                     (const unsigned long long*)uscan.as<unsigned long long>(), (const uint2*)d_src.as<uint2>(), d_off, n_parts, d_woff, d_words, N,
                     (const unsigned long long*)pflag.as<unsigned long long>(), (const unsigned long long*)pscan.as<unsigned long long>(), cap_words, o_words,
                     o_head);
  CM_HIP(hipGetLastError());
  // 7. trips of at most TREE_LAND_BYTES; the first carries the header, whose count says where the block ends
  size_t total = head_bytes + 2 * val_bytes + addr_bytes + (size_t)cap_words * 4;
  uint32_t m_words = 0;
  std::vector<uint8_t> host(total);
  for (size_t done = 0, t = 0; done < total; t++) {
    const size_t part = std::min(total - done, TREE_LAND_BYTES);
    const void* land = stage_download_async(d_out.as<uint8_t>() + done, part, st);
    CM_HIP(hipStreamSynchronize(st));
    memcpy(host.data() + done, land, part);
    done += part;
    if (t) continue;
    uint32_t head[COMPOSE_HEAD_WORDS];
    memcpy(head, host.data(), head_bytes);
    CM_CHECK(!head[CH_ERR], "composed transition: a part's record holds no word where the union needs one");
    CM_CHECK(head[CH_COUNT] <= cap_words, "composed transition: the device counts more sibling words than 28 per cell");
    m_words = head[CH_COUNT];
    total = head_bytes + 2 * val_bytes + addr_bytes + (size_t)m_words * 4;
  }
  const uint8_t* const base = host.data() + head_bytes;
  tr->addresses.resize(nu);
  tr->old_values.resize(4 * (size_t)nu);
  tr->new_values.resize(4 * (size_t)nu);
  tr->siblings.resize(m_words);
  memcpy(tr->old_values.data(), base, val_bytes);
  memcpy(tr->new_values.data(), base + val_bytes, val_bytes);
  memcpy(tr->addresses.data(), base + 2 * val_bytes, addr_bytes);
  if (m_words) memcpy(tr->siblings.data(), base + 2 * val_bytes + addr_bytes, (size_t)m_words * 4);
  // the device built this set: its addresses and its count are held to the host's rule all the same
  CM_CHECK(set_first_bad_address(tr->addresses.data(), nu) == nu, "composed transition: the device's union is not strictly ascending");
  cm_mem_set_step steps[SET_STEPS];
  const uint32_t plan = mem_set_plan(tr->addresses.data(), nu, steps);
  CM_CHECK(plan == m_words, "composed transition: the device counts " + std::to_string(m_words) + " sibling words where the host plan has " + std::to_string(plan));
  return tr.release();
}

}  // namespace

// the segmented flag pass and its scan, also the first step of the batched verifiers (mem_batch.hip)
void parts_flags_and_scan(const uint32_t* d_addr, const uint32_t* d_off, uint32_t n_parts, uint32_t n, DevBuf& flag, DevBuf& scan, DevBuf& tmp,
                          hipStream_t st) {
  const uint32_t n_pairs = SET_DEPTHS * n;
  flag.alloc((size_t)n_pairs * 8);
  scan.alloc((size_t)n_pairs * 8);
  hipLaunchKernelGGL(k_compose_flags, blocks_for(n_pairs, SET_BLOCK), dim3(SET_BLOCK), 0, st, d_addr, d_off, n_parts, n, flag.as<unsigned long long>());
  size_t bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, flag.as<unsigned long long>(), scan.as<unsigned long long>(), (int)n_pairs, st));
  tmp.alloc(bytes ? bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, flag.as<unsigned long long>(), scan.as<unsigned long long>(), (int)n_pairs, st));
}

}  // namespace cm

// ================================================================= C ABI
extern "C" int32_t cm_compose_transitions(const cm_mem_transition_view* parts, uint32_t n_parts, uint32_t device, cm_mem_transition** out) {
  return cm::abi_guard([&] {
    if (device == 1) cm::open_require_device("cm_compose_transitions");   // before any argument is looked at
    if (out) *out = nullptr;
    CM_CHECK(device <= 1, "cm_compose_transitions: `device` is not 0 (host code) or 1 (the GPU)");
    CM_CHECK(parts && out, "cm_compose_transitions: null argument");
    CM_CHECK(n_parts >= 1 && n_parts <= cm::COMPOSE_MAX_PARTS, "cm_compose_transitions: no parts, or more than 2^16 parts in one call: compose in groups");
    const cm::Chain c = cm::chain_of(parts, n_parts);
    *out = device ? cm::compose_device(c) : cm::compose_host(c);
  });
}
