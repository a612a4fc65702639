// Memory transitions (cm_input_write_set, cm_input_open_transition, cm_verify_memory_transition,
// cm_verify_memory_transition_host): which cells a segment changed, and their old and new values under ONE list of sibling words
// that folds to the root before with the old values and to the root after with the new ones (mem_transition.hpp).
//
// The write set is the link diff's classification and scan (link.hip: link_merge_enqueue) over one input's initial and final
// boundary memory, compacted to addresses alone: ascending, a cell present on one side only with an all-zero value counted and not
// listed.  A supplied set goes through the classification and a membership launch instead: the lowest changed cell it misses.
// Opening: the set opener's flag pass and scan (mem_set.hip), then
//   k_trans_gather   28 n + 2 n + 2 n lanes: the sibling words and the old value halves from the INITIAL tree's node list exactly
//                    as k_set_gather takes them, and 2 n more lanes that bisect depth 30 of the FINAL tree for the new halves.
//                    Every word is written by exactly one lane.
// Verification, launched from the records of mem_set_plan as the set verifier's, the flag pass, the scan and the head scatter run
// ONCE for both folds; a node is a pair (x = under the old values, y = under the new):
//   k_trans_cells    one lane per cell: all eight words range-checked, two nodes of depth 28.
//   k_trans_level    one lane per parent while S_k is wider than SET_TAIL: set_parent's index arithmetic and the sibling word once,
//                    two compressions.
//   k_trans_tail     one workgroup: the remaining depths of both planes in LDS (2 * 2 * 128 words), the count, both roots compared,
//                    the verdict and the two roots written.  Four words come back.
// Temporaries of the verifier: the set verifier's (mem_set.hip) plus 16 bytes of values and 8 of node buffers per cell.
#include "../../include/cairom_hip.h"
#include "mem_transition.hpp"
#include "mem_open.hpp"
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace cm {
namespace {

// device words of the verifier: the malformed flag of the hashing kernels, the verdict and the two roots of k_trans_tail
enum : uint32_t { TW_FLAG = 0, TW_VERDICT = 1, TW_ROOT0 = 2, TW_ROOT1 = 3, TRANS_DEV_WORDS = 4 };
// header words of the opener's block: the device's count of sibling words, the lowest changed cell the set misses (or NO_CELL),
// the write set's zero-only total and its error flag
enum : uint32_t { TH_COUNT = 0, TH_MISSING = 1, TH_ZERO_ONLY = 2, TH_ERR = 3, TRANS_HEAD_WORDS = 4 };
constexpr uint32_t NO_CELL = 0xffffffffu;

static_assert((uint64_t)(SET_DEPTHS + 4) * SET_MAX_CELLS < (1ull << 32), "the lanes of a launch fit 32 bits");
static_assert(LS_ERR == LS_ZERO_ONLY + 1 && TH_ERR == TH_ZERO_ONLY + 1, "one copy carries both words");

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SET_BLOCK)
k_trans_gather(const uint32_t* __restrict__ nodes0, const uint32_t* __restrict__ off0, const uint32_t* __restrict__ nodes1, const uint32_t* __restrict__ off1,
               const uint32_t* __restrict__ a, uint32_t n, const unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ scan,
               SetDefaults dflt, uint32_t cap_words, uint32_t* __restrict__ old_values, uint32_t* __restrict__ new_values, uint32_t* __restrict__ words,
               uint32_t* __restrict__ count) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x, n_pairs = SET_DEPTHS * n;
  if (t >= n_pairs) {
    const uint32_t u = t - n_pairs;
    if (u < 2u * n) set_gather_half(nodes0, off0, a, u, old_values);
    else if (u < 4u * n) set_gather_half(nodes1, off1, a, u - 2u * n, new_values);
    return;
  }
  const uint32_t needs = (uint32_t)flag[t] & 1u, pos = (uint32_t)scan[t];
  if (t == n_pairs - 1) *count = pos + needs;
  if (!needs || pos >= cap_words) return;   // (the host compares *count with its plan before it reads a word)
  words[pos] = set_gather_word(nodes0, off0, a, n, t, dflt);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_trans_cells(const uint4* __restrict__ old_values, const uint4* __restrict__ new_values, uint32_t n, uint2* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint4 q0 = old_values[t], q1 = new_values[t];
  const uint32_t v0[4] = {q0.x, q0.y, q0.z, q0.w}, v1[4] = {q1.x, q1.y, q1.z, q1.w};
  if (v0[0] >= P || v0[1] >= P || v0[2] >= P || v0[3] >= P || v1[0] >= P || v1[1] >= P || v1[2] >= P || v1[3] >= P) *bad = 1u;
  out[t] = make_uint2(range_cell_node(v0), range_cell_node(v1));
}

// the two children of parent r of S_{k+1} in both planes, where in[c] = node c of S_k; false as set_children
__device__ __forceinline__ bool trans_children(const SetView& s, const uint2* in, uint32_t k, uint32_t r, uint2& l, uint2& rr) {
  const SetParent p = set_parent(s, k, r);
  const uint2 me = in[p.c];
  if (p.paired) { l = me; rr = in[p.c + 1]; return true; }
  const uint2 w = make_uint2(p.w, p.w);   // the sibling word is the same under both roots: that is the statement
  l = p.odd ? w : me; rr = p.odd ? me : w;
  return p.w < P;
}

// in = S_k, out = S_{k+1} (n_out nodes)
__global__ void __launch_bounds__(SET_BLOCK)
k_trans_level(SetView s, const uint2* __restrict__ in, uint32_t k, uint32_t n_out, uint2* __restrict__ out, uint32_t* __restrict__ bad) {
  const uint32_t r = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (r >= n_out) return;
  uint2 l, rr;
  if (!trans_children(s, in, k, r, l, rr)) *bad = 1u;
  out[r] = make_uint2(host::poseidon2_hash(l.x, rr.x), host::poseidon2_hash(l.y, rr.y));
}

// S_k0 (w.w[k0] <= SET_TAIL nodes) up to both roots; dev[TW_FLAG] in, dev[TW_VERDICT], dev[TW_ROOT0] and dev[TW_ROOT1] out
__global__ void __launch_bounds__(SET_TAIL)
k_trans_tail(SetView s, const uint2* __restrict__ in, SetWidths w, uint32_t k0, uint32_t root0, uint32_t root1, uint32_t* __restrict__ dev) {
  __shared__ uint2 level[2][SET_TAIL];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    // the count of the addresses' own flags against the record's
    const size_t last = (size_t)SET_DEPTHS * s.n - 1;
    const uint32_t need = (uint32_t)s.scan[last] + ((uint32_t)s.flag[last] & 1u);
    bad = (dev[TW_FLAG] || need != s.n_words) ? 1u : 0u;
  }
  if (t < w.w[k0]) level[0][t] = in[t];
  __syncthreads();
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < SET_DEPTHS; k++) {
    if (t < w.w[k + 1]) {
      uint2 l, rr;
      if (!trans_children(s, level[cur], k, t, l, rr)) bad = 1u;
      level[cur ^ 1][t] = make_uint2(host::poseidon2_hash(l.x, rr.x), host::poseidon2_hash(l.y, rr.y));
    }
    __syncthreads();
    cur ^= 1;
  }
  if (t == 0) {
    const uint2 top = level[cur][0];
    dev[TW_VERDICT] = (!bad && top.x == root0 && top.y == root1) ? 1u : 0u;
    dev[TW_ROOT0] = bad ? 0u : top.x;
    dev[TW_ROOT1] = bad ? 0u : top.y;
  }
}

inline dim3 blocks_for(uint64_t n) { return dim3((uint32_t)((n + SET_BLOCK - 1) / SET_BLOCK)); }

// `bytes` of device memory at `src` into `dst` through the pinned landing buffer, at most SET_LAND_BYTES a trip; waits for st
void download(uint8_t* dst, const uint8_t* src, size_t bytes, hipStream_t st) {
  for (size_t done = 0; done < bytes;) {
    const size_t m = std::min(bytes - done, SET_LAND_BYTES);
    const void* land = stage_download_async(src + done, m, st);
    CM_HIP(hipStreamSynchronize(st));
    memcpy(dst + done, land, m);
    done += m;
  }
}

void verify_transition_device(uint32_t root0, uint32_t root1, const uint32_t* addresses, uint32_t n, const uint32_t* old_values, const uint32_t* new_values,
                              const uint32_t* siblings, uint32_t n_siblings, uint8_t* ok, uint32_t* computed, hipStream_t st) {
  *ok = 0;
  if (computed) computed[0] = computed[1] = 0;
  // nothing to launch from: these verdicts need no GPU
  if (n == 0) {
    // no cell changes: well formed without words, and then the memory after is the memory before
    if (n_siblings == 0 && computed) computed[0] = computed[1] = root0;
    *ok = (n_siblings == 0 && root0 == root1) ? 1 : 0;
    return;
  }
  if (set_first_bad_address(addresses, n) < n) return;
  cm_mem_set_step steps[SET_STEPS];
  if (mem_set_plan(addresses, n, steps) != n_siblings) return;
  SetWidths w;
  uint64_t n_heads = 0;
  for (uint32_t s = 0; s < SET_STEPS; s++) { w.w[s] = steps[s].n_nodes; if (s < SET_DEPTHS) n_heads += w.w[s]; }
  const uint32_t words0[TRANS_DEV_WORDS] = {0, 0, 0, 0};
  DevBuf d_dev(sizeof(words0)), d_addr((size_t)n * 4), d_old((size_t)n * 16), d_new((size_t)n * 16), d_words((size_t)n_siblings * 4), d_heads(n_heads * 4),
      d_a((size_t)n * 8), d_b((size_t)n * 8), flag, scan, tmp;
  stage_upload(d_dev.p, words0, sizeof(words0), st);
  stage_upload(d_addr.p, addresses, (size_t)n * 4, st);
  stage_upload(d_old.p, old_values, (size_t)n * 16, st);
  stage_upload(d_new.p, new_values, (size_t)n * 16, st);
  stage_upload(d_words.p, siblings, (size_t)n_siblings * 4, st);
  set_flags_and_scan(d_addr.u32(), n, flag, scan, tmp, st);
  set_heads_enqueue(flag, scan, n, (uint32_t)n_heads, d_heads.u32(), st);
  uint2* in = d_a.as<uint2>();
  uint2* out = d_b.as<uint2>();
  hipLaunchKernelGGL(k_trans_cells, blocks_for(n), dim3(SET_BLOCK), 0, st, (const uint4*)d_old.as<uint4>(), (const uint4*)d_new.as<uint4>(), n, in,
                     d_dev.u32() + TW_FLAG);
  const SetView view{d_addr.u32(), flag.as<unsigned long long>(), scan.as<unsigned long long>(), d_heads.u32(), d_words.u32(), n, n_siblings};
  uint32_t s = 1;
  for (; s < SET_STEPS && steps[s].kernel == SET_K_LEVEL; s++) {
    hipLaunchKernelGGL(k_trans_level, blocks_for(steps[s].n_nodes), dim3(SET_BLOCK), 0, st, view, (const uint2*)in, s - 1, steps[s].n_nodes, out,
                       d_dev.u32() + TW_FLAG);
    std::swap(in, out);
  }
  CM_CHECK(s < SET_STEPS && steps[s].kernel == SET_K_TAIL && w.w[s - 1] <= SET_TAIL, "memory transition: the plan has no tail");
  hipLaunchKernelGGL(k_trans_tail, dim3(1), dim3(SET_TAIL), 0, st, view, (const uint2*)in, w, s - 1, root0, root1, d_dev.u32());
  CM_HIP(hipGetLastError());
  const uint32_t* land = (const uint32_t*)stage_download_async(d_dev.p, sizeof(words0), st);
  CM_HIP(hipStreamSynchronize(st));   // the buffers go back to the pool behind this wait
  *ok = land[TW_VERDICT] == 1 ? 1 : 0;
  if (computed) { computed[0] = land[TW_ROOT0]; computed[1] = land[TW_ROOT1]; }
}

// the diff of d's initial and final boundary memory, enqueued; false (and nothing enqueued) when the input carries neither
bool write_set_merge(const DeviceInput& d, bool with_scan, LinkMerge& m, hipStream_t st) {
  const uint64_t n_init = d.meta.n_initial_memory, n_fin = d.meta.n_final_memory;
  if (n_init + n_fin == 0) return false;
  link_merge_enqueue(d.init_mem.u32(), n_init, d.fin_mem.u32(), n_fin, with_scan, m, st);
  return true;
}
// the totals of an enqueued diff: one small round trip
void write_set_totals(const LinkMerge& m, uint32_t totals[LS_WORDS], hipStream_t st) {
  const void* land = stage_download_async(m.state.p, LS_WORDS * 4, st);
  CM_HIP(hipStreamSynchronize(st));
  memcpy(totals, land, LS_WORDS * 4);
  CM_CHECK(!totals[LS_ERR], "write set: boundary memory rows are not in ascending address order");
}
inline uint64_t listed(const uint32_t totals[LS_WORDS]) { return (uint64_t)totals[LS_CHANGED] + totals[LS_ONLY_NEXT] + totals[LS_ONLY_PREV]; }

void write_set(const DeviceInput& d, uint32_t* addresses, uint64_t cap, uint64_t& n_total, uint64_t& n_zero_only) {
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  n_total = n_zero_only = 0;
  LinkMerge m;
  if (!write_set_merge(d, true, m, st)) return;
  const uint64_t cap_dev = std::min<uint64_t>(cap, m.n_slots);
  DevBuf out(cap_dev * 4);
  if (cap_dev) link_addresses_enqueue(m, out.u32(), (uint32_t)cap_dev, st);
  CM_HIP(hipGetLastError());
  uint32_t totals[LS_WORDS];
  write_set_totals(m, totals, st);
  n_total = listed(totals);
  n_zero_only = totals[LS_ZERO_ONLY];
  download((uint8_t*)addresses, out.as<uint8_t>(), std::min(n_total, cap_dev) * 4, st);
}

}  // namespace

cm_mem_transition* open_transition(const DeviceInput& d, const uint32_t* addresses, uint64_t n64) {
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  std::unique_ptr<cm_mem_transition> tr(new cm_mem_transition());
  tr->root_before = d.meta.initial_root;
  tr->root_after = d.meta.final_root;
  LinkMerge m;
  uint32_t n = 0, m_words = 0, cap_words = 0;
  bool diffed = false;
  if (addresses) {
    CM_CHECK(n64 > 0, "cm_input_open_transition: a set of no cells");
    CM_CHECK(n64 <= SET_MAX_CELLS, "cm_input_open_transition: more than 2^20 cells in one call: split the set");
    const uint64_t bad = set_first_bad_address(addresses, n64);
    CM_CHECK(bad == n64, "cm_input_open_transition: " + set_address_complaint(addresses, bad) + " (" + std::to_string(addresses[bad]) +
                             "): the addresses must be strictly ascending and below 2^28");
    n = (uint32_t)n64;
    cm_mem_set_step steps[SET_STEPS];
    cap_words = m_words = mem_set_plan(addresses, n, steps);
    diffed = write_set_merge(d, false, m, st);
  } else {
    // the write set: its size comes back, the addresses stay where the opening reads them
    uint32_t totals[LS_WORDS] = {0};
    if ((diffed = write_set_merge(d, true, m, st))) write_set_totals(m, totals, st);
    CM_CHECK(listed(totals) <= SET_MAX_CELLS, "cm_input_open_transition: the segment changes more than 2^20 cells: open it set by set");
    n = (uint32_t)listed(totals);
    tr->n_zero_only = totals[LS_ZERO_ONLY];
    if (n == 0) return tr.release();   // a read-only segment: nothing to open
    cap_words = SET_DEPTHS * n;
  }
  // one block: the addresses, the header, the old values, the new values, the words — what the trips through the landing buffer
  // carry, from the header on when the caller brought the addresses
  const size_t addr_bytes = (size_t)n * 4, head_bytes = TRANS_HEAD_WORDS * 4, val_bytes = (size_t)n * 16;
  DevBuf block(addr_bytes + head_bytes + 2 * val_bytes + std::max<size_t>(cap_words, 1) * 4), d_off0((air::TREE_HEIGHT + 1) * 4), d_off1((air::TREE_HEIGHT + 1) * 4),
      flag, scan, tmp;
  uint32_t* const d_addr = block.u32();
  uint32_t* const d_head = d_addr + n;
  uint32_t* const d_old = d_head + TRANS_HEAD_WORDS;
  uint32_t* const d_new = d_old + 4 * (size_t)n;
  uint32_t* const d_words = d_new + 4 * (size_t)n;
  const uint32_t head0[TRANS_HEAD_WORDS] = {0, NO_CELL, 0, 0};
  stage_upload(d_head, head0, sizeof(head0), st);
  if (addresses) {
    stage_upload(d_addr, addresses, addr_bytes, st);
    if (diffed) {
      // a membership pass: the lowest changed cell the set misses, and the diff's zero-only count and error flag beside it
      link_missing_enqueue(m, d_addr, n, d_head + TH_MISSING, st);
      CM_HIP(hipMemcpyAsync(d_head + TH_ZERO_ONLY, m.state.u32() + LS_ZERO_ONLY, 8, hipMemcpyDeviceToDevice, st));
    }
  } else link_addresses_enqueue(m, d_addr, n, st);
  SetDefaults dflt;
  const std::vector<uint32_t>& dh = host::poseidon2_default_hashes();
  for (uint32_t k = 0; k <= air::TREE_HEIGHT; k++) dflt.h[k] = dh[k];
  open_depth_offsets_enqueue(d.init_tree.as<cm_merkle_node>(), d.meta.n_initial_tree, d_off0.u32(), st);
  open_depth_offsets_enqueue(d.fin_tree.as<cm_merkle_node>(), d.meta.n_final_tree, d_off1.u32(), st);
  set_flags_and_scan(d_addr, n, flag, scan, tmp, st);
  hipLaunchKernelGGL(k_trans_gather, blocks_for((uint64_t)(SET_DEPTHS + 4) * n), dim3(SET_BLOCK), 0, st, (const uint32_t*)d.init_tree.u32(),
                     (const uint32_t*)d_off0.u32(), (const uint32_t*)d.fin_tree.u32(), (const uint32_t*)d_off1.u32(), (const uint32_t*)d_addr, n,
                     (const unsigned long long*)flag.as<unsigned long long>(), (const unsigned long long*)scan.as<unsigned long long>(), dflt, cap_words,
                     d_old, d_new, d_words, d_head + TH_COUNT);
  CM_HIP(hipGetLastError());
  // Trips of at most SET_LAND_BYTES, from the header on when the caller brought the addresses.  The first carries the header,
  // whose count says where the block ends when the plan could not.
  static_assert(4 * (size_t)SET_MAX_CELLS + TRANS_HEAD_WORDS * 4 <= SET_LAND_BYTES, "addresses and header fit the first trip");
  size_t total = block.bytes;
  std::vector<uint8_t> host(total);
  for (size_t done = addresses ? addr_bytes : 0, trip = 0; done < total; trip++) {
    const size_t part = std::min(total - done, SET_LAND_BYTES);
    const void* land = stage_download_async(block.as<uint8_t>() + done, part, st);
    CM_HIP(hipStreamSynchronize(st));   // (also keeps the temporaries alive until the kernels have run)
    memcpy(host.data() + done, land, part);
    done += part;
    if (trip) continue;
    uint32_t head[TRANS_HEAD_WORDS];
    memcpy(head, host.data() + addr_bytes, head_bytes);
    if (addresses) {
      CM_CHECK(!head[TH_ERR], "cm_input_open_transition: boundary memory rows are not in ascending address order");
      CM_CHECK(head[TH_MISSING] == NO_CELL, "cm_input_open_transition: cell " + std::to_string(head[TH_MISSING]) +
                                                " changes in this segment and is not in the set");
      CM_CHECK(head[TH_COUNT] == m_words, "memory transition: the device counts " + std::to_string(head[TH_COUNT]) +
                                              " sibling words where the host plan has " + std::to_string(m_words));
      tr->n_zero_only = head[TH_ZERO_ONLY];
    } else {
      CM_CHECK(head[TH_COUNT] <= cap_words, "memory transition: the device counts more sibling words than 28 per cell");
      m_words = head[TH_COUNT];
      total = addr_bytes + head_bytes + 2 * val_bytes + (size_t)m_words * 4;
    }
  }
  const uint8_t* const base = host.data();
  if (addresses) tr->addresses.assign(addresses, addresses + n);
  else {
    tr->addresses.resize(n);
    memcpy(tr->addresses.data(), base, addr_bytes);
    // the device built this set: its addresses and its count are held to the host's rule all the same
    CM_CHECK(set_first_bad_address(tr->addresses.data(), n) == n, "memory transition: the device's write set is not strictly ascending");
    cm_mem_set_step steps[SET_STEPS];
    const uint32_t plan = mem_set_plan(tr->addresses.data(), n, steps);
    CM_CHECK(plan == m_words, "memory transition: the device counts " + std::to_string(m_words) + " sibling words where the host plan has " +
                                  std::to_string(plan));
  }
  tr->old_values.resize(4 * (size_t)n);
  tr->new_values.resize(4 * (size_t)n);
  tr->siblings.resize(m_words);
  memcpy(tr->old_values.data(), base + addr_bytes + head_bytes, val_bytes);
  memcpy(tr->new_values.data(), base + addr_bytes + head_bytes + val_bytes, val_bytes);
  if (m_words) memcpy(tr->siblings.data(), base + addr_bytes + head_bytes + 2 * val_bytes, (size_t)m_words * 4);
  return tr.release();
}

}  // namespace cm

// ================================================================= C ABI
extern "C" int32_t cm_set_last_error(const char* msg);
namespace {
template <class F>
int32_t trans_guard(F&& f) {
  try { f(); return 0; }
  catch (const cm::CmError& e) { cm_set_last_error(e.what()); return e.code ? e.code : 1; }
  catch (const std::exception& e) { cm_set_last_error(e.what()); return 1; }
}
}  // namespace

extern "C" {
int32_t cm_input_write_set(const cm_device_input* in, uint32_t* addresses, uint64_t cap, uint64_t* n_total, uint64_t* n_zero_only) {
  return trans_guard([&] {
    cm::open_require_device("cm_input_write_set");
    CM_CHECK(in && in->d && n_total && n_zero_only, "cm_input_write_set: null argument");
    CM_CHECK(addresses || cap == 0, "cm_input_write_set: null addresses with a capacity");
    cm::write_set(*in->d, addresses, cap, *n_total, *n_zero_only);
  });
}
int32_t cm_input_open_transition(const cm_device_input* in, const uint32_t* addresses, uint64_t n, cm_mem_transition** out) {
  return trans_guard([&] {
    cm::open_require_device("cm_input_open_transition");
    CM_CHECK(in && in->d && out, "cm_input_open_transition: null argument");
    *out = cm::open_transition(*in->d, addresses, n);
  });
}
int32_t cm_mem_transition_get(const cm_mem_transition* t, cm_mem_transition_view* out) {
  return trans_guard([&] {
    CM_CHECK(t && out, "cm_mem_transition_get: null argument");
    CM_CHECK(out->struct_size >= sizeof(cm_mem_transition_view),
             "cm_mem_transition_get: struct_size does not cover cm_mem_transition_view (set it to sizeof(cm_mem_transition_view))");
    static_assert(sizeof(cm_mem_transition_view) == 24 + 4 * sizeof(void*), "six words and four pointers, as the header states");
    cm_mem_transition_view v;
    v.struct_size = sizeof(v);
    v.root_before = t->root_before; v.root_after = t->root_after;
    v.n = (uint32_t)t->addresses.size(); v.n_siblings = (uint32_t)t->siblings.size(); v.n_zero_only = t->n_zero_only;
    v.addresses = t->addresses.data(); v.old_values = t->old_values.data(); v.new_values = t->new_values.data(); v.siblings = t->siblings.data();
    memcpy(out, &v, sizeof(v));
  });
}
int32_t cm_mem_transition_free(cm_mem_transition* t) { delete t; return 0; }
int32_t cm_verify_memory_transition(uint32_t root_before, uint32_t root_after, const uint32_t* addresses, uint64_t n, const uint32_t* old_values,
                                    const uint32_t* new_values, const uint32_t* siblings, uint32_t n_siblings, uint8_t* ok, uint32_t computed[2],
                                    cm_stream_t s) {
  return trans_guard([&] {
    cm::open_require_device("cm_verify_memory_transition");
    CM_CHECK(addresses && old_values && new_values && siblings && ok, "cm_verify_memory_transition: null argument");
    CM_CHECK(n <= cm::SET_MAX_CELLS, "cm_verify_memory_transition: more than 2^20 cells in one call: split the set");
    cm::bind_thread_to_library_device();
    cm::verify_transition_device(root_before, root_after, addresses, (uint32_t)n, old_values, new_values, siblings, n_siblings, ok, computed,
                                 s ? (hipStream_t)(uintptr_t)s : cm::thread_main_stream());
  });
}
// host code: no device call on this path.  Both folds are set_root_host's; the old side is judged, and named, first.
int32_t cm_verify_memory_transition_host(uint32_t root_before, uint32_t root_after, const uint32_t* addresses, uint64_t n, const uint32_t* old_values,
                                         const uint32_t* new_values, const uint32_t* siblings, uint32_t n_siblings) {
  const char* const who = "cm_verify_memory_transition_host";
  if (!new_values) return cm_set_last_error((std::string(who) + ": null argument").c_str());
  const std::string head = "memory transition of " + std::to_string(n) + " cells: ";
  if (n == 0 && addresses && old_values && siblings) {
    if (n_siblings) return cm_set_last_error((head + std::to_string(n_siblings) + " sibling words where the addresses need 0").c_str()), 11;
    if (root_before == root_after) return 0;
    cm_set_last_error((head + "no cell changes, and root " + std::to_string(root_before) + " is not root " + std::to_string(root_after)).c_str());
    return 11;
  }
  uint32_t got0 = 0, got1 = 0;
  int32_t rc = cm::set_root_host(who, addresses, n, old_values, siblings, n_siblings, &got0, "memory transition", "old value word");
  if (rc) return rc;
  rc = cm::set_root_host(who, addresses, n, new_values, siblings, n_siblings, &got1, "memory transition", "new value word");
  if (rc) return rc;
  if (got0 != root_before)
    return cm_set_last_error((head + "the old values hash to root " + std::to_string(got0) + ", not " + std::to_string(root_before)).c_str()), 11;
  if (got1 != root_after)
    return cm_set_last_error((head + "the new values hash to root " + std::to_string(got1) + ", not " + std::to_string(root_after)).c_str()), 11;
  return 0;
}
}  // extern "C"
