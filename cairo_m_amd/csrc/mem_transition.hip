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
// ONCE for both folds: the shared ladder of set_fold.hpp with the two-plane verifier policy, VerifyFold<2>, whose node is a pair
// (x = under the old values, y = under the new):
//   k_fold_cells     one lane per cell: all eight words range-checked, two nodes of depth 28.
//   k_fold_level     one lane per parent while S_k is wider than SET_TAIL: set_parent's index arithmetic and the sibling word once,
//                    two compressions.
//   k_fold_tail      one workgroup: the remaining depths of both planes in LDS (2 * 2 * 128 words), the count, both roots compared,
//                    the verdict and the two roots written.  Four words come back.
// Temporaries of the verifier: the set verifier's (mem_set.hip) plus 16 bytes of values and 8 of node buffers per cell.
#include "../../include/cairom_hip.h"
#include "mem_transition.hpp"
#include "set_fold.hpp"
#include "mem_open.hpp"
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace cm {
namespace {

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
               TreeDefaults dflt, uint32_t cap_words, uint32_t* __restrict__ old_values, uint32_t* __restrict__ new_values, uint32_t* __restrict__ words,
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

void verify_transition_device(uint32_t root0, uint32_t root1, const uint32_t* addresses, uint32_t n, const uint32_t* old_values, const uint32_t* new_values,
                              const uint32_t* siblings, uint32_t n_siblings, uint8_t* ok, uint32_t* computed, hipStream_t st) {
  *ok = 0;
  if (computed) computed[0] = computed[1] = 0;
  // nothing to launch from: this verdict needs no GPU
  if (n == 0) {
    // no cell changes: well formed without words, and then the memory after is the memory before
    if (n_siblings == 0 && computed) computed[0] = computed[1] = root0;
    *ok = (n_siblings == 0 && root0 == root1) ? 1 : 0;
    return;
  }
  verify_fold_device<2>("memory transition", {root0, root1}, addresses, n, {old_values, new_values}, siblings, n_siblings, ok, computed, st);
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
  download(addresses, out.p, std::min(n_total, cap_dev) * 4, st);
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
  const TreeDefaults dflt = tree_defaults();
  open_depth_offsets_enqueue(d.init_tree.as<cm_merkle_node>(), d.meta.n_initial_tree, d_off0.u32(), st);
  open_depth_offsets_enqueue(d.fin_tree.as<cm_merkle_node>(), d.meta.n_final_tree, d_off1.u32(), st);
  set_flags_and_scan(d_addr, n, flag, scan, tmp, st);
  hipLaunchKernelGGL(k_trans_gather, blocks_for((uint64_t)(SET_DEPTHS + 4) * n, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint32_t*)d.init_tree.u32(),
                     (const uint32_t*)d_off0.u32(), (const uint32_t*)d.fin_tree.u32(), (const uint32_t*)d_off1.u32(), (const uint32_t*)d_addr, n,
                     (const unsigned long long*)flag.as<unsigned long long>(), (const unsigned long long*)scan.as<unsigned long long>(), dflt, cap_words,
                     d_old, d_new, d_words, d_head + TH_COUNT);
  CM_HIP(hipGetLastError());
  // Trips of at most TREE_LAND_BYTES, from the header on when the caller brought the addresses.  The first carries the header,
  // whose count says where the block ends when the plan could not.
  static_assert(4 * (size_t)SET_MAX_CELLS + TRANS_HEAD_WORDS * 4 <= TREE_LAND_BYTES, "addresses and header fit the first trip");
  size_t total = block.bytes;
  std::vector<uint8_t> host(total);
  for (size_t done = addresses ? addr_bytes : 0, trip = 0; done < total; trip++) {
    const size_t part = std::min(total - done, TREE_LAND_BYTES);
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
extern "C" {
int32_t cm_input_write_set(const cm_device_input* in, uint32_t* addresses, uint64_t cap, uint64_t* n_total, uint64_t* n_zero_only) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_input_write_set");
    CM_CHECK(in && in->d && n_total && n_zero_only, "cm_input_write_set: null argument");
    CM_CHECK(addresses || cap == 0, "cm_input_write_set: null addresses with a capacity");
    cm::write_set(*in->d, addresses, cap, *n_total, *n_zero_only);
  });
}
int32_t cm_input_open_transition(const cm_device_input* in, const uint32_t* addresses, uint64_t n, cm_mem_transition** out) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_input_open_transition");
    CM_CHECK(in && in->d && out, "cm_input_open_transition: null argument");
    *out = cm::open_transition(*in->d, addresses, n);
  });
}
int32_t cm_mem_transition_get(const cm_mem_transition* t, cm_mem_transition_view* out) {
  return cm::abi_guard([&] {
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
  return cm::abi_guard([&] {
    cm::open_require_device("cm_verify_memory_transition");
    CM_CHECK(addresses && old_values && new_values && siblings && ok, "cm_verify_memory_transition: null argument");
    CM_CHECK(n <= cm::SET_MAX_CELLS, "cm_verify_memory_transition: more than 2^20 cells in one call: split the set");
    cm::bind_thread_to_library_device();
    cm::verify_transition_device(root_before, root_after, addresses, (uint32_t)n, old_values, new_values, siblings, n_siblings, ok, computed,
                                 cm::stream_or_own(s));
  });
}
// host code: no device call on this path.  Both folds are set_root_host's; the old side is judged, and named, first.
int32_t cm_verify_memory_transition_host(uint32_t root_before, uint32_t root_after, const uint32_t* addresses, uint64_t n, const uint32_t* old_values,
                                         const uint32_t* new_values, const uint32_t* siblings, uint32_t n_siblings) {
  return cm::abi_guard([&]() -> int32_t {
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
  });
}
}  // extern "C"
