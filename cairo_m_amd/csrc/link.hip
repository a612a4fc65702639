// Link diff of a run (cm_link_diff, cm_check_chain; the per-link half of cm_check_run): which cells make segment i's initial
// memory root differ from segment i - 1's final one.
//
// Both sides are boundary-memory row arrays (cm_memory_cell: address, value[4], clock, multiplicity) in ascending address order,
// resident in a DeviceInput.  A cell counts as a difference when the two partial Merkle trees hash different leaves for it.  An
// absent leaf hashes as the default of its depth, and the default leaf is ZERO (adapter/merkle.rs:259-265 fills missing nodes with
// H::default_hashes()[depth]; host_adapter.hpp poseidon2_default_hashes: v[TREE_HEIGHT] = 0, v[d] = hash(v[d + 1], v[d + 1])), so a
// cell that is present on one side only with value (0, 0, 0, 0) leaves the root unchanged: it is counted (n_zero_only), not
// listed.  Clocks and multiplicities are not leaves and are not compared.
//
// Three launches and one scan on the calling thread's stream, one host round trip:
//   k_link_classify  one thread per row of either array.  A block loads its 256 rows (7 KiB) cooperatively into LDS with 16-byte
//                    loads, every thread takes its row from there (row stride 7 words: odd, conflict-free) and bisects the OTHER
//                    array's addresses (4 of every 28 bytes: the upper levels of the search stay in L2).  The row's place in the
//                    merge of both arrays is its own index plus the bisection's result — prev row i sits at i + |{next < a}|,
//                    next row j at j + |{prev <= a}| — so every row owns one slot of the merged order without any atomic.
//   scan             exclusive sum of the listed flags over the merged order (hipCUB, as the run tail's gap scan)
//   k_link_compact   one thread per merged slot: a listed slot below `cap` gathers its two rows into one cm_link_cell
// The four totals are integer sums (one atomic per wave and kind): their value does not depend on the order of the adds.
//
// The classification and the scan are link_merge_enqueue, for any two row arrays: a segment's write set (mem_transition.hip) runs
// them over one input's initial and final boundary memory and compacts with
//   k_link_addresses the listed slots' addresses alone, ascending, or asks with
//   k_link_missing   for the lowest listed address that a given ascending set does not hold (a minimum).
#include "../../include/cairom_hip.h"
#include "segment_input.hpp"
#include "handles.hpp"
#include "mem_tree.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <string>

namespace cm {
namespace {

constexpr uint32_t LINK_BLOCK = 256, ROW_WORDS = 7;
constexpr uint32_t NO_ROW = 0xffffffffu, SIDE_NEXT = 0x80000000u;
// cells that travel with the totals; a caller that asked for more and has more gets the rest in a second copy
constexpr uint64_t LINK_FIRST_TRIP = 4096;

static_assert(sizeof(cm_memory_cell) == 4 * ROW_WORDS, "boundary-memory rows are seven words");
static_assert(sizeof(cm_link_cell) == 44 && sizeof(cm_link_report) == 240 && sizeof(cm_run_check) == sizeof(cm_check_report) + 240 + 16,
              "cm_link_cell / cm_link_report / cm_run_check: plain words, sizes as the header states them");

// rows of `rows` (n of them, ascending address) whose address is below a (or_equal: not above a)
__device__ __forceinline__ uint32_t rows_below(const uint32_t* __restrict__ rows, uint32_t n, uint32_t a, bool or_equal) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1), x = rows[ROW_WORDS * (size_t)mid];
    if (or_equal ? x <= a : x < a) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// blocks [0, blocks_prev) take the rows of prev, the others those of next.  flag: zeroed by the caller, n_prev + n_next words.
__global__ void __launch_bounds__(LINK_BLOCK)
k_link_classify(const uint32_t* __restrict__ prev, uint32_t n_prev, const uint32_t* __restrict__ next, uint32_t n_next, uint32_t blocks_prev,
                int vec16, uint32_t* __restrict__ flag, uint2* __restrict__ src, uint32_t* __restrict__ state) {
  __shared__ __attribute__((aligned(16))) uint32_t tile[LINK_BLOCK * ROW_WORDS];
  const bool side_next = blockIdx.x >= blocks_prev;
  const uint32_t* const own = side_next ? next : prev;
  const uint32_t* const other = side_next ? prev : next;
  const uint32_t n_own = side_next ? n_next : n_prev, n_other = side_next ? n_prev : n_next;
  const uint32_t r0 = (side_next ? blockIdx.x - blocks_prev : blockIdx.x) * LINK_BLOCK;
  const uint32_t cnt = min(LINK_BLOCK, n_own - r0), words = cnt * ROW_WORDS;
  const uint32_t* const g = own + ROW_WORDS * (size_t)r0;   // (256 rows = 7168 bytes: a tile starts 16-byte aligned when the array does)
  const uint32_t nvec = vec16 ? words >> 2 : 0u;
  for (uint32_t w = threadIdx.x; w < nvec; w += LINK_BLOCK) reinterpret_cast<uint4*>(tile)[w] = reinterpret_cast<const uint4*>(g)[w];
  for (uint32_t w = 4 * nvec + threadIdx.x; w < words; w += LINK_BLOCK) tile[w] = g[w];
  __syncthreads();
  uint32_t kind = 0;   // 1..3 as cm_link_cell, 4 = present on this side only with an all-zero value
  if (threadIdx.x < cnt) {
    const uint32_t* const row = tile + ROW_WORDS * threadIdx.x;
    const uint32_t i = r0 + threadIdx.x, a = row[0];
    if (i > 0 && (threadIdx.x ? row[-(int)ROW_WORDS] : own[ROW_WORDS * (size_t)(i - 1)]) >= a) atomicOr(state + LS_ERR, 1u);
    const bool nonzero = (row[1] | row[2] | row[3] | row[4]) != 0;
    uint32_t rank, partner = NO_ROW;
    if (!side_next) {
      const uint32_t lb = rows_below(other, n_other, a, false);
      rank = i + lb;
      if (lb < n_other && other[ROW_WORDS * (size_t)lb] == a) {
        partner = lb;
        const uint32_t* o = other + ROW_WORDS * (size_t)lb;
        kind = (o[1] != row[1] || o[2] != row[2] || o[3] != row[3] || o[4] != row[4]) ? 1u : 0u;
      } else kind = nonzero ? 3u : 4u;
    } else {
      const uint32_t ub = rows_below(other, n_other, a, true);
      rank = i + ub;
      const bool found = ub > 0 && other[ROW_WORDS * (size_t)(ub - 1)] == a;   // (the pair is judged by its prev row)
      kind = found ? 0u : nonzero ? 2u : 4u;
    }
    // rank <= (n_own - 1) + n_other whatever the arrays hold: inside flag / src even for rows that are not sorted
    if (kind >= 1 && kind <= 3) { flag[rank] = 1u; src[rank] = make_uint2(i | (side_next ? SIDE_NEXT : 0u), partner); }
  }
  for (uint32_t k = 1; k <= 4; k++) {
    const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
    if ((threadIdx.x & 63u) == 0 && c) atomicAdd(state + (k == 1 ? LS_CHANGED : k == 2 ? LS_ONLY_NEXT : k == 3 ? LS_ONLY_PREV : LS_ZERO_ONLY), c);
  }
}

__global__ void __launch_bounds__(LINK_BLOCK)
k_link_compact(const uint32_t* __restrict__ prev, uint32_t n_prev, const uint32_t* __restrict__ next, uint32_t n_next, const uint32_t* __restrict__ flag,
               const uint32_t* __restrict__ pos, const uint2* __restrict__ src, uint32_t n_slots, uint32_t cap, uint32_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * LINK_BLOCK + threadIdx.x;
  if (r >= n_slots || !flag[r]) return;
  const uint32_t p = pos[r];
  if (p >= cap) return;
  const uint2 s = src[r];
  const bool side_next = (s.x & SIDE_NEXT) != 0;
  const uint32_t i = s.x & ~SIDE_NEXT;
  if (i >= (side_next ? n_next : n_prev) || (s.y != NO_ROW && s.y >= n_next)) return;   // (never: classify wrote both)
  const uint32_t* const a = side_next ? nullptr : prev + ROW_WORDS * (size_t)i;
  const uint32_t* const b = side_next ? next + ROW_WORDS * (size_t)i : s.y != NO_ROW ? next + ROW_WORDS * (size_t)s.y : nullptr;
  uint32_t* const o = out + 11 * (size_t)p;
  o[0] = side_next ? 2u : b ? 1u : 3u;
  o[1] = a ? a[0] : b[0];
  for (int k = 0; k < 4; k++) { o[2 + k] = a ? a[1 + k] : 0u; o[6 + k] = b ? b[1 + k] : 0u; }
  o[10] = a ? a[5] : 0u;
}

// the address of the listed merged slot whose source is s
__device__ __forceinline__ uint32_t slot_address(const uint32_t* __restrict__ prev, const uint32_t* __restrict__ next, uint2 s) {
  return ((s.x & SIDE_NEXT) ? next : prev)[ROW_WORDS * (size_t)(s.x & ~SIDE_NEXT)];
}
// the write set's form of the compaction: a listed slot below `cap` stores its address alone
__global__ void __launch_bounds__(LINK_BLOCK)
k_link_addresses(const uint32_t* __restrict__ prev, const uint32_t* __restrict__ next, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                 const uint2* __restrict__ src, uint32_t n_slots, uint32_t cap, uint32_t* __restrict__ out) {
  const uint32_t r = blockIdx.x * LINK_BLOCK + threadIdx.x;
  if (r >= n_slots || !flag[r]) return;
  const uint32_t p = pos[r];
  if (p < cap) out[p] = slot_address(prev, next, src[r]);
}
// a listed slot bisects the ascending `set` (n_set addresses) for its address: *missing = the lowest one that is not there
// (a minimum: the order of the atomics does not decide it); the caller stored NO_ROW
__global__ void __launch_bounds__(LINK_BLOCK)
k_link_missing(const uint32_t* __restrict__ prev, const uint32_t* __restrict__ next, const uint32_t* __restrict__ flag, const uint2* __restrict__ src,
               uint32_t n_slots, const uint32_t* __restrict__ set, uint32_t n_set, uint32_t* __restrict__ missing) {
  const uint32_t r = blockIdx.x * LINK_BLOCK + threadIdx.x;
  if (r >= n_slots || !flag[r]) return;
  const uint32_t a = slot_address(prev, next, src[r]);
  uint32_t lo = 0, hi = n_set;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (set[mid] < a) lo = mid + 1; else hi = mid;
  }
  if (lo >= n_set || set[lo] != a) atomicMin(missing, a);
}

void set_message(cm_link_report& rep, const std::string& m) {
  const size_t n = std::min(m.size(), sizeof(rep.message) - 1);
  memcpy(rep.message, m.data(), n);
  rep.message[n] = 0;
}

void require_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw CmError(3, std::string(who) + ": no HIP device available (libcairom_hip has no CPU fallback)");
}

}  // namespace

void link_merge_enqueue(const uint32_t* a, uint64_t n_a, const uint32_t* b, uint64_t n_b, bool with_scan, LinkMerge& m, hipStream_t st) {
  const uint64_t n_slots = n_a + n_b;
  CM_CHECK(n_slots > 0 && n_slots < (1ull << 31), "link diff: boundary memories too large");
  m.prev = a; m.next = b; m.n_prev = (uint32_t)n_a; m.n_next = (uint32_t)n_b; m.n_slots = (uint32_t)n_slots;
  m.state.alloc(LS_WORDS * 4); m.flag.alloc(n_slots * 4); m.src.alloc(n_slots * 8);
  CM_HIP(hipMemsetAsync(m.state.p, 0, LS_WORDS * 4, st));
  CM_HIP(hipMemsetAsync(m.flag.p, 0, n_slots * 4, st));
  const dim3 ga = blocks_for(n_a, LINK_BLOCK), gb = blocks_for(n_b, LINK_BLOCK);
  const int vec16 = (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
  hipLaunchKernelGGL(k_link_classify, dim3(ga.x + gb.x), dim3(LINK_BLOCK), 0, st, a, (uint32_t)n_a, b, (uint32_t)n_b, ga.x, vec16, m.flag.u32(),
                     m.src.as<uint2>(), m.state.u32());
  if (!with_scan) return;
  m.pos.alloc(n_slots * 4);
  size_t tmp_bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, m.flag.u32(), m.pos.u32(), (int)n_slots, st));
  m.tmp.alloc(tmp_bytes ? tmp_bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(m.tmp.p, tmp_bytes, m.flag.u32(), m.pos.u32(), (int)n_slots, st));
}
void link_addresses_enqueue(const LinkMerge& m, uint32_t* out, uint32_t cap, hipStream_t st) {
  hipLaunchKernelGGL(k_link_addresses, blocks_for(m.n_slots, LINK_BLOCK), dim3(LINK_BLOCK), 0, st, m.prev, m.next, (const uint32_t*)m.flag.u32(),
                     (const uint32_t*)m.pos.u32(), (const uint2*)m.src.as<uint2>(), m.n_slots, cap, out);
}
void link_missing_enqueue(const LinkMerge& m, const uint32_t* set, uint32_t n_set, uint32_t* missing, hipStream_t st) {
  CM_HIP(hipMemsetAsync(missing, 0xff, 4, st));
  hipLaunchKernelGGL(k_link_missing, blocks_for(m.n_slots, LINK_BLOCK), dim3(LINK_BLOCK), 0, st, m.prev, m.next, (const uint32_t*)m.flag.u32(),
                     (const uint2*)m.src.as<uint2>(), m.n_slots, set, n_set, missing);
}

void link_diff(const DeviceInput& prev, const DeviceInput& next, uint32_t seg_index, cm_link_report& rep, cm_link_cell* cells, uint64_t cap,
               uint64_t& n_total) {
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  const uint64_t n_prev = prev.meta.n_final_memory, n_next = next.meta.n_initial_memory, n_slots = n_prev + n_next;
  CM_CHECK(n_slots < (1ull << 31), "link diff: boundary memories too large");
  uint32_t totals[LS_WORDS] = {0};
  if (n_slots) {
    const uint64_t cap_dev = std::min<uint64_t>(cap, n_slots), first = std::min<uint64_t>(cap_dev, LINK_FIRST_TRIP);
    const uint32_t* const a = prev.fin_mem.u32();
    const uint32_t* const b = next.init_mem.u32();
    LinkMerge m;
    DevBuf recs(cap_dev * sizeof(cm_link_cell) + 4);
    link_merge_enqueue(a, n_prev, b, n_next, true, m, st);
    DevBuf &state = m.state, &flag = m.flag, &pos = m.pos, &src = m.src;
    if (cap_dev)
      hipLaunchKernelGGL(k_link_compact, blocks_for(n_slots, LINK_BLOCK), dim3(LINK_BLOCK), 0, st, a, (uint32_t)n_prev, b, (uint32_t)n_next, flag.u32(), pos.u32(),
                         src.as<uint2>(), (uint32_t)n_slots, (uint32_t)cap_dev, recs.u32());
    CM_HIP(hipGetLastError());
    // totals and the first cells in one round trip
    uint8_t* land = (uint8_t*)stage_landing(LS_WORDS * 4 + first * sizeof(cm_link_cell), st);
    CM_HIP(hipMemcpyAsync(land, state.p, LS_WORDS * 4, hipMemcpyDeviceToHost, st));
    if (first) CM_HIP(hipMemcpyAsync(land + LS_WORDS * 4, recs.p, first * sizeof(cm_link_cell), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));   // (also keeps the temporaries alive until the kernels have read them)
    memcpy(totals, land, sizeof(totals));
    CM_CHECK(!totals[LS_ERR], "link diff: boundary memory rows are not in ascending address order");
    const uint64_t listed = (uint64_t)totals[LS_CHANGED] + totals[LS_ONLY_NEXT] + totals[LS_ONLY_PREV], written = std::min(listed, cap_dev);
    if (written) memcpy(cells, land + LS_WORDS * 4, std::min(written, first) * sizeof(cm_link_cell));
    if (written > first) {
      const size_t rest = (written - first) * sizeof(cm_link_cell);
      const void* more = stage_download_async(recs.as<uint8_t>() + first * sizeof(cm_link_cell), rest, st);
      CM_HIP(hipStreamSynchronize(st));
      memcpy(cells + first, more, rest);
    }
  }
  const cm_prover_input &p = prev.meta, &q = next.meta;
  const size_t keep = rep.struct_size;
  memset(&rep, 0, sizeof(rep));
  rep.struct_size = (uint32_t)keep;
  rep.prev_final_pc = p.final_pc; rep.prev_final_fp = p.final_fp; rep.next_initial_pc = q.initial_pc; rep.next_initial_fp = q.initial_fp;
  rep.pc_equal = p.final_pc == q.initial_pc; rep.fp_equal = p.final_fp == q.initial_fp; rep.roots_equal = p.final_root == q.initial_root;
  rep.prev_final_root = p.final_root; rep.next_initial_root = q.initial_root;
  rep.n_changed = totals[LS_CHANGED]; rep.n_only_next = totals[LS_ONLY_NEXT]; rep.n_only_prev = totals[LS_ONLY_PREV];
  rep.n_zero_only = totals[LS_ZERO_ONLY];
  n_total = rep.n_changed + rep.n_only_next + rep.n_only_prev;
  // first sentence: cm_verify_run's own words for the first field that differs
  std::string m;
  const char* field = !rep.pc_equal ? "pc" : !rep.fp_equal ? "fp" : !rep.roots_equal ? "root" : nullptr;
  if (field) m = "run: segment " + std::to_string(seg_index) + " initial_" + field + " != segment " + std::to_string(seg_index - 1) + " final_" + field;
  if (n_total) {
    if (!m.empty()) m += ". ";
    m += std::to_string(n_total) + " cells differ: " + std::to_string(rep.n_changed) + " changed, " + std::to_string(rep.n_only_next) + " new, " +
         std::to_string(rep.n_only_prev) + " gone";
    if (cap && cells) m += "; first address " + std::to_string(cells[0].address);
  }
  set_message(rep, m);
}

bool link_is_bad(const cm_run_check& c) {
  return !c.link.pc_equal || !c.link.fp_equal || !c.link.roots_equal || c.link_cells_total != 0;
}
// one line for cm_last_error(): the first bad link or segment in run order (link i sits in front of segment i), or empty
std::string run_check_summary(const cm_run_check* out, uint32_t n, bool with_air) {
  for (uint32_t i = 0; i < n; i++) {
    if (i > 0 && link_is_bad(out[i])) return "link " + std::to_string(i) + ": " + out[i].link.message;
    if (with_air && out[i].check.status) return "segment " + std::to_string(i) + ": " + out[i].check.message;
  }
  return "";
}
void check_link_into(const DeviceInput& prev, const DeviceInput& next, uint32_t i, cm_run_check& rec, cm_link_cell* cells, uint64_t cap_per_link) {
  rec.link.struct_size = sizeof(cm_link_report);
  uint64_t total = 0;
  link_diff(prev, next, i, rec.link, cap_per_link ? cells + (size_t)i * cap_per_link : nullptr, cap_per_link, total);
  rec.link_cells_total = total;
  rec.link_cells_written = std::min(total, cap_per_link);
}

}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_link_diff(const cm_device_input* prev, const cm_device_input* next, cm_link_report* report, cm_link_cell* cells, uint64_t cap,
                     uint64_t* n_total) {
  return cm::abi_guard([&] {
    cm::require_device("cm_link_diff");
    CM_CHECK(prev && prev->d && next && next->d && report && n_total, "cm_link_diff: null argument");
    CM_CHECK(cells || cap == 0, "cm_link_diff: null cells with a capacity");
    CM_CHECK(report->struct_size >= sizeof(cm_link_report), "cm_link_diff: struct_size does not cover cm_link_report (set it to sizeof(cm_link_report))");
    cm_link_report r;
    r.struct_size = sizeof(r);
    uint64_t total = 0;
    cm::link_diff(*prev->d, *next->d, 1, r, cells, cap, total);
    memcpy(report, &r, sizeof(r));
    *n_total = total;
  });
}
int32_t cm_check_chain(const cm_device_input* const* inputs, uint32_t n, cm_run_check* out, cm_link_cell* cells, uint64_t cap_per_link) {
  return cm::abi_guard([&] {
    cm::require_device("cm_check_chain");
    CM_CHECK(n >= 1 && inputs && out, "cm_check_chain: no inputs / null output");
    CM_CHECK(cells || cap_per_link == 0, "cm_check_chain: null cells with a capacity");
    for (uint32_t i = 0; i < n; i++) CM_CHECK(inputs[i] && inputs[i]->d, "cm_check_chain: null input");
    memset(out, 0, (size_t)n * sizeof(cm_run_check));
    for (uint32_t i = 1; i < n; i++) cm::check_link_into(*inputs[i - 1]->d, *inputs[i]->d, i, out[i], cells, cap_per_link);
    cm_set_last_error(cm::run_check_summary(out, n, false).c_str());
  });
}
}  // extern "C"
