// Batched verification of memory transitions and sets (cm_verify_memory_transitions, cm_verify_memory_sets, cm_mem_batch_plan):
// many records, each with a set of its own, through ONE ladder of launches whose length is that of the part with the most
// per-level steps — a follower's per-segment checks are launch-bound, so they are batched as cells, proofs and programs already are.
//
// Host: the argument checks (status 1, before any address is read), then per part the checks the single-record verifiers make
// before their first launch (set_first_bad_address, mem_set_plan against n_siblings).  A part that fails them has its verdict
// here and is left out; batch_plan (mem_batch.hpp) lays the others out and is also what cm_mem_batch_plan hands out.
// Device, PLANES = 2 for transitions and 1 for sets from the same templates, the same launches whatever the number of parts:
//   one upload of one block: the parts' device words (zeros), lvl, woff, the roots, the addresses, the value planes, the words;
//   k_compose_flags + ONE ExclusiveSum over the 28 N pairs, part-major (mem_compose.hip's, shared);
//   k_batch_heads    lane t with the head flag stores its lane index INSIDE its part at heads[scan[t] >> 32]: the scan counts the
//                    heads of the parts in front, so the ranks of part p start at the high word of the scan at its slice;
//   k_batch_cells    k_fold_cells on the concatenation; a range failure raises the flag word of the lane's own part;
//   k_batch_level    one lane per parent of the combined S_{k+1}: it bisects lvl[k + 1] for its part, does set_parent's index
//                    arithmetic inside that part's slice (set_parent_from), reads and writes the part's slice of the two ping-pong
//                    node buffers and raises the part's flag word with a plain store.  Launched while ANY part's S_k is wider
//                    than SET_TAIL; a part that is already narrow rides along;
//   k_batch_tail     one workgroup of SET_TAIL lanes per part: the level in LDS, the remaining depths, the count of the part's own
//                    flags against its n_words, the root or roots compared, [flag, verdict, root0, root1] written;
//   one download of the 4 B words, one wait.
// Each kernel has one call site of the permutation per plane (fold_hash of set_fold.hpp).  Temporaries per cell of the batch: the
// single-record verifier's (flags and scan 448 bytes, head lanes at most 112, 16 per value plane, the address, two node buffers
// of 4 per plane) plus, per part, 29 + 1 + PLANES + 4 words of tables.
#include "../../include/cairom_hip.h"
#include "mem_batch.hpp"
#include "mem_open.hpp"
#include "set_fold.hpp"
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

namespace cm {
namespace {

static_assert(sizeof(cm_mem_set_view) == 16 + 3 * sizeof(void*), "four words and three pointers, as the header states");
static_assert(BATCH_ROOT + 2 == BATCH_WORDS && BATCH_FLAG == FOLD_FLAG, "a part's words hold both planes' roots");

// VerifyFold's parent with the word position taken from the part's slice
template <class Node>
__device__ __forceinline__ Node batch_parent(const BatchPart& bp, const Node* in, uint32_t k, uint32_t r, bool& bad) {
  const SetParent p = set_parent_from(bp.s, k, r, bp.q0);
  const Node me = in[p.c];
  Node l = me, rr;
  if (p.paired) rr = in[p.c + 1];
  else {
    Node w;
    fold_splat(p.w, w);
    bad = !(p.w < P);   // missing (set_parent answers P), or not a field element
    l = p.odd ? w : me; rr = p.odd ? me : w;
  }
  return fold_hash(l, rr);   // ONE call site of the permutation per plane
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
template <uint32_t PLANES>
__global__ void __launch_bounds__(SET_BLOCK)
k_batch_cells(FoldValues<PLANES> values, BatchView bv, uint32_t n, typename FoldPlanes<PLANES>::Node* __restrict__ out, uint32_t* __restrict__ dev) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  uint32_t v[PLANES][4], h[PLANES];
  bool range = true;
#pragma unroll
  for (uint32_t j = 0; j < PLANES; j++) {
    const uint4 q = values.v[j][t];
    v[j][0] = q.x; v[j][1] = q.y; v[j][2] = q.z; v[j][3] = q.w;
    range = range && q.x < P && q.y < P && q.z < P && q.w < P;
  }
  if (!range) dev[BATCH_WORDS * compose_part_of(bv.lvl, bv.B, t) + BATCH_FLAG] = 1u;
#pragma unroll
  for (uint32_t j = 0; j < PLANES; j++) h[j] = range_cell_node(v[j]);
  if constexpr (PLANES == 1) out[t] = h[0];
  else out[t] = make_uint2(h[0], h[1]);
}

// in = every part's S_k at its slice, out = every part's S_{k+1} (n_out nodes in all)
template <uint32_t PLANES>
__global__ void __launch_bounds__(SET_BLOCK)
k_batch_level(BatchView v, const typename FoldPlanes<PLANES>::Node* __restrict__ in, uint32_t k, uint32_t n_out,
              typename FoldPlanes<PLANES>::Node* __restrict__ out, uint32_t* __restrict__ dev) {
  const uint32_t g = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (g >= n_out) return;
  const uint32_t* const row = v.level(k + 1);
  const uint32_t p = compose_part_of(row, v.B, g), r = g - row[p];
  const BatchPart bp = batch_part(v, p);
  bool bad = false;
  out[bp.at + r] = batch_parent(bp, in + bp.at, k, r, bad);   // (r < |S_{k+1}| of the part <= its cells: inside its slice)
  if (bad) dev[BATCH_WORDS * p + BATCH_FLAG] = 1u;
}

// part blockIdx.x: its S_k0 (at most SET_TAIL nodes: the host plan's k_tail) up to the top, and its four words
template <uint32_t PLANES>
__global__ void __launch_bounds__(SET_TAIL)
k_batch_tail(BatchView v, const typename FoldPlanes<PLANES>::Node* __restrict__ in, uint32_t k0, uint32_t* __restrict__ dev) {
  using Node = typename FoldPlanes<PLANES>::Node;
  __shared__ Node level[2][SET_TAIL];
  __shared__ uint32_t w[SET_STEPS];
  __shared__ uint32_t bad;
  const uint32_t t = threadIdx.x, p = blockIdx.x;
  const BatchPart bp = batch_part(v, p);
  uint32_t* const mine = dev + BATCH_WORDS * p;
  if (t < SET_STEPS) {
    const uint32_t* const row = v.level(t);
    const uint32_t width = row[p + 1] - row[p];
    w[t] = width < SET_TAIL ? width : SET_TAIL;   // (the plan's are at most SET_TAIL from k0 on)
  }
  if (t == 0) {
    // the count of the part's own flags against its record's
    const size_t last = (size_t)SET_DEPTHS * bp.s.n - 1;
    const uint32_t need = (uint32_t)bp.s.scan[last] + ((uint32_t)bp.s.flag[last] & 1u) - bp.q0;
    bad = (mine[BATCH_FLAG] || need != bp.s.n_words) ? 1u : 0u;
  }
  __syncthreads();
  if (t < w[k0]) level[0][t] = in[bp.at + t];
  __syncthreads();
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < SET_DEPTHS; k++) {
    if (t < w[k + 1]) {
      bool b = false;
      level[cur ^ 1][t] = batch_parent(bp, (const Node*)level[cur], k, t, b);
      if (b) bad = 1u;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (t != 0) return;
  const Node top = level[cur][0];
  bool same = true;
#pragma unroll
  for (uint32_t j = 0; j < 2; j++) {
    if (j < PLANES) same = same && fold_plane(top, j) == v.roots[PLANES * p + j];
    mine[BATCH_ROOT + j] = (bad || j >= PLANES) ? 0u : fold_plane(top, j);
  }
  mine[BATCH_VERDICT] = (!bad && same) ? 1u : 0u;
}

// ---- the device path -------------------------------------------------------------------------------------------------------
inline size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

// one part as the host sees it, either kind
template <uint32_t PLANES> struct HostPart { const uint32_t* a; const uint32_t* v[PLANES]; const uint32_t* w; uint32_t n, m, root[PLANES]; };

// ok[i] and computed[PLANES i ..] of the parts bp.part lists; every other part has its verdict already
template <uint32_t PLANES>
void verify_batch_device(const BatchPlan& bp, const std::vector<HostPart<PLANES>>& parts, uint8_t* ok, uint32_t* computed, hipStream_t st) {
  using Node = typename FoldPlanes<PLANES>::Node;
  const uint32_t B = bp.B, N = bp.N, W = bp.W;
  if (B == 0) return;   // nothing to launch from
  // the block, every array on a 16-byte boundary: dev[4 B] | lvl[29 (B + 1)] | woff[B + 1] | roots[PLANES B] | addresses[N] |
  // values[4 N] per plane | words[W]
  const size_t at_lvl = (size_t)BATCH_WORDS * B, at_woff = at_lvl + round4((size_t)SET_STEPS * (B + 1)), at_roots = at_woff + round4(B + 1),
               at_addr = at_roots + round4((size_t)PLANES * B), at_vals = at_addr + round4(N), at_words = at_vals + (size_t)PLANES * 4 * N,
               total = at_words + W;
  std::vector<uint32_t> block(total, 0u);
  memcpy(block.data() + at_lvl, bp.lvl.data(), bp.lvl.size() * 4);
  memcpy(block.data() + at_woff, bp.woff.data(), bp.woff.size() * 4);
  const uint32_t* const off = bp.level(0);
  for (uint32_t b = 0; b < B; b++) {
    const HostPart<PLANES>& p = parts[bp.part[b]];
    for (uint32_t j = 0; j < PLANES; j++) {
      block[at_roots + (size_t)PLANES * b + j] = p.root[j];
      memcpy(block.data() + at_vals + (size_t)j * 4 * N + 4 * (size_t)off[b], p.v[j], (size_t)p.n * 16);
    }
    memcpy(block.data() + at_addr + off[b], p.a, (size_t)p.n * 4);
    if (p.m) memcpy(block.data() + at_words + bp.woff[b], p.w, (size_t)p.m * 4);
  }
  DevBuf d_block(total * 4), d_heads(bp.n_heads * 4), d_a((size_t)N * sizeof(Node)), d_b((size_t)N * sizeof(Node)), flag, scan, tmp;
  const StreamWait wait{st};   // nothing goes back to the pool while the stream still runs, on the error paths too
  stage_upload(d_block.p, block.data(), total * 4, st);
  uint32_t* const d_dev = d_block.u32();
  const uint32_t* const d_lvl = d_block.u32() + at_lvl;
  const uint32_t* const d_addr = d_block.u32() + at_addr;
  parts_flags_and_scan(d_addr, d_lvl, B, N, flag, scan, tmp, st);
  const BatchView v{d_lvl, d_block.u32() + at_woff, d_block.u32() + at_roots, d_addr, flag.as<unsigned long long>(), scan.as<unsigned long long>(),
                    d_heads.u32(), d_block.u32() + at_words, B, (uint32_t)bp.n_heads};
  hipLaunchKernelGGL(k_batch_heads, blocks_for((uint64_t)SET_DEPTHS * N, SET_BLOCK), dim3(SET_BLOCK), 0, st, v, N, d_heads.u32());
  FoldValues<PLANES> vals;
  for (uint32_t j = 0; j < PLANES; j++) vals.v[j] = (const uint4*)(d_block.u32() + at_vals + (size_t)j * 4 * N);
  Node* in = d_a.as<Node>();
  Node* out = d_b.as<Node>();
  hipLaunchKernelGGL(k_batch_cells<PLANES>, blocks_for(N, SET_BLOCK), dim3(SET_BLOCK), 0, st, vals, v, N, in, d_dev);
  for (uint32_t k = 0; k < bp.k_tail; k++) {
    const uint32_t n_out = bp.steps[k + 1].n_nodes;
    hipLaunchKernelGGL(k_batch_level<PLANES>, blocks_for(n_out, SET_BLOCK), dim3(SET_BLOCK), 0, st, v, (const Node*)in, k, n_out, out, d_dev);
    std::swap(in, out);
  }
  hipLaunchKernelGGL(k_batch_tail<PLANES>, dim3(B), dim3(SET_TAIL), 0, st, v, (const Node*)in, bp.k_tail, d_dev);
  CM_HIP(hipGetLastError());
  static_assert((size_t)BATCH_WORDS * 4 * BATCH_MAX_PARTS <= TREE_LAND_BYTES, "the parts' words come back in one trip");
  const uint32_t* const land = (const uint32_t*)stage_download_async(d_dev, (size_t)BATCH_WORDS * 4 * B, st);
  CM_HIP(hipStreamSynchronize(st));
  for (uint32_t b = 0; b < B; b++) {
    const uint32_t i = bp.part[b];
    ok[i] = land[BATCH_WORDS * b + BATCH_VERDICT] == 1 ? 1 : 0;
    for (uint32_t j = 0; computed && j < PLANES; j++) computed[(size_t)PLANES * i + j] = land[BATCH_WORDS * b + BATCH_ROOT + j];
  }
}

// the refusals of the arguments alone, in the header's order, for either kind of view
template <class View>
void batch_check_arguments(const char* who, const View* parts, uint32_t n_parts, const uint8_t* ok, const char* view_name) {
  const std::string head = std::string(who) + ": ";
  CM_CHECK(parts && ok, head + "null argument");
  CM_CHECK(n_parts >= 1 && n_parts <= BATCH_MAX_PARTS, head + "no parts, or more than 2^16 parts in one call: verify in groups");
  uint64_t cells = 0;
  for (uint32_t i = 0; i < n_parts; i++) {
    const View& p = parts[i];
    const std::string part = head + "part " + std::to_string(i);
    CM_CHECK(p.struct_size >= sizeof(View), part + ": struct_size does not cover " + view_name + " (set it to sizeof(" + view_name + "))");
    bool arrays = p.n == 0 || p.addresses;
    if constexpr (std::is_same<View, cm_mem_transition_view>::value) arrays = arrays && (p.n == 0 || (p.old_values && p.new_values));
    else arrays = arrays && (p.n == 0 || p.values);
    CM_CHECK(arrays && (p.n_siblings == 0 || p.siblings), part + ": null array");
    CM_CHECK(p.n <= SET_MAX_CELLS, part + ": more than 2^20 cells: split the set");
    cells += p.n;
  }
  CM_CHECK(cells <= SET_MAX_CELLS, head + "the parts hold " + std::to_string(cells) + " cells, more than 2^20 in one call: verify in groups");
}

template <uint32_t PLANES>
void verify_batch(const std::vector<HostPart<PLANES>>& parts, uint8_t* ok, uint32_t* computed, hipStream_t st) {
  const uint32_t n_parts = (uint32_t)parts.size();
  std::vector<const uint32_t*> addrs(n_parts);
  std::vector<uint32_t> n(n_parts), m(n_parts);
  for (uint32_t i = 0; i < n_parts; i++) { addrs[i] = parts[i].a; n[i] = parts[i].n; m[i] = parts[i].m; }
  BatchPlan bp;
  batch_plan(addrs.data(), n.data(), m.data(), n_parts, bp);
  verify_batch_device<PLANES>(bp, parts, ok, computed, st);
}

}  // namespace
}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_verify_memory_transitions(const cm_mem_transition_view* parts, uint32_t n_parts, uint8_t* ok, uint32_t* computed, cm_stream_t s) {
  return cm::abi_guard([&] {
    cm::batch_check_arguments("cm_verify_memory_transitions", parts, n_parts, ok, "cm_mem_transition_view");
    cm::open_require_device("cm_verify_memory_transitions");
    std::vector<cm::HostPart<2>> hp(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) {
      const cm_mem_transition_view& p = parts[i];
      hp[i] = cm::HostPart<2>{p.addresses, {p.old_values, p.new_values}, p.siblings, p.n, p.n_siblings, {p.root_before, p.root_after}};
      // the verdicts that need no GPU: a part without cells is well formed without words, and then the memory after is the memory
      // before; every other part is rejected until the fold says otherwise
      const bool still = p.n == 0 && p.n_siblings == 0;
      ok[i] = (still && p.root_before == p.root_after) ? 1 : 0;
      if (computed) computed[2 * (size_t)i] = computed[2 * (size_t)i + 1] = still ? p.root_before : 0u;
    }
    cm::bind_thread_to_library_device();
    cm::verify_batch<2>(hp, ok, computed, cm::stream_or_own(s));
  });
}
int32_t cm_verify_memory_sets(const cm_mem_set_view* parts, uint32_t n_parts, uint8_t* ok, uint32_t* computed, cm_stream_t s) {
  return cm::abi_guard([&] {
    cm::batch_check_arguments("cm_verify_memory_sets", parts, n_parts, ok, "cm_mem_set_view");
    cm::open_require_device("cm_verify_memory_sets");
    std::vector<cm::HostPart<1>> hp(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) {
      const cm_mem_set_view& p = parts[i];
      hp[i] = cm::HostPart<1>{p.addresses, {p.values}, p.siblings, p.n, p.n_siblings, {p.root}};
      ok[i] = 0;
      if (computed) computed[i] = 0;
    }
    cm::bind_thread_to_library_device();
    cm::verify_batch<1>(hp, ok, computed, cm::stream_or_own(s));
  });
}
// host code: no device call on this path
int32_t cm_mem_batch_plan(const uint32_t* const* addresses, const uint32_t* n, uint32_t n_parts, cm_mem_batch_step* steps, uint32_t cap, uint32_t* n_steps) {
  return cm::abi_guard([&] {
    const std::string head = "cm_mem_batch_plan: ";
    CM_CHECK(addresses && n && n_steps && (steps || cap == 0), head + "null argument");
    CM_CHECK(n_parts >= 1 && n_parts <= cm::BATCH_MAX_PARTS, head + "no parts, or more than 2^16 parts in one call: verify in groups");
    uint64_t cells = 0;
    for (uint32_t i = 0; i < n_parts; i++) {
      CM_CHECK(n[i] == 0 || addresses[i], head + "part " + std::to_string(i) + ": null array");
      CM_CHECK(n[i] <= cm::SET_MAX_CELLS, head + "part " + std::to_string(i) + ": more than 2^20 cells: split the set");
      cells += n[i];
    }
    CM_CHECK(cells <= cm::SET_MAX_CELLS, head + "the parts hold " + std::to_string(cells) + " cells, more than 2^20 in one call: verify in groups");
    cm::BatchPlan bp;
    cm::batch_plan(addresses, n, nullptr, n_parts, bp);
    *n_steps = (uint32_t)bp.steps.size();
    CM_CHECK(cap >= bp.steps.size(), head + "output buffer too small (" + std::to_string(bp.steps.size()) + " steps)");
    for (size_t i = 0; i < bp.steps.size(); i++) steps[i] = bp.steps[i];
  });
}
}  // extern "C"
