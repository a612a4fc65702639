// Memory openings (cm_input_open_memory, cm_run_open_memory, cm_verify_memory_openings, cm_verify_memory_opening): the value of a
// cell and its authentication path under a 31-bit Poseidon2 memory root, built on the GPU from a partial Merkle tree's node list,
// checked in batches on the GPU and one at a time in host code.
//
// The tree (adapter/merkle.rs:183-295) has height 30.  Cell a < 2^28 owns the leaves 4a .. 4a + 3 = the four words of its value;
// h29_0 = H(v0, v1), h29_1 = H(v2, v3), n28 = H(h29_0, h29_1) is the node of depth 28 with index a.  Above it the path has one
// sibling per depth 28 .. 1; at depth d the path's node has index a >> (28 - d) and is the right child when that index is odd.
// A node the list does not hold is the default hash of its depth (default[30] = 0, default[d] = H(default[d + 1], default[d + 1])),
// so an absent cell opens as the value (0, 0, 0, 0) and a present cell holding zeros hashes exactly like an absent one (link.hip).
// Multiplicities enter no hash.
//
// A node record (cm_merkle_node) of depth d holds BOTH children of one parent: index = the left child's index at depth d (even),
// left_value / right_value = the two nodes of depth d, an absent one already replaced by default[d].  The list is ordered by depth
// 30 .. 1, then by ascending index (host_adapter.hpp and partial_merkle_tree_enqueue agree), so:
//   k_open_depth_offsets  31 lanes: off[j] = the number of records deeper than 30 - j, by bisection over the depth words; the
//                         records of depth d are [off[30 - d], off[31 - d]).  Stays on the device.
//   k_open_paths          32 lanes per query.  Lane k < 28 bisects depth 28 - k's slice for the pair (a >> k) & ~1 and takes the
//                         half the path does not pass through, or default[28 - k]; lanes 28 and 29 bisect depth 30 for the pairs
//                         4a and 4a + 2: value[4] and `present`.  Every lane stores its own words of the 34-word record: no atomic,
//                         any order and any repetition of the addresses, the same bytes every time.
//   k_verify_openings     one lane per opening: 31 Poseidon2 calls in a row (the two pairs of the cell, their parent, 28 levels),
//                         ok[i] = well formed and the recomputed root is the expected one.  The chain is serial; the batch is the
//                         parallelism.
//   k_image_leaves        one lane per cell of a run's image: its four leaves, `hi` reversed into ascending address order.
#include "../../include/cairom_hip.h"
#include "mem_open.hpp"
#include "mem_tree.hpp"
#include "segment_input.hpp"
#include "handles.hpp"
#include "host_adapter.hpp"
#include <cstring>
#include <string>

namespace cm {
namespace {

constexpr uint32_t OPEN_BLOCK = 256, OPEN_LANES = 32, OPEN_WORDS = 34, OPEN_SIBLINGS = 28, NODE_WORDS = 8;
constexpr uint32_t ADDRESS_SPACE = host::MAX_ADDRESS + 1;   // 2^28
constexpr uint64_t OPEN_MAX_BATCH = 1ull << 26;             // 32 lanes per query stay below 2^32 threads
constexpr uint32_t VERIFY_BLOCK = 64;                        // one wave per block: a small batch still spreads over the CUs
// record words: 0 address, 1 present, 2..5 value, 6..33 siblings (siblings[k] = the sibling at depth 28 - k)
enum : uint32_t { OW_ADDRESS = 0, OW_PRESENT = 1, OW_VALUE = 2, OW_SIBLINGS = 6 };

static_assert(sizeof(cm_mem_opening) == 4 * OPEN_WORDS && sizeof(cm_merkle_node) == 4 * NODE_WORDS, "plain words, sizes as the header states them");
static_assert(air::TREE_HEIGHT == 30 && ADDRESS_SPACE == (1u << 28), "a cell is four leaves of a tree of height 30");

// ---- one opening, host and device ------------------------------------------------------------------------------------------
// 0 = well formed; 1 address, 2 present, 3 + i value word i, 7 + k sibling k, 35 = absent with a non-zero value
CM_HD uint32_t opening_malformed(const uint32_t* w) {
  if (w[OW_ADDRESS] >= ADDRESS_SPACE) return 1;
  if (w[OW_PRESENT] > 1) return 2;
  for (uint32_t i = 0; i < 4 + OPEN_SIBLINGS; i++)
    if (w[OW_VALUE + i] >= P) return 3 + i;
  if (!w[OW_PRESENT] && (w[OW_VALUE] | w[OW_VALUE + 1] | w[OW_VALUE + 2] | w[OW_VALUE + 3])) return 35;
  return 0;
}
// the root a well-formed record hashes to (one call site of the permutation: the loop is not unrolled)
CM_HD uint32_t opening_root(const uint32_t* w) {
  const uint32_t a = w[OW_ADDRESS];
  uint32_t h = 0, h29_0 = 0;
#pragma unroll 1
  for (uint32_t i = 0; i < 3 + OPEN_SIBLINGS; i++) {
    uint32_t l, r;
    if (i == 0) { l = w[OW_VALUE]; r = w[OW_VALUE + 1]; }
    else if (i == 1) { h29_0 = h; l = w[OW_VALUE + 2]; r = w[OW_VALUE + 3]; }
    else if (i == 2) { l = h29_0; r = h; }
    else {
      const uint32_t k = i - 3, s = w[OW_SIBLINGS + k];
      const bool right = (a >> k) & 1u;   // the path's node at depth 28 - k has index a >> k
      l = right ? s : h; r = right ? h : s;
    }
    h = host::poseidon2_hash(l, r);
  }
  return h;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
k_open_depth_offsets(const uint32_t* __restrict__ nodes, uint32_t n_nodes, uint32_t* __restrict__ off) {
  const uint32_t j = threadIdx.x;
  if (blockIdx.x || j > air::TREE_HEIGHT) return;
  const uint32_t floor_depth = air::TREE_HEIGHT - j;   // records with depth > floor_depth come first
  uint32_t lo = 0, hi = n_nodes;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (nodes[NODE_WORDS * (size_t)mid + 1] > floor_depth) lo = mid + 1; else hi = mid;
  }
  off[j] = lo;
}

__global__ void __launch_bounds__(OPEN_BLOCK)
k_open_paths(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ addresses, uint32_t n,
             TreeDefaults dflt, uint32_t* __restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * OPEN_BLOCK + threadIdx.x;
  const uint32_t q = (uint32_t)(t / OPEN_LANES), slot = (uint32_t)(t % OPEN_LANES);
  if (q >= n || slot >= OPEN_SIBLINGS + 2) return;
  const uint32_t a = addresses[q];
  const bool cell = slot >= OPEN_SIBLINGS;
  const uint32_t depth = cell ? air::TREE_HEIGHT : OPEN_SIBLINGS - slot;
  const uint32_t index = cell ? 4u * a + 2u * (slot - OPEN_SIBLINGS) : (a >> slot) & ~1u;
  const uint32_t end = off[air::TREE_HEIGHT + 1 - depth];
  uint32_t lo = off[air::TREE_HEIGHT - depth], hi = end;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (nodes[NODE_WORDS * (size_t)mid] < index) lo = mid + 1; else hi = mid;
  }
  const uint32_t* const nd = nodes + NODE_WORDS * (size_t)lo;
  const bool found = lo < end && nd[0] == index;
  uint32_t* const o = out + OPEN_WORDS * (size_t)q;
  if (!cell) {
    // the path's node is the right child when its index is odd: the sibling is the other half of the pair
    o[OW_SIBLINGS + slot] = found ? (((a >> slot) & 1u) ? nd[2] : nd[3]) : dflt.h[depth];
  } else {
    const uint32_t half = slot - OPEN_SIBLINGS;
    if (half == 0) { o[OW_ADDRESS] = a; o[OW_PRESENT] = found ? 1u : 0u; }
    o[OW_VALUE + 2 * half] = found ? nd[2] : 0u;
    o[OW_VALUE + 2 * half + 1] = found ? nd[3] : 0u;
  }
}

__global__ void __launch_bounds__(VERIFY_BLOCK)
k_verify_openings(const uint32_t* __restrict__ recs, uint32_t n, uint32_t root, uint8_t* __restrict__ ok) {
  const uint32_t i = blockIdx.x * VERIFY_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t* const w = recs + OPEN_WORDS * (size_t)i;
  ok[i] = (opening_malformed(w) == 0 && opening_root(w) == root) ? 1 : 0;
}

__global__ void __launch_bounds__(OPEN_BLOCK)
k_image_leaves(const uint4* __restrict__ lo, uint32_t n_lo, const uint4* __restrict__ hi, uint32_t n_hi, uint4* __restrict__ idx,
               uint4* __restrict__ val, uint4* __restrict__ mult) {
  const uint32_t t = blockIdx.x * OPEN_BLOCK + threadIdx.x;
  if (t >= n_lo + n_hi) return;
  // row t of the image in ascending address: the locals as they lie, then the heap from its lowest address (= its last index)
  const uint32_t j = t - n_lo;
  const uint32_t a = t < n_lo ? t : ADDRESS_SPACE - n_hi + j;
  const uint4 v = t < n_lo ? lo[t] : hi[n_hi - 1 - j];
  idx[t] = make_uint4(4u * a, 4u * a + 1, 4u * a + 2, 4u * a + 3);
  val[t] = v;
  mult[t] = make_uint4(1u, 1u, 1u, 1u);
}

}  // namespace

void open_require_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    throw CmError(3, std::string(who) + ": no HIP device available (libcairom_hip has no CPU fallback)");
}
void open_check_addresses(const char* who, const uint32_t* addresses, uint64_t n, const cm_mem_opening* out) {
  CM_CHECK(n == 0 || (addresses && out), std::string(who) + ": null addresses or null output");
  CM_CHECK(n <= OPEN_MAX_BATCH, std::string(who) + ": more than 2^26 addresses in one call: split it");
  for (uint64_t i = 0; i < n; i++)
    CM_CHECK(addresses[i] < ADDRESS_SPACE, std::string(who) + ": address " + std::to_string(addresses[i]) + " (query " + std::to_string(i) +
                                               ") is beyond the address space of 2^28 cells");
}

void open_depth_offsets_enqueue(const cm_merkle_node* nodes, uint64_t n_nodes, uint32_t* off, hipStream_t st) {
  CM_CHECK(n_nodes < (1ull << 32), "memory openings: the tree is too large");
  hipLaunchKernelGGL(k_open_depth_offsets, dim3(1), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(nodes), (uint32_t)n_nodes, off);
  CM_HIP(hipGetLastError());
}

void image_leaves_enqueue(const uint32_t* lo, uint32_t n_lo, const uint32_t* hi, uint32_t n_hi, uint32_t* idx, uint32_t* val, uint32_t* mult,
                          hipStream_t st) {
  const uint64_t cells = (uint64_t)n_lo + n_hi;
  CM_CHECK(cells > 0 && cells <= ADDRESS_SPACE, "image leaves: no cells, or more than the address space");
  hipLaunchKernelGGL(k_image_leaves, blocks_for(cells, OPEN_BLOCK), dim3(OPEN_BLOCK), 0, st, reinterpret_cast<const uint4*>(lo), n_lo,
                     reinterpret_cast<const uint4*>(hi), n_hi, reinterpret_cast<uint4*>(idx), reinterpret_cast<uint4*>(val), reinterpret_cast<uint4*>(mult));
  CM_HIP(hipGetLastError());
}

void open_paths(const cm_merkle_node* nodes, uint64_t n_nodes, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, hipStream_t st) {
  if (!n) return;
  CM_CHECK(n <= OPEN_MAX_BATCH && n_nodes < (1ull << 32), "memory openings: the batch or the tree is too large");
  const TreeDefaults dflt = tree_defaults();
  DevBuf d_addr(n * 4), d_off((air::TREE_HEIGHT + 1) * 4), d_out(n * sizeof(cm_mem_opening));
  stage_upload(d_addr.p, addresses, n * 4, st);
  hipLaunchKernelGGL(k_open_depth_offsets, dim3(1), dim3(64), 0, st, reinterpret_cast<const uint32_t*>(nodes), (uint32_t)n_nodes, d_off.u32());
  hipLaunchKernelGGL(k_open_paths, blocks_for(n * OPEN_LANES, OPEN_BLOCK), dim3(OPEN_BLOCK), 0, st, reinterpret_cast<const uint32_t*>(nodes),
                     (const uint32_t*)d_off.u32(), (const uint32_t*)d_addr.u32(), (uint32_t)n, dflt, d_out.u32());
  CM_HIP(hipGetLastError());
  const void* land = stage_download_async(d_out.p, n * sizeof(cm_mem_opening), st);
  CM_HIP(hipStreamSynchronize(st));   // the call's one round trip (also keeps the temporaries alive until the kernels have run)
  memcpy(out, land, n * sizeof(cm_mem_opening));
}

void verify_openings_device(uint32_t root, const cm_mem_opening* openings, uint64_t n, uint8_t* ok, hipStream_t st) {
  if (!n) return;
  DevBuf d_recs(n * sizeof(cm_mem_opening)), d_ok(n);
  stage_upload(d_recs.p, openings, n * sizeof(cm_mem_opening), st);
  hipLaunchKernelGGL(k_verify_openings, blocks_for(n, VERIFY_BLOCK), dim3(VERIFY_BLOCK), 0, st, (const uint32_t*)d_recs.u32(), (uint32_t)n, root,
                     d_ok.as<uint8_t>());
  CM_HIP(hipGetLastError());
  const void* land = stage_download_async(d_ok.p, n, st);
  CM_HIP(hipStreamSynchronize(st));
  memcpy(ok, land, n);
}

}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_input_open_memory(const cm_device_input* in, uint32_t which, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_input_open_memory");
    CM_CHECK(in && in->d && root, "cm_input_open_memory: null argument");
    CM_CHECK(which <= 1, "cm_input_open_memory: `which` is not 0 (the initial tree) or 1 (the final tree)");
    cm::open_check_addresses("cm_input_open_memory", addresses, n, out);
    const cm::DeviceInput& d = *in->d;
    cm::bind_thread_to_library_device();
    *root = which ? d.meta.final_root : d.meta.initial_root;
    cm::open_paths((which ? d.fin_tree : d.init_tree).as<cm_merkle_node>(), which ? d.meta.n_final_tree : d.meta.n_initial_tree, addresses, n, out,
                   cm::thread_main_stream());
  });
}
int32_t cm_verify_memory_openings(uint32_t root, const cm_mem_opening* openings, uint64_t n, uint8_t* ok, cm_stream_t s) {
  return cm::abi_guard([&] {
    cm::open_require_device("cm_verify_memory_openings");
    CM_CHECK(n == 0 || (openings && ok), "cm_verify_memory_openings: null openings or null ok");
    CM_CHECK(n <= cm::OPEN_MAX_BATCH, "cm_verify_memory_openings: more than 2^26 openings in one call: split it");
    cm::bind_thread_to_library_device();
    cm::verify_openings_device(root, openings, n, ok, cm::stream_or_own(s));
  });
}
// host code: no device call on this path
int32_t cm_verify_memory_opening(uint32_t root, const cm_mem_opening* opening) {
  return cm::abi_guard([&]() -> int32_t {
    if (!opening) return cm_set_last_error("cm_verify_memory_opening: null opening");
    const uint32_t* const w = reinterpret_cast<const uint32_t*>(opening);
    const std::string who = "memory opening of address " + std::to_string(w[cm::OW_ADDRESS]) + ": ";
    std::string why;
    const uint32_t bad = cm::opening_malformed(w);
    if (bad == 1) why = "the address is beyond the address space of 2^28 cells";
    else if (bad == 2) why = "present is " + std::to_string(w[cm::OW_PRESENT]) + ", not 0 or 1";
    else if (bad >= 3 && bad < 7) why = "value word " + std::to_string(bad - 3) + " is not below P (depth 30)";
    else if (bad >= 7 && bad < 35) why = "the sibling at depth " + std::to_string(cm::OPEN_SIBLINGS - (bad - 7)) + " is not below P";
    else if (bad == 35) why = "an absent cell with a non-zero value (depth 30)";
    else {
      const uint32_t got = cm::opening_root(w);
      if (got == root) return 0;
      why = "the path hashes to root " + std::to_string(got) + ", not " + std::to_string(root);
    }
    cm_set_last_error((who + why).c_str());
    return 11;
  });
}
}  // extern "C"
