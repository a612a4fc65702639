// Followed memory (cm_mem_image_*): a memory image with its partial Merkle tree, resident on the GPU (or, device == 0, in host
// memory) and independent of any prover handle.  It absorbs a segment's writes by re-hashing only the dirty paths, checks itself
// against the proof's roots, serves the three kinds of opening under its current root and re-emits a full transition for light
// clients from a bare update (addresses and new values).
//
// The handle holds ONE node list of cm_merkle_node records in the order every opener reads (mem_open.hip): depth 30 .. 1, ascending
// index inside a depth.  The cells are its depth-30 slice: a held cell a owns the records 4a and 4a + 2 there (its four value
// words) and the record 2a of depth 29, so cell c of the image is records 2c and 2c + 1 of the list and no second store is kept.
//
// The update is the set fold (mem_set.hpp) with each sibling word taken from the image's own tree.  With S_k the distinct
// a[i] >> k, the dirty nodes of depth 28 - k are exactly S_k and the dirty pair records of that depth are one per node of S_{k+1}:
//   k_img_check      one lane per cell half: the current value (range_find in the depth-30 slice, zeros when absent), compared with
//                    old_values when given; the lowest differing cell by atomicMin (a minimum: no order decides it).
//   k_img_cells      one lane per cell: the two depth-30 records and the depth-29 record from the new value alone, three hashes.
// then the shared ladder of set_fold.hpp with the image's policy, ImageFold:
//   k_fold_level     one lane per PARENT of S_{k+1} while S_k is wider than SET_TAIL: set_parent's index arithmetic; a child in S_k
//                    takes its new hash from the level below, a child that is not takes the old tree's word (range_find of the old
//                    record of that pair, or the depth's default hash); the dirty record of depth 28 - k and the parent's hash.
//   k_fold_tail      one workgroup: the remaining depths in LDS with a barrier between them; the depth-1 record's parent is the root.
// The steps, their widths and the kernel choice are cm_mem_set_plan's for the same addresses.  The commit:
//   k_img_rank       one lane per dirty record: its bisection rank in the old slice of its depth and whether it is an insert;
//   ExclusiveSum     of the insert flags, in node-list order;
//   k_img_merge      one lane per old and per dirty record into a NEW buffer: an old record moves up by the inserts in front of it
//                    (and is dropped where a dirty record replaces it), a dirty record lands at its rank plus the inserts in front;
//   k_img_offsets    the depth offsets of the new list from the old ones and the scan.
// Everything is enqueued before the call's one round trip (the lowest mismatch, the root, the new offsets); the handle swaps
// buffers only when every check passed, so a refused update leaves the image byte-identical.  The number of launches does not
// depend on the image size, and on n only through the plan's per-level steps.  Every word is written by exactly one lane.
// Temporaries: the set verifier's flags, scan and heads (mem_set.hip), 32 bytes per dirty record (3 n + sum |S_{k+1}|) plus 12 of
// ranks and scan, and the new node list.
// Host images run the same fold in plain C++ (host_update, host_merge): same roots, same node words, same statuses and messages.
#include "../../include/cairom_hip.h"
#include "mem_transition.hpp"
#include "mem_batch.hpp"
#include "kprof.hpp"
#include "set_fold.hpp"
#include "mem_open.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace cm {
namespace {

constexpr uint32_t IMG_MAX_CELLS = 1u << 22;    // cm_mem_image_create: the builder's transient block is 3840 bytes per cell (15 GiB)
constexpr uint32_t IMG_MAX_READ = 1u << 24;     // cm_mem_image_read: one call
constexpr uint32_t NO_CELL = 0xffffffffu;
constexpr uint32_t IMG_SLICES = air::TREE_HEIGHT;   // one slice of the node list per depth 30 .. 1
// device words of one update, and of the handle: the lowest cell whose old value differs, the new root, then the depth offsets
// off[j], j = 0 .. 30, of the (new) node list as k_open_depth_offsets defines them
enum : uint32_t { IW_MISMATCH = 0, IW_ROOT = 1, IW_OFF = 4, IMG_DEV_WORDS = IW_OFF + IMG_SLICES + 2 };

static_assert(sizeof(cm_merkle_node) == 32 && RANGE_NODE_WORDS == 8, "a node record is two uint4");
static_assert(sizeof(cm_mem_image_stats) == 32, "size as the header states it");

// the dirty records of depth 30 - q are D[o[q], o[q + 1]), q = 0 .. 29, in node-list order; o[30] = their number
struct ImgSlices { uint32_t o[IMG_SLICES + 2]; };

inline ImgSlices slices_of(const cm_mem_set_step steps[SET_STEPS], uint32_t n) {
  ImgSlices s;
  s.o[0] = 0; s.o[1] = 2 * n; s.o[2] = 3 * n;
  for (uint32_t k = 0; k < SET_DEPTHS; k++) s.o[3 + k] = s.o[2 + k] + steps[k + 1].n_nodes;
  s.o[IMG_SLICES + 1] = s.o[IMG_SLICES];
  return s;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void put_node(uint4* __restrict__ d, uint32_t j, uint32_t index, uint32_t depth, uint32_t l, uint32_t r, uint32_t p,
                                         uint32_t lm, uint32_t rm) {
  d[2 * (size_t)j] = make_uint4(index, depth, l, r);
  d[2 * (size_t)j + 1] = make_uint4(p, lm, rm, 1u);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_img_check(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a, uint32_t n,
            const uint32_t* __restrict__ old_values, uint32_t* __restrict__ cur, uint32_t* __restrict__ dev) {
  const uint32_t u = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (u >= 2u * n) return;
  set_gather_half(nodes, off, a, u, cur);
  if (old_values && (old_values[2 * (size_t)u] != cur[2 * (size_t)u] || old_values[2 * (size_t)u + 1] != cur[2 * (size_t)u + 1]))
    atomicMin(dev + IW_MISMATCH, u >> 1);
}

// values[2 u], values[2 u + 1] = half u & 1 of cell a[u / 2], any order and any repetition of the addresses
__global__ void __launch_bounds__(SET_BLOCK)
k_img_read(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a, uint32_t n, uint32_t* __restrict__ values) {
  const uint32_t u = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (u < 2u * n) set_gather_half(nodes, off, a, u, values);
}

// the four leaves of every cell for the device tree builder, as k_image_leaves
__global__ void __launch_bounds__(SET_BLOCK)
k_img_leaves(const uint32_t* __restrict__ a, const uint4* __restrict__ values, uint32_t n, uint4* __restrict__ idx, uint4* __restrict__ val,
             uint4* __restrict__ mult) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint32_t x = 4u * a[t];
  idx[t] = make_uint4(x, x + 1, x + 2, x + 3);
  val[t] = values[t];
  mult[t] = make_uint4(1u, 1u, 1u, 1u);
}

// Cell t of an update of n cells, address x and new value q: its three records into the update's dirty slice, its node of depth 28
// returned.  One call site of the permutation: the loop is not unrolled (range_cell_node's shape, with the records stored on the way)
__device__ __forceinline__ uint32_t img_cell_records(uint32_t x, uint4 q, uint32_t t, uint32_t n, uint4* __restrict__ dirty) {
  uint32_t h = 0, h29_0 = 0;
#pragma unroll 1
  for (uint32_t i = 0; i < 3; i++) {
    const uint32_t l = i == 0 ? q.x : i == 1 ? q.z : h29_0;
    const uint32_t r = i == 0 ? q.y : i == 1 ? q.w : h;
    if (i == 1) h29_0 = h;
    h = host::poseidon2_hash(l, r);
    if (i < 2) put_node(dirty, 2 * t + i, 4u * x + 2u * i, air::TREE_HEIGHT, l, r, h, 1u, 1u);
    else put_node(dirty, 2 * n + t, 2u * x, air::TREE_HEIGHT - 1, l, r, h, 1u, 1u);
  }
  return h;
}
__global__ void __launch_bounds__(SET_BLOCK)
k_img_cells(const uint32_t* __restrict__ a, const uint4* __restrict__ new_values, uint32_t n, uint4* __restrict__ dirty, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  out[t] = img_cell_records(a[t], new_values[t], t, n, dirty);
}

// what a hashing lane reads beside the set's view: the old tree and where the dirty records go
struct ImgTree {
  const uint32_t* nodes;
  const uint32_t* off;
  uint4* dirty;
};

// Parent p of S_{k+1} (set_parent's answer), where in[c] = the new hash of node c of S_k: a child that is not in S_k takes the OLD
// tree's word (range_find of the old record of that pair, or the depth's default hash); the dirty record of depth 28 - k goes to
// `slot` of tr.dirty; the parent's hash.  The single update and the batch (one tree per part) hash through this.
__device__ __forceinline__ uint32_t img_parent(const SetParent& p, const uint32_t* in, uint32_t k, const ImgTree& tr, const TreeDefaults& dflt, uint32_t slot) {
  const uint32_t depth = SET_DEPTHS - k, me = in[p.c];
  uint32_t l, rr, lm = 1u, rm = 1u;
  if (p.paired) { l = me; rr = in[p.c + 1]; }
  else {
    const uint32_t empty = dflt.h[depth];   // (read as a value in front of the lookup: merged with nd's loads it would put the policy in scratch)
    const uint32_t* const nd = range_find(tr.nodes, tr.off, depth, p.x & ~1u);
    const uint32_t w = nd ? (p.odd ? nd[2] : nd[3]) : empty, wm = nd ? (p.odd ? nd[5] : nd[6]) : 0u;
    l = p.odd ? w : me; rr = p.odd ? me : w;
    lm = p.odd ? wm : 1u; rm = p.odd ? 1u : wm;
  }
  const uint32_t h = host::poseidon2_hash(l, rr);
  put_node(tr.dirty, slot, p.x & ~1u, depth, l, rr, h, lm, rm);
  return h;
}

// The image's policy of the shared ladder (set_fold.hpp): a node is its new hash; a child that is not in S_k takes the OLD tree's
// word, so no record of sibling words is read and nothing is checked; every parent files the dirty record of its depth.
struct ImageFold {
  using Node = uint32_t;
  static constexpr bool CHECKS = false;
  ImgTree tr;
  TreeDefaults dflt;
  ImgSlices sl;
  // parent r of S_{k+1}, where in[c] = the new hash of node c of S_k: the dirty record of depth 28 - k at slot sl.o[2 + k] + r,
  // the parent's hash
  __device__ __forceinline__ uint32_t parent(const SetView& s, const uint32_t* in, uint32_t k, uint32_t r, bool&) const {
    return img_parent(set_parent(s, k, r), in, k, tr, dflt, sl.o[2 + k] + r);
  }
  __device__ __forceinline__ void finish(uint32_t top, bool, uint32_t* dev) const { dev[IW_ROOT] = top; }
};

// the slice q of dirty record j: o[q] <= j < o[q + 1]
__device__ __forceinline__ uint32_t img_slice_of(const ImgSlices& sl, uint32_t j) {
  uint32_t q = 0;
#pragma unroll 1
  for (uint32_t i = 1; i < IMG_SLICES; i++) q = sl.o[i] <= j ? i : q;
  return q;
}
// the first record of [lo, hi) of `list` whose index is not below `index`
__device__ __forceinline__ uint32_t img_lower_bound(const uint32_t* __restrict__ list, uint32_t lo, uint32_t hi, uint32_t index) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (list[RANGE_NODE_WORDS * (size_t)mid] < index) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// rank[j] = the old records in front of dirty record j (those of deeper slices and those of its own with a lower index);
// ins[j] = 1 when the old list has no record of that depth and index; ins[n_dirty] = 0 so that the scan ends in the total
__device__ __forceinline__ void img_rank_lane(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ dirty,
                                              const ImgSlices& sl, uint32_t j, uint32_t* __restrict__ rank, uint32_t* __restrict__ ins) {
  if (j == sl.o[IMG_SLICES]) { ins[j] = 0u; return; }
  const uint32_t q = img_slice_of(sl, j), index = dirty[RANGE_NODE_WORDS * (size_t)j], end = off[q + 1];
  const uint32_t lb = img_lower_bound(nodes, off[q], end, index);
  rank[j] = lb;
  ins[j] = (lb < end && nodes[RANGE_NODE_WORDS * (size_t)lb] == index) ? 0u : 1u;
}
__global__ void __launch_bounds__(SET_BLOCK)
k_img_rank(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ dirty, ImgSlices sl, uint32_t* __restrict__ rank,
           uint32_t* __restrict__ ins) {
  const uint32_t j = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (j <= sl.o[IMG_SLICES]) img_rank_lane(nodes, off, dirty, sl, j, rank, ins);
}

// lane t < n_old: old record t, unless a dirty record replaces it; lane n_old + j: dirty record j.  scan[j] = the inserts in front
// of dirty record j, counted from scan0 (a batch scans the records of many updates at once: scan0 = the scan at this update's
// first record).  cap = the records `out` has room for.
__device__ __forceinline__ void img_merge_lane(const uint4* __restrict__ nodes, uint32_t n_old, const uint4* __restrict__ dirty, const ImgSlices& sl,
                                               const uint32_t* __restrict__ rank, const uint32_t* __restrict__ scan, uint32_t scan0, uint32_t cap,
                                               uint4* __restrict__ out, uint32_t t) {
  const uint4* src;
  uint32_t pos;
  if (t < n_old) {
    src = nodes + 2 * (size_t)t;
    const uint4 head = src[0];   // index, depth, left, right
    if (head.y < 1u || head.y > air::TREE_HEIGHT) return;
    const uint32_t q = air::TREE_HEIGHT - head.y, end = sl.o[q + 1];
    const uint32_t lb = img_lower_bound(reinterpret_cast<const uint32_t*>(dirty), sl.o[q], end, head.x);
    if (lb < end && dirty[2 * (size_t)lb].x == head.x) return;
    pos = t + (scan[lb] - scan0);
  } else {
    const uint32_t j = t - n_old;
    src = dirty + 2 * (size_t)j;
    pos = rank[j] + (scan[j] - scan0);
  }
  if (pos >= cap) return;
  out[2 * (size_t)pos] = src[0];
  out[2 * (size_t)pos + 1] = src[1];
}
__global__ void __launch_bounds__(SET_BLOCK)
k_img_merge(const uint4* __restrict__ nodes, uint32_t n_old, const uint4* __restrict__ dirty, ImgSlices sl, const uint32_t* __restrict__ rank,
            const uint32_t* __restrict__ scan, uint32_t cap, uint4* __restrict__ out) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t < n_old + sl.o[IMG_SLICES]) img_merge_lane(nodes, n_old, dirty, sl, rank, scan, 0u, cap, out, t);
}

// the depth offsets of the merged list: every old offset moves up by the inserts of the deeper slices
__global__ void __launch_bounds__(64)
k_img_offsets(const uint32_t* __restrict__ off, ImgSlices sl, const uint32_t* __restrict__ scan, uint32_t* __restrict__ out) {
  const uint32_t q = threadIdx.x;
  if (blockIdx.x || q > IMG_SLICES) return;
  out[q] = off[q] + scan[sl.o[q]];
}

[[noreturn]] void reject(const std::string& why) { throw CmError(11, "memory image: " + why); }

std::string cell_words(const uint32_t* v) {
  return "(" + std::to_string(v[0]) + ", " + std::to_string(v[1]) + ", " + std::to_string(v[2]) + ", " + std::to_string(v[3]) + ")";
}

}  // namespace
}  // namespace cm

// the handle (opaque in the header): one node list, on the device or in host memory, and what the host knows of it
struct cm_mem_image {
  std::mutex mu;   // one call at a time
  bool device = false;
  uint32_t root = 0;
  uint64_t n_nodes = 0;
  uint32_t off[cm::IMG_SLICES + 2] = {0};   // the records of depth d are [off[30 - d], off[31 - d]); off[30] = n_nodes
  std::vector<cm_merkle_node> h_nodes;      // device == 0
  cm::DevBuf d_nodes, d_words;              // device == 1: the list, and IMG_DEV_WORDS words whose IW_OFF part the openers' lookup reads
  uint64_t n_cells() const { return off[1] / 2; }
  const uint32_t* d_off() const { return d_words.u32() + cm::IW_OFF; }
};

namespace cm {
namespace {

// ---- host images ---------------------------------------------------------------------------------------------------------
void host_offsets(cm_mem_image& img) {
  const std::vector<cm_merkle_node>& nd = img.h_nodes;
  for (uint32_t j = 0; j <= IMG_SLICES; j++)
    img.off[j] = (uint32_t)(std::partition_point(nd.begin(), nd.end(), [&](const cm_merkle_node& x) { return x.depth > air::TREE_HEIGHT - j; }) - nd.begin());
  img.n_nodes = nd.size();
}
const cm_merkle_node* host_find(const cm_mem_image& img, uint32_t depth, uint32_t index) {
  const cm_merkle_node* const lo = img.h_nodes.data() + img.off[air::TREE_HEIGHT - depth];
  const cm_merkle_node* const hi = img.h_nodes.data() + img.off[air::TREE_HEIGHT + 1 - depth];
  const cm_merkle_node* const it = std::partition_point(lo, hi, [&](const cm_merkle_node& x) { return x.index < index; });
  return it < hi && it->index == index ? it : nullptr;
}
void host_read(const cm_mem_image& img, const uint32_t* a, uint64_t n, uint32_t* values) {
  for (uint64_t u = 0; u < 2 * n; u++) {
    const cm_merkle_node* const nd = host_find(img, air::TREE_HEIGHT, 4u * a[u >> 1] + 2u * (uint32_t)(u & 1u));
    values[2 * u] = nd ? nd->left_value : 0u;
    values[2 * u + 1] = nd ? nd->right_value : 0u;
  }
}
// the dirty records of an update in node-list order, the sibling words the fold read (a set opening's record under the OLD tree,
// in its canonical order) and the new root: the walk of set_root_host with each word taken from the image's own tree
struct HostUpdate { std::vector<cm_merkle_node> dirty; std::vector<uint32_t> siblings; uint32_t root = 0; };
HostUpdate host_update(const cm_mem_image& img, const uint32_t* a, uint32_t n, const uint32_t* nv) {
  const std::vector<uint32_t>& dflt = host::poseidon2_default_hashes();
  HostUpdate u;
  std::vector<uint32_t> x(a, a + n), h(n), px, ph;
  std::vector<cm_merkle_node> d29(n);
  u.dirty.reserve(4 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t* const v = nv + 4 * (size_t)i;
    const uint32_t h0 = host::poseidon2_hash(v[0], v[1]), h1 = host::poseidon2_hash(v[2], v[3]);
    h[i] = host::poseidon2_hash(h0, h1);
    u.dirty.push_back(cm_merkle_node{4u * a[i], air::TREE_HEIGHT, v[0], v[1], h0, 1u, 1u, 1u});
    u.dirty.push_back(cm_merkle_node{4u * a[i] + 2u, air::TREE_HEIGHT, v[2], v[3], h1, 1u, 1u, 1u});
    d29[i] = cm_merkle_node{2u * a[i], air::TREE_HEIGHT - 1, h0, h1, h[i], 1u, 1u, 1u};
  }
  u.dirty.insert(u.dirty.end(), d29.begin(), d29.end());
  for (uint32_t k = 0; k < SET_DEPTHS; k++) {
    const uint32_t depth = SET_DEPTHS - k;
    px.clear(); ph.clear();
    for (size_t j = 0; j < x.size(); j++) {
      const uint32_t me = x[j];
      uint32_t l, r, lm = 1u, rm = 1u;
      if (!(me & 1u) && j + 1 < x.size() && x[j + 1] == me + 1) { l = h[j]; r = h[j + 1]; j++; }
      else {
        const cm_merkle_node* const nd = host_find(img, depth, me & ~1u);
        const bool odd = me & 1u;
        const uint32_t w = nd ? (odd ? nd->left_value : nd->right_value) : dflt[depth], wm = nd ? (odd ? nd->left_mult : nd->right_mult) : 0u;
        u.siblings.push_back(w);
        l = odd ? w : h[j]; r = odd ? h[j] : w;
        lm = odd ? wm : 1u; rm = odd ? 1u : wm;
      }
      const uint32_t p = host::poseidon2_hash(l, r);
      u.dirty.push_back(cm_merkle_node{me & ~1u, depth, l, r, p, lm, rm, 1u});
      px.push_back(me >> 1);
      ph.push_back(p);
    }
    x.swap(px); h.swap(ph);
  }
  u.root = h[0];
  return u;
}
// both lists are in node-list order; a dirty record replaces the old one of its depth and index
std::vector<cm_merkle_node> host_merge(const std::vector<cm_merkle_node>& old_nodes, const std::vector<cm_merkle_node>& dirty) {
  auto before = [](const cm_merkle_node& x, const cm_merkle_node& y) { return x.depth != y.depth ? x.depth > y.depth : x.index < y.index; };
  std::vector<cm_merkle_node> out;
  out.reserve(old_nodes.size() + dirty.size());
  size_t i = 0, j = 0;
  while (i < old_nodes.size() || j < dirty.size()) {
    if (j == dirty.size() || (i < old_nodes.size() && before(old_nodes[i], dirty[j]))) out.push_back(old_nodes[i++]);
    else {
      if (i < old_nodes.size() && !before(dirty[j], old_nodes[i])) i++;
      out.push_back(dirty[j++]);
    }
  }
  return out;
}

// ---- device images -------------------------------------------------------------------------------------------------------
void device_create(cm_mem_image& img, const uint32_t* a, const uint32_t* values, uint32_t n) {
  bind_thread_to_library_device();
  const hipStream_t st = thread_main_stream();
  img.d_words.alloc(IMG_DEV_WORDS * 4);
  const StreamWait wait{st};
  if (n) {
    DevBuf d_addr((size_t)n * 4), d_vals((size_t)n * 16);
    stage_upload(d_addr.p, a, (size_t)n * 4, st);
    stage_upload(d_vals.p, values, (size_t)n * 16, st);
    leaves_tree_build(n, [&](uint32_t* idx, uint32_t* val, uint32_t* mult) {
      hipLaunchKernelGGL(k_img_leaves, blocks_for(n, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint32_t*)d_addr.u32(), (const uint4*)d_vals.as<uint4>(), n,
                         reinterpret_cast<uint4*>(idx), reinterpret_cast<uint4*>(val), reinterpret_cast<uint4*>(mult));
    }, img.d_nodes, img.n_nodes, img.root, st);
  } else {
    img.d_nodes.alloc(4);
    img.n_nodes = 0;
    img.root = host::poseidon2_default_hashes()[0];
  }
  open_depth_offsets_enqueue(img.d_nodes.as<cm_merkle_node>(), img.n_nodes, img.d_words.u32() + IW_OFF, st);
  download(img.off, img.d_off(), (IMG_SLICES + 1) * 4, st);
  CM_CHECK(img.off[IMG_SLICES] == img.n_nodes && img.off[1] == 2ull * n && img.off[2] == 3ull * n, "memory image: the tree does not hold every cell");
}

// what an update leaves for the commit, which is a swap
struct DeviceUpdate {
  DevBuf nodes, words;
  uint32_t off[IMG_SLICES + 2] = {0};
};

// Enqueues the whole update and makes the call's one round trip.  mismatch = the index of the lowest cell whose old value
// differs (NO_CELL when none, or when old_values is NULL), cur4 then its current value; root = the root the image would have.
void device_update(const cm_mem_image& img, const uint32_t* a, uint32_t n, const uint32_t* nv, const uint32_t* ov, const cm_mem_set_step steps[SET_STEPS],
                   DeviceUpdate& up, uint32_t& mismatch, uint32_t cur4[4], uint32_t& root, hipStream_t st) {
  const ImgSlices sl = slices_of(steps, n);
  const uint32_t n_dirty = sl.o[IMG_SLICES], n_old = (uint32_t)img.n_nodes;
  CM_CHECK((uint64_t)n_old + n_dirty < (1ull << 32), "memory image: the tree is too large");
  uint32_t words0[IMG_DEV_WORDS] = {0};
  words0[IW_MISMATCH] = NO_CELL;
  DevBuf d_addr((size_t)n * 4), d_new((size_t)n * 16), d_old, d_cur((size_t)n * 16), d_a((size_t)n * 4), d_b((size_t)n * 4),
      d_dirty((size_t)n_dirty * 32), d_rank((size_t)n_dirty * 4), d_ins(((size_t)n_dirty + 1) * 4), d_scan(((size_t)n_dirty + 1) * 4), tmp_ins;
  SetFold f;
  up.words.alloc(IMG_DEV_WORDS * 4);
  up.nodes.alloc(((size_t)n_old + n_dirty) * 32);
  const StreamWait wait{st};
  stage_upload(up.words.p, words0, sizeof(words0), st);
  stage_upload(d_addr.p, a, (size_t)n * 4, st);
  stage_upload(d_new.p, nv, (size_t)n * 16, st);
  if (ov) { d_old.alloc((size_t)n * 16); stage_upload(d_old.p, ov, (size_t)n * 16, st); }
  const uint32_t* const nodes = img.d_nodes.u32();
  const uint32_t* const off = img.d_off();
  // the cells: the current values against the old ones, and the three self-contained records of every cell
  hipLaunchKernelGGL(k_img_check, blocks_for(2ull * n, SET_BLOCK), dim3(SET_BLOCK), 0, st, nodes, off, (const uint32_t*)d_addr.u32(), n,
                     (const uint32_t*)(ov ? d_old.u32() : nullptr), d_cur.u32(), up.words.u32());
  hipLaunchKernelGGL(k_img_cells, blocks_for(n, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint32_t*)d_addr.u32(), (const uint4*)d_new.as<uint4>(), n, d_dirty.as<uint4>(),
                     d_a.u32());
  // the levels, launched from the plan's records as the set verifier's
  set_fold_prepare(f, d_addr.u32(), n, steps, nullptr, 0, st);
  set_fold_enqueue(f, steps, ImageFold{ImgTree{nodes, off, d_dirty.as<uint4>()}, tree_defaults(), sl}, d_a.u32(), d_b.u32(), up.words.u32(), "memory image", st);
  // the merge into a new list; the handle keeps the old one until every check has passed
  hipLaunchKernelGGL(k_img_rank, blocks_for((uint64_t)n_dirty + 1, SET_BLOCK), dim3(SET_BLOCK), 0, st, nodes, off, (const uint32_t*)d_dirty.u32(), sl, d_rank.u32(), d_ins.u32());
  size_t bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_ins.u32(), d_scan.u32(), (int)(n_dirty + 1), st));
  tmp_ins.alloc(bytes ? bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp_ins.p, bytes, d_ins.u32(), d_scan.u32(), (int)(n_dirty + 1), st));
  hipLaunchKernelGGL(k_img_merge, blocks_for((uint64_t)n_old + n_dirty, SET_BLOCK), dim3(SET_BLOCK), 0, st, (const uint4*)img.d_nodes.as<uint4>(), n_old,
                     (const uint4*)d_dirty.as<uint4>(), sl, (const uint32_t*)d_rank.u32(), (const uint32_t*)d_scan.u32(), n_old + n_dirty, up.nodes.as<uint4>());
  hipLaunchKernelGGL(k_img_offsets, dim3(1), dim3(64), 0, st, off, sl, (const uint32_t*)d_scan.u32(), up.words.u32() + IW_OFF);
  CM_HIP(hipGetLastError());
  uint32_t land[IMG_DEV_WORDS];
  download(land, up.words.p, sizeof(land), st);
  mismatch = land[IW_MISMATCH];
  root = land[IW_ROOT];
  memcpy(up.off, land + IW_OFF, (IMG_SLICES + 1) * 4);
  if (mismatch != NO_CELL) {
    CM_CHECK(mismatch < n, "memory image: the device names a cell outside the update");
    download(cur4, d_cur.u32() + 4 * (size_t)mismatch, 16, st);
  }
  CM_CHECK(up.off[IMG_SLICES] >= n_old && up.off[IMG_SLICES] <= n_old + n_dirty, "memory image: the device counts more records than the merge can make");
}

// ---- what both kinds of image share ----------------------------------------------------------------------------------------
void check_update_addresses(const char* who, const uint32_t* addresses, uint64_t n) {
  CM_CHECK(n > 0, std::string(who) + ": a set of no cells");
  CM_CHECK(n <= SET_MAX_CELLS, std::string(who) + ": more than 2^20 cells in one call: split the set");
  const uint64_t bad = set_first_bad_address(addresses, n);
  CM_CHECK(bad == n, std::string(who) + ": " + set_address_complaint(addresses, bad) + " (" + std::to_string(addresses[bad]) +
                         "): the addresses must be strictly ascending and below 2^28");
}

// The refusals of an update in the header's words, one function per check: the single call and the batch (mem_image_batch.inc) say
// the same.  Checks 2 and 3 read only what the host holds.
void check_new_words(const uint32_t* a, uint32_t n, const uint32_t* nv) {
  for (uint64_t i = 0; i < 4ull * n; i++)
    if (nv[i] >= P) reject("new value word " + std::to_string(i % 4) + " of cell " + std::to_string(a[i / 4]) + " is not below P");
}
void check_root_before(const cm_mem_image& img, const uint32_t* root_before) {
  if (root_before && *root_before != img.root)
    reject("the image is at root " + std::to_string(img.root) + ", the update starts from " + std::to_string(*root_before));
}
[[noreturn]] void old_differs(const uint32_t* a, const uint32_t* ov, uint32_t cell, const uint32_t* cur) {
  reject("cell " + std::to_string(a[cell]) + " holds " + cell_words(cur) + ", the update's old value is " + cell_words(ov + 4 * (size_t)cell));
}
void check_root_after(const uint32_t* root_after, uint32_t root) {
  if (root_after && *root_after != root) reject("the image would hash to root " + std::to_string(root) + ", not " + std::to_string(*root_after));
}

// the checks of cm_mem_image_apply from the second on, in the header's order; the image changes only behind the last of them
void apply_locked(cm_mem_image& img, const uint32_t* a, uint32_t n, const uint32_t* nv, const uint32_t* ov, const uint32_t* root_before,
                  const uint32_t* root_after, uint32_t* root_out, cm_mem_transition** record_out) {
  check_new_words(a, n, nv);
  check_root_before(img, root_before);
  cm_mem_set_step steps[SET_STEPS];
  const uint32_t n_words = mem_set_plan(a, n, steps);
  std::unique_ptr<cm_mem_transition> rec;
  if (record_out) {
    rec.reset(new cm_mem_transition());
    rec->addresses.assign(a, a + n);
    rec->new_values.assign(nv, nv + 4 * (size_t)n);
    rec->old_values.resize(4 * (size_t)n);
    rec->siblings.resize(n_words);
    rec->root_before = img.root;
  }
  if (!img.device) {
    std::vector<uint32_t> cur(4 * (size_t)n);
    host_read(img, a, n, cur.data());
    if (ov)
      for (uint32_t i = 0; i < n; i++)
        if (memcmp(cur.data() + 4 * (size_t)i, ov + 4 * (size_t)i, 16)) old_differs(a, ov, i, cur.data() + 4 * (size_t)i);
    HostUpdate u = host_update(img, a, n, nv);
    check_root_after(root_after, u.root);
    CM_CHECK(u.siblings.size() == n_words, "memory image: the fold read " + std::to_string(u.siblings.size()) + " sibling words where the plan has " +
                                               std::to_string(n_words));
    if (rec) { rec->old_values = cur; rec->siblings = u.siblings; }
    std::vector<cm_merkle_node> merged = host_merge(img.h_nodes, u.dirty);
    img.h_nodes.swap(merged);
    host_offsets(img);
    img.root = u.root;
  } else {
    bind_thread_to_library_device();
    const hipStream_t st = thread_main_stream();
    DeviceUpdate up;
    uint32_t mismatch = NO_CELL, cur4[4] = {0, 0, 0, 0}, root = 0;
    device_update(img, a, n, nv, ov, steps, up, mismatch, cur4, root, st);
    if (mismatch != NO_CELL) old_differs(a, ov, mismatch, cur4);
    check_root_after(root_after, root);
    // the record is read from the tree before the update, through the set opener
    if (rec) open_set(img.d_nodes.as<cm_merkle_node>(), img.n_nodes, a, n, rec->old_values.data(), rec->siblings.data(), n_words, st);
    img.d_nodes = std::move(up.nodes);
    img.d_words = std::move(up.words);
    memcpy(img.off, up.off, sizeof(img.off));
    img.n_nodes = img.off[IMG_SLICES];
    img.root = root;
  }
  *root_out = img.root;
  if (rec) { rec->root_after = img.root; *record_out = rec.release(); }
}

void require_device_image(const cm_mem_image& img, const char* who) {
  CM_CHECK(img.device, std::string(who) + ": a host image serves no openings: create the image with device = 1");
  CM_CHECK(img.n_nodes > 0, std::string(who) + ": the image is empty: there is no tree to open");
}

}  // namespace
}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_mem_image_create(const uint32_t* addresses, const uint32_t* values, uint64_t n, uint32_t device, cm_mem_image** out) {
  return cm::abi_guard([&] {
    if (device == 1) cm::open_require_device("cm_mem_image_create");   // before any argument is looked at
    if (out) *out = nullptr;
    CM_CHECK(device <= 1, "cm_mem_image_create: `device` is not 0 (host memory) or 1 (the GPU)");
    CM_CHECK(out && (n == 0 || (addresses && values)), "cm_mem_image_create: null argument");
    CM_CHECK(n <= cm::IMG_MAX_CELLS, "cm_mem_image_create: more than 2^22 cells in one image");
    const uint64_t bad = cm::set_first_bad_address(addresses, n);
    CM_CHECK(bad == n, "cm_mem_image_create: " + cm::set_address_complaint(addresses, bad) + " (" + std::to_string(addresses[bad]) +
                           "): the addresses must be strictly ascending and below 2^28");
    for (uint64_t i = 0; i < 4 * n; i++)
      CM_CHECK(values[i] < cm::P, "cm_mem_image_create: value word " + std::to_string(i % 4) + " of cell " + std::to_string(addresses[i / 4]) + " is not below P");
    std::unique_ptr<cm_mem_image> img(new cm_mem_image());
    img->device = device == 1;
    if (img->device) cm::device_create(*img, addresses, values, (uint32_t)n);
    else {
      // the update of the empty image by every cell: the fold's own records, all of them inserts
      img->root = cm::host::poseidon2_default_hashes()[0];
      if (n) {
        cm::HostUpdate u = cm::host_update(*img, addresses, (uint32_t)n, values);
        img->h_nodes = cm::host_merge(img->h_nodes, u.dirty);
        img->root = u.root;
      }
      cm::host_offsets(*img);
    }
    *out = img.release();
  });
}
int32_t cm_mem_image_free(cm_mem_image* img) {
  return cm::abi_guard([&] {
    if (!img) return;
    if (img->device) cm::bind_thread_to_library_device();
    delete img;
  });
}
int32_t cm_mem_image_root(cm_mem_image* img, uint32_t* root) {
  return cm::abi_guard([&] {
    CM_CHECK(img && root, "cm_mem_image_root: null argument");
    std::lock_guard<std::mutex> lk(img->mu);
    *root = img->root;
  });
}
int32_t cm_mem_image_stats_get(cm_mem_image* img, cm_mem_image_stats* out) {
  return cm::abi_guard([&] {
    CM_CHECK(img && out, "cm_mem_image_stats_get: null argument");
    CM_CHECK(out->struct_size >= sizeof(cm_mem_image_stats),
             "cm_mem_image_stats_get: struct_size does not cover cm_mem_image_stats (set it to sizeof(cm_mem_image_stats))");
    std::lock_guard<std::mutex> lk(img->mu);
    cm_mem_image_stats s;
    s.struct_size = sizeof(s);
    s.device = img->device ? 1u : 0u;
    s.n_cells = img->n_cells();
    s.n_nodes = img->n_nodes;
    s.bytes = img->device ? cm::pool_round(img->d_nodes.bytes) + cm::pool_round(img->d_words.bytes) : img->h_nodes.capacity() * sizeof(cm_merkle_node);
    memcpy(out, &s, sizeof(s));
  });
}
int32_t cm_mem_image_read(cm_mem_image* img, const uint32_t* addresses, uint64_t n, uint32_t* values) {
  return cm::abi_guard([&] {
    CM_CHECK(img && (n == 0 || (addresses && values)), "cm_mem_image_read: null argument");
    CM_CHECK(n <= cm::IMG_MAX_READ, "cm_mem_image_read: more than 2^24 addresses in one call: split it");
    for (uint64_t i = 0; i < n; i++)
      CM_CHECK(addresses[i] < cm::RANGE_SPACE, "cm_mem_image_read: address " + std::to_string(addresses[i]) + " (query " + std::to_string(i) +
                                                   ") is beyond the address space of 2^28 cells");
    if (!n) return;
    std::lock_guard<std::mutex> lk(img->mu);
    if (!img->device) { cm::host_read(*img, addresses, n, values); return; }
    cm::bind_thread_to_library_device();
    const hipStream_t st = cm::thread_main_stream();
    cm::DevBuf d_addr(n * 4), d_vals(n * 16);
    const cm::StreamWait wait{st};
    cm::stage_upload(d_addr.p, addresses, n * 4, st);
    hipLaunchKernelGGL(cm::k_img_read, cm::blocks_for(2 * n, cm::SET_BLOCK), dim3(cm::SET_BLOCK), 0, st, (const uint32_t*)img->d_nodes.u32(), img->d_off(),
                       (const uint32_t*)d_addr.u32(), (uint32_t)n, d_vals.u32());
    CM_HIP(hipGetLastError());
    cm::download(values, d_vals.p, n * 16, st);
  });
}
int32_t cm_mem_image_nodes(cm_mem_image* img, cm_merkle_node* nodes, uint64_t cap, uint64_t* n_total) {
  return cm::abi_guard([&] {
    CM_CHECK(img && n_total, "cm_mem_image_nodes: null argument");
    CM_CHECK(nodes || cap == 0, "cm_mem_image_nodes: null nodes with a capacity");
    std::lock_guard<std::mutex> lk(img->mu);
    *n_total = img->n_nodes;
    const uint64_t m = std::min(cap, img->n_nodes);
    if (!m) return;
    if (!img->device) { memcpy(nodes, img->h_nodes.data(), m * sizeof(cm_merkle_node)); return; }
    cm::bind_thread_to_library_device();
    cm::download(nodes, img->d_nodes.p, m * sizeof(cm_merkle_node), cm::thread_main_stream());
  });
}
int32_t cm_mem_image_cells(cm_mem_image* img, uint32_t* addresses, uint32_t* values, uint64_t cap, uint64_t* n_total) {
  return cm::abi_guard([&] {
    CM_CHECK(img && n_total, "cm_mem_image_cells: null argument");
    CM_CHECK((addresses && values) || cap == 0, "cm_mem_image_cells: null arrays with a capacity");
    std::lock_guard<std::mutex> lk(img->mu);
    *n_total = img->n_cells();
    const uint64_t m = std::min(cap, img->n_cells());
    if (!m) return;
    // cell c of the image is records 2c and 2c + 1 of the list: the two halves of its value at depth 30
    std::vector<cm_merkle_node> tmp;
    const cm_merkle_node* recs = img->h_nodes.data();
    if (img->device) {
      cm::bind_thread_to_library_device();
      tmp.resize(2 * m);
      cm::download(tmp.data(), img->d_nodes.p, 2 * m * sizeof(cm_merkle_node), cm::thread_main_stream());
      recs = tmp.data();
    }
    for (uint64_t c = 0; c < m; c++) {
      const cm_merkle_node &lo = recs[2 * c], &hi = recs[2 * c + 1];
      CM_CHECK(lo.depth == air::TREE_HEIGHT && hi.depth == air::TREE_HEIGHT && !(lo.index & 3u) && hi.index == lo.index + 2,
               "memory image: the depth-30 slice does not hold two records per cell");
      addresses[c] = lo.index >> 2;
      values[4 * c] = lo.left_value; values[4 * c + 1] = lo.right_value; values[4 * c + 2] = hi.left_value; values[4 * c + 3] = hi.right_value;
    }
  });
}
int32_t cm_mem_image_apply(cm_mem_image* img, const uint32_t* addresses, const uint32_t* new_values, uint64_t n, const uint32_t* old_values,
                           const uint32_t* root_before, const uint32_t* root_after, uint32_t* root_out, cm_mem_transition** record_out) {
  return cm::abi_guard([&] {
    if (record_out) *record_out = nullptr;
    CM_CHECK(img && addresses && new_values && root_out, "cm_mem_image_apply: null argument");
    cm::check_update_addresses("cm_mem_image_apply", addresses, n);
    std::lock_guard<std::mutex> lk(img->mu);
    cm::apply_locked(*img, addresses, (uint32_t)n, new_values, old_values, root_before, root_after, root_out, record_out);
  });
}
int32_t cm_mem_image_apply_transition(cm_mem_image* img, const cm_mem_transition_view* t, cm_mem_transition** record_out) {
  return cm::abi_guard([&] {
    if (record_out) *record_out = nullptr;
    CM_CHECK(img && t, "cm_mem_image_apply_transition: null argument");
    CM_CHECK(t->struct_size >= sizeof(cm_mem_transition_view),
             "cm_mem_image_apply_transition: struct_size does not cover cm_mem_transition_view (set it to sizeof(cm_mem_transition_view))");
    uint32_t root = 0;
    if (t->n) {
      CM_CHECK(t->addresses && t->old_values && t->new_values, "cm_mem_image_apply_transition: null array");
      cm::check_update_addresses("cm_mem_image_apply_transition", t->addresses, t->n);
      std::lock_guard<std::mutex> lk(img->mu);
      cm::apply_locked(*img, t->addresses, t->n, t->new_values, t->old_values, &t->root_before, &t->root_after, &root, record_out);
      return;
    }
    // no cell changes: the roots are still checked, and then the memory after is the memory before
    std::lock_guard<std::mutex> lk(img->mu);
    if (t->root_before != img->root)
      cm::reject("the image is at root " + std::to_string(img->root) + ", the update starts from " + std::to_string(t->root_before));
    if (t->root_after != t->root_before)
      cm::reject("no cell changes, and root " + std::to_string(t->root_before) + " is not root " + std::to_string(t->root_after));
    if (record_out) {
      std::unique_ptr<cm_mem_transition> rec(new cm_mem_transition());
      rec->root_before = rec->root_after = img->root;
      *record_out = rec.release();
    }
  });
}
// The openings: thin calls into the openers of mem_open.hip, mem_range.hip and mem_set.hip over the image's node list; the
// contract of their cm_run_open_* twins.  Device images only.
int32_t cm_mem_image_open_memory(cm_mem_image* img, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    CM_CHECK(img && root, "cm_mem_image_open_memory: null argument");
    cm::open_check_addresses("cm_mem_image_open_memory", addresses, n, out);
    std::lock_guard<std::mutex> lk(img->mu);
    cm::require_device_image(*img, "cm_mem_image_open_memory");
    cm::bind_thread_to_library_device();
    *root = img->root;
    cm::open_paths(img->d_nodes.as<cm_merkle_node>(), img->n_nodes, addresses, n, out, cm::thread_main_stream());
  });
}
int32_t cm_mem_image_open_memory_range(cm_mem_image* img, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out, uint32_t* root) {
  return cm::abi_guard([&] {
    CM_CHECK(img && root, "cm_mem_image_open_memory_range: null argument");
    cm::open_range_check("cm_mem_image_open_memory_range", start, n_cells, values, out);
    std::lock_guard<std::mutex> lk(img->mu);
    cm::require_device_image(*img, "cm_mem_image_open_memory_range");
    cm::bind_thread_to_library_device();
    cm::open_range(img->d_nodes.as<cm_merkle_node>(), img->n_nodes, start, n_cells, values, out, cm::thread_main_stream());
    *root = img->root;
  });
}
int32_t cm_mem_image_open_memory_set(cm_mem_image* img, const uint32_t* addresses, uint64_t n, uint32_t* values, uint32_t* siblings, uint32_t cap_siblings,
                                     uint32_t* n_siblings, uint32_t* root) {
  return cm::abi_guard([&] {
    CM_CHECK(img && root, "cm_mem_image_open_memory_set: null argument");
    cm::open_set_check("cm_mem_image_open_memory_set", addresses, n, values, siblings, cap_siblings, n_siblings);
    std::lock_guard<std::mutex> lk(img->mu);
    cm::require_device_image(*img, "cm_mem_image_open_memory_set");
    cm::bind_thread_to_library_device();
    cm::open_set(img->d_nodes.as<cm_merkle_node>(), img->n_nodes, addresses, (uint32_t)n, values, siblings, *n_siblings, cm::thread_main_stream());
    *root = img->root;
  });
}
}  // extern "C"

// cm_mem_images_apply: many images, one update each, through ONE ladder
#include "mem_image_batch.inc"

// cm_mem_images_open_memory_sets: many sets under many images, one chain of launches and one round trip
#include "mem_image_open_batch.inc"
