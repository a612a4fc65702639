// The set fold (mem_set.hpp), once, for everything that hashes the address set S_k up one depth at a time: the set verifier
// (mem_set.hip), the transition verifier (mem_transition.hip) and the image update (mem_image.hip).  One hashing lane per parent
// while S_k is wider than SET_TAIL (k_fold_level, from one ping-pong buffer into the other), then one workgroup with the level in
// LDS for every remaining depth (k_fold_tail).  What differs between the three is a small policy, passed to the kernels by value:
//   Node                               what a lane keeps per node: one word, an (old, new) pair, ...
//   CHECKS                             whether the fold consumes a record of sibling words: the tail's lane 0 then compares the
//                                      record's length with the count of the addresses' own flags, and a parent that finds its word
//                                      missing or malformed raises dev[FOLD_FLAG] with a plain store (every writer stores 1)
//   parent(view, in, k, r, bad) -> Node   parent r of S_{k+1} from in[c] = node c of S_k, by set_parent's index arithmetic; side
//                                      effects (the image's dirty records) included
//   finish(top, bad, dev)              what lane 0 of the tail does with the top node
// Device code; the kernels and the driver have internal linkage, so every translation unit instantiates its own policies.
#pragma once
#include "mem_set.hpp"
#include <string>
#include <utility>

namespace cm {

// device words of a checking fold: the malformed flag of its hashing kernels; a verifier adds the verdict and, from FOLD_ROOT on,
// one computed root per plane
enum : uint32_t { FOLD_FLAG = 0, FOLD_VERDICT = 1, FOLD_ROOT = 2 };

static_assert(SET_TAIL <= 1024 && SET_TAIL >= 2, "one workgroup holds a level");

// ---- prepare: what every fold needs of the addresses before its first level ----------------------------------------------------
// The flags, their scan and the head lanes of (d_addr, n), the plan's widths and the view the hashing lanes read.  The buffers
// are alive until the stream has been waited for: the struct outlives that wait.
struct CM_INTERNAL SetFold {
  DevBuf flag, scan, tmp, heads;
  SetWidths w;
  SetView view;
};
// enqueues k_set_flags, the scan and k_set_heads on st; `steps` is mem_set_plan's for the same addresses, `words` the record's
// n_words sibling words on the device (nullptr and 0 for a fold that reads none)
CM_INTERNAL void set_fold_prepare(SetFold& f, const uint32_t* d_addr, uint32_t n, const cm_mem_set_step steps[SET_STEPS], const uint32_t* words,
                                  uint32_t n_words, hipStream_t st);

namespace {

// ---- the verifier policy: PLANES folds of values over one set and ONE list of sibling words ------------------------------------
// A node is one word per plane (two planes: 8 bytes, loaded and stored as such).  The sibling word is the same in every plane:
// that is the statement of a transition.
template <uint32_t PLANES> struct FoldPlanes;
template <> struct FoldPlanes<1> { using Node = uint32_t; };
template <> struct FoldPlanes<2> { using Node = uint2; };
__device__ __forceinline__ uint32_t fold_plane(uint32_t v, uint32_t) { return v; }
__device__ __forceinline__ uint32_t fold_plane(uint2 v, uint32_t j) { return j ? v.y : v.x; }
__device__ __forceinline__ void fold_splat(uint32_t w, uint32_t& out) { out = w; }
__device__ __forceinline__ void fold_splat(uint32_t w, uint2& out) { out = make_uint2(w, w); }
__device__ __forceinline__ uint32_t fold_hash(uint32_t l, uint32_t r) { return host::poseidon2_hash(l, r); }
__device__ __forceinline__ uint2 fold_hash(uint2 l, uint2 r) { return make_uint2(host::poseidon2_hash(l.x, r.x), host::poseidon2_hash(l.y, r.y)); }

template <uint32_t PLANES>
struct VerifyFold {
  using Node = typename FoldPlanes<PLANES>::Node;
  static constexpr bool CHECKS = true;
  uint32_t root[PLANES];
  __device__ __forceinline__ Node parent(const SetView& s, const Node* in, uint32_t k, uint32_t r, bool& bad) const {
    const SetParent p = set_parent(s, k, r);
    const Node me = in[p.c];
    Node l = me, rr;
    if (p.paired) rr = in[p.c + 1];
    else {
      Node w;
      fold_splat(p.w, w);
      bad = !(p.w < P);   // missing (set_parent answers P), or not a field element
      l = p.odd ? w : me; rr = p.odd ? me : w;
    }
    return fold_hash(l, rr);   // ONE call site of the permutation per plane: paired and lone parents share a wave
  }
  __device__ __forceinline__ void finish(Node top, bool bad, uint32_t* dev) const {
    bool same = true;
#pragma unroll
    for (uint32_t j = 0; j < PLANES; j++) {
      same = same && fold_plane(top, j) == root[j];
      dev[FOLD_ROOT + j] = bad ? 0u : fold_plane(top, j);
    }
    dev[FOLD_VERDICT] = (!bad && same) ? 1u : 0u;
  }
};

// ---- kernels -----------------------------------------------------------------------------------------------------------
// one lane per cell: its four words of every plane range-checked, three Poseidon2 calls per plane -> the node of depth 28
template <uint32_t PLANES> struct FoldValues { const uint4* v[PLANES]; };
template <uint32_t PLANES>
__global__ void __launch_bounds__(SET_BLOCK)
k_fold_cells(FoldValues<PLANES> values, uint32_t n, typename FoldPlanes<PLANES>::Node* __restrict__ out, uint32_t* __restrict__ bad) {
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
  if (!range) *bad = 1u;
#pragma unroll
  for (uint32_t j = 0; j < PLANES; j++) h[j] = range_cell_node(v[j]);
  if constexpr (PLANES == 1) out[t] = h[0];
  else out[t] = make_uint2(h[0], h[1]);
}

// in = S_k, out = S_{k+1} (n_out nodes)
template <class Policy>
__global__ void __launch_bounds__(SET_BLOCK)
k_fold_level(SetView s, Policy pol, const typename Policy::Node* __restrict__ in, uint32_t k, uint32_t n_out, typename Policy::Node* __restrict__ out,
             uint32_t* __restrict__ dev) {
  const uint32_t r = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (r >= n_out) return;
  bool bad = false;
  out[r] = pol.parent(s, in, k, r, bad);
  if (Policy::CHECKS && bad) dev[FOLD_FLAG] = 1u;
}

// S_k0 (w.w[k0] <= SET_TAIL nodes) up to the top, which goes to the policy's finish
template <class Policy>
__global__ void __launch_bounds__(SET_TAIL)
k_fold_tail(SetView s, Policy pol, const typename Policy::Node* __restrict__ in, SetWidths w, uint32_t k0, uint32_t* __restrict__ dev) {
  using Node = typename Policy::Node;
  __shared__ Node level[2][SET_TAIL];
  __shared__ uint32_t bad;   // (only a checking fold touches it)
  const uint32_t t = threadIdx.x;
  if (Policy::CHECKS && t == 0) {
    // the count of the addresses' own flags against the record's
    const size_t last = (size_t)SET_DEPTHS * s.n - 1;
    const uint32_t need = (uint32_t)s.scan[last] + ((uint32_t)s.flag[last] & 1u);
    bad = (dev[FOLD_FLAG] || need != s.n_words) ? 1u : 0u;
  }
  if (t < w.w[k0]) level[0][t] = in[t];
  __syncthreads();
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < SET_DEPTHS; k++) {
    if (t < w.w[k + 1]) {
      bool b = false;
      level[cur ^ 1][t] = pol.parent(s, level[cur], k, t, b);
      if (Policy::CHECKS && b) bad = 1u;
    }
    __syncthreads();
    cur ^= 1;
  }
  if (t == 0) pol.finish(level[cur][0], Policy::CHECKS && bad, dev);
}

// ---- the driver --------------------------------------------------------------------------------------------------------
// Enqueues the per-level steps of the plan from `in` (S_0, the cells' nodes) through the two buffers, then the tail.  `noun`
// names the caller in the one error this can raise.
template <class Policy>
void set_fold_enqueue(const SetFold& f, const cm_mem_set_step steps[SET_STEPS], const Policy& pol, typename Policy::Node* in, typename Policy::Node* out,
                      uint32_t* dev, const char* noun, hipStream_t st) {
  using Node = typename Policy::Node;
  uint32_t s = 1;
  for (; s < SET_STEPS && steps[s].kernel == SET_K_LEVEL; s++) {
    hipLaunchKernelGGL(k_fold_level<Policy>, blocks_for(steps[s].n_nodes, SET_BLOCK), dim3(SET_BLOCK), 0, st, f.view, pol, (const Node*)in, s - 1,
                       steps[s].n_nodes, out, dev);
    std::swap(in, out);
  }
  CM_CHECK(s < SET_STEPS && steps[s].kernel == SET_K_TAIL && f.w.w[s - 1] <= SET_TAIL, std::string(noun) + ": the plan has no tail");
  hipLaunchKernelGGL(k_fold_tail<Policy>, dim3(1), dim3(SET_TAIL), 0, st, f.view, pol, (const Node*)in, f.w, s - 1, dev);
}

// ---- the verifiers' device path --------------------------------------------------------------------------------------------
// PLANES folds of (addresses, values[j], siblings) against roots[j]: *ok, and computed[j] = the roots the record hashes to (zeros
// when it is malformed).  n > 0; the verdicts that need no GPU (bad addresses, a count that is not the plan's) are given here.
// One round trip of 2 + PLANES words on st.
template <uint32_t PLANES>
void verify_fold_device(const char* noun, const uint32_t (&roots)[PLANES], const uint32_t* addresses, uint32_t n, const uint32_t* const (&values)[PLANES],
                        const uint32_t* siblings, uint32_t n_siblings, uint8_t* ok, uint32_t* computed, hipStream_t st) {
  using Node = typename FoldPlanes<PLANES>::Node;
  if (set_first_bad_address(addresses, n) < n) return;
  cm_mem_set_step steps[SET_STEPS];
  if (mem_set_plan(addresses, n, steps) != n_siblings) return;
  const uint32_t words0[FOLD_ROOT + PLANES] = {0};
  DevBuf d_dev(sizeof(words0)), d_addr((size_t)n * 4), d_vals[PLANES], d_words((size_t)n_siblings * 4), d_a((size_t)n * sizeof(Node)),
      d_b((size_t)n * sizeof(Node));
  SetFold f;
  stage_upload(d_dev.p, words0, sizeof(words0), st);
  stage_upload(d_addr.p, addresses, (size_t)n * 4, st);
  FoldValues<PLANES> vals;
  VerifyFold<PLANES> pol;
  for (uint32_t j = 0; j < PLANES; j++) {
    d_vals[j].alloc((size_t)n * 16);
    stage_upload(d_vals[j].p, values[j], (size_t)n * 16, st);
    vals.v[j] = (const uint4*)d_vals[j].p;
    pol.root[j] = roots[j];
  }
  stage_upload(d_words.p, siblings, (size_t)n_siblings * 4, st);
  set_fold_prepare(f, d_addr.u32(), n, steps, d_words.u32(), n_siblings, st);
  hipLaunchKernelGGL(k_fold_cells<PLANES>, blocks_for(n, SET_BLOCK), dim3(SET_BLOCK), 0, st, vals, n, d_a.as<Node>(), d_dev.u32() + FOLD_FLAG);
  set_fold_enqueue(f, steps, pol, d_a.as<Node>(), d_b.as<Node>(), d_dev.u32(), noun, st);
  CM_HIP(hipGetLastError());
  const uint32_t* land = (const uint32_t*)stage_download_async(d_dev.p, sizeof(words0), st);
  CM_HIP(hipStreamSynchronize(st));   // the buffers go back to the pool behind this wait
  *ok = land[FOLD_VERDICT] == 1 ? 1 : 0;
  for (uint32_t j = 0; computed && j < PLANES; j++) computed[j] = land[FOLD_ROOT + j];
}

}  // namespace
}  // namespace cm
