// Host half of the composition phase (stwo prove: constraint quotients of every component -> composition polynomial), shared by the
// single-GPU prover (prover.hip) and the sharded one (prover_sharded.inc): the evaluation-domain copies for log_blowup_factor > 1,
// the accumulator layout and its one zeroing launch, the per-component arguments both compute alike, and
// DomainEvaluationAccumulator::finalize.  What stays with each prover is where they really differ: column tables, slot policy,
// uploads, the side-stream plan of the region, the device transcript step and the cross-rank reduction.
#pragma once
#include "prover_common.hpp"
#include "air_kernels.hpp"
#include "gpu_air.hpp"
#include <map>
#include <set>

namespace cm {
// (coset_vanishing_canonic, fill_constraint_args: air_kernels.hpp)
// up to three device ranges zeroed by ONE launch (the constraints phase clears two accumulator sets and the slot buffer right in
// front of its kernels: three dependent hipMemsetAsync = three packets on the critical path behind the interaction tree)
struct ZeroRanges { uint4* p[3]; uint64_t n16[3]; };
__global__ void __launch_bounds__(256) k_zero_ranges(ZeroRanges z) {
  for (int r = 0; r < 3; r++)
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < z.n16[r]; i += (uint64_t)gridDim.x * 256) z.p[r][i] = make_uint4(0, 0, 0, 0);
}
static void zero_ranges(void* const p[3], const size_t bytes[3], hipStream_t st) {
  ZeroRanges z;
  uint64_t total = 0;
  for (int r = 0; r < 3; r++) {
    CM_CHECK(((uintptr_t)p[r] & 15) == 0 && (bytes[r] & 15) == 0, "zero_ranges: ranges must be 16-byte aligned");
    z.p[r] = (uint4*)p[r]; z.n16[r] = bytes[r] / 16; total += z.n16[r];
  }
  if (!total) return;
  const unsigned blocks = (unsigned)std::min<uint64_t>((total + 255) / 256, 256 * 16);
  hipLaunchKernelGGL(k_zero_ranges, dim3(blocks), dim3(256), 0, st, z);
  CM_HIP(hipGetLastError());
}

// The constraints are evaluated on CanonicCoset(log + 1).  With log_blowup_factor = 1 (REGULAR_96_BITS) that is the committed LDE
// domain and the kernels read the committed columns; with a larger blowup every polynomial of trees 0..2 is evaluated on its
// (log + 1) domain separately (Stwo does the same: `poly.evaluate(eval_domain)`), at the cost of one more forward transform per
// column and its memory.  `src` = the coefficient sets this prover holds of the three trees.
// No host synchronisation: the pointer table is a temporary, but a freed block goes back to the calling thread's pool and is only
// handed to later work of the same thread, which is ordered behind `st` (pool.hip; DevBuf in engine.hpp).
inline void eval_domain_copies(ColumnSet (&cdom)[3], const ColumnSet* const (&src)[3], const Twiddles& tw, hipStream_t st) {
  for (int t = 0; t < 3; t++) {
    std::vector<uint32_t> logs(src[t]->logs);
    for (auto& l : logs) l += 1;
    cdom[t].alloc(logs, st);
    std::vector<const uint32_t*> table;
    struct Grp { uint32_t log, n; size_t off; };
    std::vector<Grp> grps;
    for (auto& kv : by_log(src[t]->logs)) {
      grps.push_back(Grp{kv.first, (uint32_t)kv.second.size(), table.size()});
      for (auto i : kv.second) table.push_back(src[t]->ptrs[i]);
      for (auto i : kv.second) table.push_back(cdom[t].ptrs[i]);
    }
    DevBuf d_table = upload(table, st);
    const uint32_t** dt = d_table.as<const uint32_t*>();
    for (auto& g : grps) evaluate((const uint32_t* const*)(dt + g.off), (uint32_t* const*)(dt + g.off + g.n), g.n, g.log, g.log + 1, tw, st);
  }
}

// Accumulators: 4 columns per evaluation log.  The top size gets its own ColumnSet (it becomes the coefficient set of tree 3), all
// smaller sizes share one — two pointer tables and ONE zeroing launch (together with the slot buffer) instead of one pair per size.
struct ConstraintAccumulators {
  uint32_t comp_log = 0;
  std::map<uint32_t, std::vector<int>> cgroups;   // evaluation log -> the components that take part
  ColumnSet top, rest;
  std::map<uint32_t, size_t> at;                  // evaluation log below comp_log -> first of its four columns in `rest`
  std::set<uint32_t> interpolated;                // evaluation logs whose accumulator was interpolated inside the constraints region
  template <class Pred>
  void plan(const uint32_t* clog, uint32_t comp_log_, Pred takes_part) {
    comp_log = comp_log_;
    for (int c = 0; c < air::N_COMPONENTS; c++) if (takes_part(c)) cgroups[clog[c] + 1].push_back(c);
  }
  // upload_ptrs = false: the pointer tables travel in the caller's own upload (ColumnSet::d_view); top_contiguous: exchanged as one block
  void alloc(hipStream_t st, bool upload_ptrs, bool top_contiguous) {
    std::vector<uint32_t> rest_logs;
    for (auto& kv : cgroups)
      if (kv.first != comp_log) { at[kv.first] = rest_logs.size(); rest_logs.insert(rest_logs.end(), 4, kv.first); }
    top.alloc(std::vector<uint32_t>(4, comp_log), st, upload_ptrs, top_contiguous);
    if (!rest_logs.empty()) rest.alloc(rest_logs, st, upload_ptrs);
  }
  uint32_t* const* of(uint32_t el) const { return el == comp_log ? top.dev() : rest.dev(at.at(el)); }
  // both sets and the caller's slot buffer, in one launch
  void zero(void* slots, size_t slot_words, hipStream_t st) const {
    void* const zp[3] = {top.buf.p, rest.buf.p ? rest.buf.p : top.buf.p, slots};
    const size_t zb[3] = {top.buf.bytes & ~(size_t)15, rest.buf.p ? (rest.buf.bytes & ~(size_t)15) : 0, (slot_words * 4 + 15) & ~(size_t)15};
    zero_ranges(zp, zb, st);
  }
};

// A WIDE component of few rows (poseidon2: 443 columns, 426 constraints on 2^10 evaluation rows) is one long program per row on four
// blocks: ~0.33 ms of pure latency.  In size order it was enqueued last and ran ALONE behind the large kernels; launched first it
// hides under them.  "cons_wide_first" = 0: the plain size order (A/B).
inline bool is_wide_component(int c, const uint32_t* clog) {
  return tune(T_CONS_WIDE_FIRST) != 0 && air::component_info(c).n_trace >= 128 && clog[c] <= 14;
}

// DomainEvaluationAccumulator::finalize.  Stwo walks the sizes upward: interpolate(vals_l + evaluate_l(cur)).  Interpolation is
// linear and interpolate_l(evaluate_l(cur)) is cur zero-padded (coefficient bases nest), so the same coefficients come from
// interpolating every accumulator at its OWN size and adding the zero-padded coefficient vectors — field arithmetic is exact, the
// result is bit-identical, and the extend/add chain over the large domains disappears.  What the region did not interpolate (the
// slotted / batched small sizes: a handful of single-launch transforms) is interpolated here in a row, largest first; ONE launch
// adds all sizes into `top`.
inline void finalize_accumulators(ConstraintAccumulators& acc, const Twiddles& tw, hipStream_t st) {
  if (!acc.interpolated.count(acc.comp_log)) interpolate(acc.top.dev(), 4, acc.comp_log, tw, st);
  for (auto it = acc.at.rbegin(); it != acc.at.rend(); ++it)
    if (!acc.interpolated.count(it->first)) interpolate(acc.of(it->first), 4, it->first, tw, st);
  AddColumnsSrc as;
  as.n = 0;
  for (auto& kv : acc.at) {
    CM_CHECK(as.n < 28, "composition: too many accumulator sizes");
    as.log[as.n] = kv.first;
    as.src[as.n++] = (const uint32_t* const*)acc.of(kv.first);
  }
  add_columns_multi(acc.top.dev(), as, 4, st);
}
}  // namespace cm
