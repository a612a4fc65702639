// Relation tracker for gfx950 (reference: debug_tools/relation_tracker.rs, RelationSummary::summarize_relations): one thread per
// TRACE-domain row, the same entries k_relsum sums.
//   k_track_emit<C>      : every entry of ONE selected relation becomes a record in a fixed slot (entry-major: a wave writes 256
//                          contiguous bytes per array and ordinal); no atomics, no count / scan pass, bit-reproducible.  The grouping
//                          key is the entry's LogUp denominator, which the LogUp argument itself cannot tell apart from the tuple.
//   k_track_emit_small   : every component of <= 256 rows in one launch (blockIdx.y = job), as k_relsum_small does.
//   k_track_recover      : for the survivors of the netting pass: the values of entry `ordinal` of one row, one thread per survivor.
// Invalid witnesses are the normal input: no kernel indexes memory by a cell value.
// Split into parts (kernels_track_N.hip) only to parallelise compilation.
#include "gpu_air.hpp"
#include "track_kernels.hpp"
#include "air_kernels.hpp"
#include "kprof.hpp"

namespace cm {

#define CM_TRACK_SMALL_BOUNDS __launch_bounds__(256, 2)   /* see CM_SMALL_KERNEL_BOUNDS in kernels_air.inc */

#if CM_TRACK_PART == 0 || CM_TRACK_PART == 1
// The entries of relation `sel` of one row -> records.  The relation index of every entry is a compile-time constant after inlining,
// so `r != sel` is a wave-uniform scalar test and the entries of the other relations cost nothing but their cell loads.
struct TrackEval : air::LogupStream<TrackEval, M31, QM31> {
  const uint32_t* const* tr;
  const uint32_t* const* pp;
  const DevRelations* rels;
  TrackRecords rec;
  unsigned long long slot;   // base + row; advanced by 2^log_size per entry of the selected relation
  unsigned long long loc;    // TRACK_LOC(component, row, 0); the ordinal is added per entry
  uint32_t row, stride;
  int sel, ci = 0;
  __device__ M31 next() { return M31(CM_GCOL(tr[ci++])[row]); }
  __device__ M31 preproc(int id) { return M31(CM_GCOL(pp[id])[row]); }
  __device__ M31 c(uint32_t v) { return M31(v); }
  __device__ void constraint(M31) {}
  __device__ QM31 combine(int r, const M31* v, int n) { return dev_combine(rels, r, v, n); }
  __device__ QM31 ef_from(M31 m) { return QM31(m); }
  __device__ void on_entry(int, M31, const M31*, int) {}
  __device__ void emit_batch(bool, QM31, QM31) {}
  __device__ __forceinline__ void rel_arr(int r, M31 mult, const M31* vals, int n) {
    if (r != sel) return;
    unsigned long long hi = TRACK_KEY_NONE, lo = TRACK_KEY_NONE;
    if (!mult.is_zero()) {
      const QM31 d = dev_combine(rels, r, vals, n);
      hi = ((unsigned long long)d.a.a.v << 32) | d.a.b.v;
      lo = ((unsigned long long)d.b.a.v << 32) | d.b.b.v;
    }
    rec.key_hi[slot] = hi;
    rec.key_lo[slot] = lo;
    rec.mult[slot] = mult.v;
    rec.loc[slot] = loc;
    slot += stride;
    loc++;
  }
  __device__ __forceinline__ void finalize_pairs() {}
  __device__ __forceinline__ void finalize_single() {}
};
template <class C>
__device__ __forceinline__ void track_emit_row(const TrackEmitArgs& a, uint32_t r) {
  TrackEval e;
  e.tr = a.tr; e.pp = a.pp; e.rels = a.rels; e.rec = a.rec;
  e.row = r; e.stride = 1u << a.log_size; e.sel = a.relation;
  e.slot = a.base + r;
  e.loc = TRACK_LOC((unsigned long long)a.cid, r, 0);
  C::eval(e);
}
#endif
#if CM_TRACK_PART == 0
template <class C>
__global__ void __launch_bounds__(256) k_track_emit(TrackEmitArgs a) {
  const uint32_t n = 1u << a.log_size;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) track_emit_row<C>(a, r);
}
void launch_track_emit(int cid, const TrackEmitArgs& a, hipStream_t st) {
  const air::ComponentInfo& info = air::component_info(cid);
  KProfScope kp("k_track_emit", (4.0 * info.n_trace + 28.0 * info.rel_count[a.relation]) * (double)(1u << a.log_size), st);
  const uint32_t nb = ((1u << a.log_size) + 255) / 256, grid = nb < 2048 ? nb : 2048;
  switch (cid) {
#define CM_X(id, T) case air::id: hipLaunchKernelGGL(k_track_emit<air::T>, dim3(grid), dim3(256), 0, st, a); break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    default: CM_CHECK(false, "launch_track_emit: bad component id");
  }
  CM_HIP(hipGetLastError());
}
#endif
#if CM_TRACK_PART == 1
template <class C>
__device__ __noinline__ void track_emit_row_call(const TrackEmitArgs* a, uint32_t r) { track_emit_row<C>(*a, r); }
__global__ void CM_TRACK_SMALL_BOUNDS k_track_emit_small(const TrackEmitArgs* __restrict__ jobs, const int* __restrict__ cids) {
  const TrackEmitArgs* a = jobs + blockIdx.y;
  const uint32_t r = threadIdx.x;
  if (r >= (1u << a->log_size)) return;
  switch (cids[blockIdx.y]) {
#define CM_X(id, T) case air::id: track_emit_row_call<air::T>(a, r); break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
  }
}
void launch_track_emit_small(const TrackEmitArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st) {
  if (!n_jobs) return;
  KProfScope kp("k_track_emit_small", 0.0, st);
  hipLaunchKernelGGL(k_track_emit_small, dim3(1, n_jobs), dim3(256), 0, st, d_jobs, d_cids);
  CM_HIP(hipGetLastError());
}
#endif

#if CM_TRACK_PART == 2
// the values of entry `target` of relation `sel` on one row
struct RecoverEval : air::LogupStream<RecoverEval, M31, EmptyEF> {
  const uint32_t* const* tr;
  const uint32_t* const* pp;
  uint32_t* out;   // [TRACK_RECOVER_WORDS]
  uint32_t row, target, ord = 0;
  int sel, ci = 0;
  __device__ M31 next() { return M31(CM_GCOL(tr[ci++])[row]); }
  __device__ M31 preproc(int id) { return M31(CM_GCOL(pp[id])[row]); }
  __device__ M31 c(uint32_t v) { return M31(v); }
  __device__ void constraint(M31) {}
  __device__ EmptyEF combine(int, const M31*, int) { return {}; }
  __device__ EmptyEF ef_from(M31) { return {}; }
  __device__ void on_entry(int, M31, const M31*, int) {}
  __device__ void emit_batch(bool, EmptyEF, EmptyEF) {}
  __device__ __forceinline__ void rel_arr(int r, M31, const M31* vals, int n) {
    if (r != sel) return;
    if (ord++ != target) return;
    out[0] = (uint32_t)n;
    for (int i = 0; i < n; i++) out[1 + i] = vals[i].v;
  }
  __device__ __forceinline__ void finalize_pairs() {}
  __device__ __forceinline__ void finalize_single() {}
};
template <class C>
__device__ __noinline__ void track_recover_call(const TrackRecoverJob* j, const uint32_t* const* pp, uint32_t* out) {
  RecoverEval e;
  e.tr = j->tr; e.pp = pp; e.out = out; e.row = j->row; e.target = j->ordinal; e.sel = j->relation;
  C::eval(e);
}
__global__ void __launch_bounds__(64) k_track_recover(const TrackRecoverJob* __restrict__ jobs, uint32_t n_jobs, const uint32_t* const* pp,
                                                      uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_jobs) return;
  const TrackRecoverJob* j = jobs + i;
  uint32_t* o = out + (size_t)TRACK_RECOVER_WORDS * i;
  for (int k = 0; k < TRACK_RECOVER_WORDS; k++) o[k] = 0;
  switch (j->cid) {
#define CM_X(id, T) case air::id: track_recover_call<air::T>(j, pp, o); break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
  }
}
void launch_track_recover(const TrackRecoverJob* d_jobs, uint32_t n_jobs, const uint32_t* const* d_pp, uint32_t* d_out, hipStream_t st) {
  if (!n_jobs) return;
  KProfScope kp("k_track_recover", 0.0, st);
  hipLaunchKernelGGL(k_track_recover, dim3((n_jobs + 63) / 64), dim3(64), 0, st, d_jobs, n_jobs, d_pp, d_out);
  CM_HIP(hipGetLastError());
}
#endif

}  // namespace cm
