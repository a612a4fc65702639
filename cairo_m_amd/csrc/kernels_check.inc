// PCS-free AIR check for gfx950 (reference: debug_tools/assert_constraints.rs; the relation tracker proper is kernels_track.inc):
// one thread per TRACE-domain row.
//   k_check<C>        : every constraint of component C tested for zero on every row (RowCheckEval); failing rows counted with a
//                       wave ballot + one atomic per wave that saw one, the lowest (row, constraint) by a 64-bit atomicMin.  A row
//                       that satisfies its constraints issues no atomic at all.
//   k_relsum<C>       : per relation, sum over rows and entries of mult / combine_r(values) (RelSumEval), reduced per block into
//                       64-bit word sums (one atomic per block and word).
//   k_*_small         : every component of <= 256 rows in one launch (blockIdx.y = job), as k_constraints_small does.
//   k_lookup_diag<C>  : after the histogram flagged an out-of-range lookup value, the lowest (component, row) and its table.
// Invalid witnesses are the normal input: no kernel indexes memory by a cell value, and failures are data, never a trap.
// Split into parts (kernels_check_N.hip) only to parallelise compilation.
#include "gpu_air.hpp"
#include "check_kernels.hpp"
#include "air_kernels.hpp"
#include "kprof.hpp"

namespace cm {

constexpr int CHECK_PREFETCH_MAX = 80;   // components with more trace columns (poseidon2: 443) load on demand
#define CM_CHECK_SMALL_BOUNDS __launch_bounds__(256, 2)   /* see CM_SMALL_KERNEL_BOUNDS in kernels_air.inc */

#if CM_CHECK_PART == 0 || CM_CHECK_PART == 1
// lowest failing constraint of row r, -1 = none
template <class C>
__device__ __forceinline__ int check_row(const CheckArgs& a, uint32_t r) {
  RowCheckEval e;
  e.tr = a.tr; e.it = a.it; e.pp = a.pp; e.rels = a.rels;
  e.row = r; e.prev_row = shifted_row(r, a.log_size, a.log_size, -1);
  e.n_base = a.n_base;
  e.cumsum_shift = QM31::from_u32(a.claimed_sum) * M31(1u << (31 - a.log_size));   // 1 / 2^n = 2^(31 - n) modulo 2^31 - 1
  constexpr int NPF = C::N_TRACE <= CHECK_PREFETCH_MAX ? C::N_TRACE : 1;
  uint32_t trv[NPF];
  if (C::N_TRACE <= CHECK_PREFETCH_MAX) {
#pragma unroll
    for (int c = 0; c < NPF; c++) trv[c] = CM_GCOL(a.tr[c])[r];
    e.trv = trv;
  }
  C::eval(e);
  return e.first_bad;
}
// every lane of the wave calls this (live = the lane has a row)
__device__ __forceinline__ void check_report(const CheckArgs& a, uint32_t r, bool live, int fb) {
  const bool bad = live && fb >= 0;
  if (live && a.row_status) a.row_status[r] = bad ? (uint32_t)fb : CHECK_KEY_NONE;
  const unsigned long long m = __ballot(bad);
  if (!m) return;
  unsigned long long key = bad ? (((unsigned long long)r << 16) | (uint32_t)fb) : ~0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off, 64);
    const unsigned long long o = ((unsigned long long)hi << 32) | lo;
    key = o < key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(a.failing_rows, (unsigned long long)__popcll(m));
    atomicMin(a.first, key);
  }
}
#endif
#if CM_CHECK_PART == 0
template <class C>
__global__ void __launch_bounds__(256) k_check(CheckArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = r < (1u << a.log_size);
  const int fb = live ? check_row<C>(a, r) : -1;
  check_report(a, r, live, fb);
}
void launch_check(int cid, const CheckArgs& a, hipStream_t st) {
  KProfScope kp("k_check", 4.0 * (air::component_info(cid).n_trace + air::component_info(cid).n_interaction) * (double)(1u << a.log_size), st);
  const dim3 grid(((1u << a.log_size) + 255) / 256);
  switch (cid) {
#define CM_X(id, T) case air::id: hipLaunchKernelGGL(k_check<air::T>, grid, dim3(256), 0, st, a); break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    default: CM_CHECK(false, "launch_check: bad component id");
  }
  CM_HIP(hipGetLastError());
}
#endif
#if CM_CHECK_PART == 1
template <class C>
__device__ __noinline__ int check_row_call(const CheckArgs* a, uint32_t r) { return check_row<C>(*a, r); }
__global__ void CM_CHECK_SMALL_BOUNDS k_check_small(const CheckArgs* __restrict__ jobs, const int* __restrict__ cids) {
  const CheckArgs* a = jobs + blockIdx.y;
  const uint32_t r = threadIdx.x;
  const bool live = r < (1u << a->log_size);
  int fb = -1;
  if (live) {
    switch (cids[blockIdx.y]) {
#define CM_X(id, T) case air::id: fb = check_row_call<air::T>(a, r); break;
      AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    }
  }
  check_report(*a, r, live, fb);
}
void launch_check_small(const CheckArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st) {
  if (!n_jobs) return;
  KProfScope kp("k_check_small", 0.0, st);
  hipLaunchKernelGGL(k_check_small, dim3(1, n_jobs), dim3(256), 0, st, d_jobs, d_cids);
  CM_HIP(hipGetLastError());
}
#endif

#if CM_CHECK_PART == 2 || CM_CHECK_PART == 3
template <class C>
__device__ __forceinline__ void relsum_row(const RelSumArgs& a, uint32_t r, QM31 out[air::N_RELATIONS]) {
  RelSumEval e;
  e.tr = a.tr; e.pp = a.pp; e.rels = a.rels; e.row = r;
  C::eval(e);
  e.finish(out);
}
// block sum of acc[r] (all lanes of the block call this) -> one 64-bit atomic per non-zero word
__device__ __forceinline__ void relsum_flush(const RelSumArgs& a, const QM31 acc[air::N_RELATIONS]) {
  __shared__ uint32_t red[4][air::N_RELATIONS * 4];   // [wave][word]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < air::N_RELATIONS; r++) {
    const QM31 q = wave_reduce_qm31(acc[r]);
    if (lane == 0) q.to_u32(&red[w][4 * r]);
  }
  __syncthreads();
  if (threadIdx.x < air::N_RELATIONS * 4) {
    unsigned long long s = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); k++) s += red[k][threadIdx.x];
    if (s) atomicAdd(a.sums + threadIdx.x, s);
  }
}
#endif
#if CM_CHECK_PART == 2
// persistent blocks (grid-stride over the rows): at most 1024 blocks per component, so at most 1024 atomics per word
template <class C>
__global__ void __launch_bounds__(256) k_relsum(RelSumArgs a) {
  QM31 acc[air::N_RELATIONS];
  const uint32_t n = 1u << a.log_size;
  for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += gridDim.x * blockDim.x) {
    QM31 out[air::N_RELATIONS];
    relsum_row<C>(a, r, out);
#pragma unroll
    for (int k = 0; k < air::N_RELATIONS; k++) acc[k] += out[k];
  }
  relsum_flush(a, acc);
}
void launch_relsum(int cid, const RelSumArgs& a, hipStream_t st) {
  KProfScope kp("k_relsum", 4.0 * air::component_info(cid).n_trace * (double)(1u << a.log_size), st);
  const uint32_t nb = ((1u << a.log_size) + 255) / 256, grid = nb < 1024 ? nb : 1024;
  switch (cid) {
#define CM_X(id, T) case air::id: hipLaunchKernelGGL(k_relsum<air::T>, dim3(grid), dim3(256), 0, st, a); break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    default: CM_CHECK(false, "launch_relsum: bad component id");
  }
  CM_HIP(hipGetLastError());
}
#endif
#if CM_CHECK_PART == 3
template <class C>
__device__ __noinline__ void relsum_row_call(const RelSumArgs* a, uint32_t r, QM31* out) { relsum_row<C>(*a, r, out); }
__global__ void CM_CHECK_SMALL_BOUNDS k_relsum_small(const RelSumArgs* __restrict__ jobs, const int* __restrict__ cids) {
  const RelSumArgs* a = jobs + blockIdx.y;
  const uint32_t r = threadIdx.x;
  QM31 acc[air::N_RELATIONS];
  if (r < (1u << a->log_size)) {
    switch (cids[blockIdx.y]) {
#define CM_X(id, T) case air::id: relsum_row_call<air::T>(a, r, acc); break;
      AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    }
  }
  relsum_flush(*a, acc);
}
void launch_relsum_small(const RelSumArgs* d_jobs, const int* d_cids, uint32_t n_jobs, hipStream_t st) {
  if (!n_jobs) return;
  KProfScope kp("k_relsum_small", 0.0, st);
  hipLaunchKernelGGL(k_relsum_small, dim3(1, n_jobs), dim3(256), 0, st, d_jobs, d_cids);
  CM_HIP(hipGetLastError());
}

// the same range tests as HistEval (gpu_air.hpp), which raised the flag; table of the row's first out-of-range entry, -1 = none
struct LookupDiagEval : air::LogupStream<LookupDiagEval, M31, EmptyEF> {
  const uint32_t* const* cols;
  uint32_t row;
  int ci = 0, table = -1;
  __device__ M31 next() { return M31(CM_GCOL(cols[ci++])[row]); }
  __device__ M31 preproc(int) { return M31(); }
  __device__ M31 c(uint32_t v) { return M31(v); }
  __device__ void constraint(M31) {}
  __device__ EmptyEF combine(int, const M31*, int) { return {}; }
  __device__ EmptyEF ef_from(M31) { return {}; }
  __device__ void emit_batch(bool, EmptyEF, EmptyEF) {}
  __device__ void on_entry(int rel, M31, const M31* v, int) {
    int t = -1;
    if (rel == air::REL_RC8) t = v[0].v < 256u ? -1 : 0;
    else if (rel == air::REL_RC16) t = v[0].v < (1u << 16) ? -1 : 1;
    else if (rel == air::REL_RC20) t = v[0].v < (1u << 20) ? -1 : 2;
    else if (rel == air::REL_BITWISE) t = ((v[0].v < 3u) & (v[1].v < 256u) & (v[2].v < 256u)) ? -1 : 3;
    if (t >= 0 && table < 0) table = t;
  }
};
template <class C>
__global__ void __launch_bounds__(256) k_lookup_diag(const uint32_t* const* __restrict__ cols, uint32_t log_size, unsigned long long cid_key,
                                                     unsigned long long* key) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= (1u << log_size)) return;
  LookupDiagEval e;
  e.cols = cols; e.row = r;
  C::eval(e);
  if (e.table >= 0) atomicMin(key, cid_key | ((unsigned long long)r << 8) | (unsigned)e.table);   // (runs only after a flagged input)
}
void launch_lookup_diag(int cid, const uint32_t* const* d_cols, uint32_t log_size, unsigned long long* key, hipStream_t st) {
  const dim3 grid(((1u << log_size) + 255) / 256);
  const unsigned long long ck = (unsigned long long)cid << 40;
  switch (cid) {
#define CM_X(id, T) case air::id: hipLaunchKernelGGL(k_lookup_diag<air::T>, grid, dim3(256), 0, st, d_cols, log_size, ck, key); break;
    AIR_OPCODE_COMPONENTS(CM_X)
#undef CM_X
    default: CM_CHECK(false, "launch_lookup_diag: not an opcode component");
  }
  CM_HIP(hipGetLastError());
}
#endif

}  // namespace cm
