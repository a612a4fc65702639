// k_verify_oods<CM_OODS_GROUP>: the device point evaluator of the batched verifier (formats: verify_prelude.hpp), included by
// verify_prelude_oods_0.hip .. _3.hip with CM_OODS_GROUP defined.  One kernel per component GROUP, every component's description
// inlined into its arm of the switch: an arm then owns the kernel's whole register file (256 VGPRs + 256 AGPRs at one wave per
// SIMD) and saves nothing for a caller, and the kernels report no scratch.  One kernel with all 34 arms compiles for 13 minutes;
// four compile side by side in under two.  Every group is launched over the WHOLE job list and leaves the other groups' jobs
// alone (a wave holds one component, so a foreign wave ends at once).
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "verify_prelude.hpp"
#include <type_traits>

namespace cm {

namespace {

constexpr uint32_t OODS_THREADS = 64;

__device__ __forceinline__ QM31 ldq(const uint32_t* p) { return QM31::from_u32(p); }
__device__ __forceinline__ void stq(uint32_t* p, const QM31& v) { v.to_u32(p); }
__device__ __forceinline__ QM31 rel_z(const uint32_t* rel, int r) { return ldq(rel + 4 * r); }
__device__ __forceinline__ QM31 rel_alpha(const uint32_t* rel, int r, int i) { return ldq(rel + 4 * air::N_RELATIONS + 4 * (r * air::MAX_REL_SIZE + i)); }
__device__ __forceinline__ QM31 dev_combine_ef(const QM31* c4) {
  return c4[0] + c4[1] * QM31(M31(0), M31(1), M31(0), M31(0)) + c4[2] * QM31(M31(0), M31(0), M31(1), M31(0)) +
         c4[3] * QM31(M31(0), M31(0), M31(0), M31(1));
}

// ---- device point evaluator: PointEvalH (point_eval.hip) over words in global memory.  Every index below is a compile-time
// constant once a component's description is inlined, so mask values, relation words and coefficients are read through pointers
// at constant offsets and no local array is indexed at run time.
// A PASS evaluates a slice of the constraints: PASS_BASE the base constraints [LO, HI), PASS_LOGUP the LogUp batches [LO, HI);
// what the other constraints would have computed is dead code and the values only they read are never loaded.  The sum over
// a partition of the constraints is the whole numerator (exact field arithmetic: the order does not show).  The two widest
// components are evaluated in five passes, every other one in PASS_ALL.
enum : int { PASS_ALL = 0, PASS_BASE = 1, PASS_LOGUP = 2 };
template <int MODE, int LO, int HI>
struct PointEvalD : air::LogupStream<PointEvalD<MODE, LO, HI>, QM31, QM31> {
  const uint32_t *tr, *it, *pp, *rw, *coeff;   // rw: air::RelationsRaw words
  uint32_t n_base;
  QM31 cumsum_shift, prev_col, acc;
  int ci = 0, ii = 0, kb = 0, kl = 0;
  __device__ __forceinline__ QM31 next() { return ldq(tr + 4 * ci++); }
  __device__ __forceinline__ QM31 preproc(int id) { return ldq(pp + 4 * id); }
  __device__ __forceinline__ QM31 c(uint32_t v) { return QM31(M31(v)); }
  __device__ __forceinline__ void constraint(QM31 x) {
    if (MODE == PASS_ALL || (MODE == PASS_BASE && kb >= LO && kb < HI)) acc += ldq(coeff + 4 * kb) * x;
    kb++;
  }
  __device__ __forceinline__ void constraint_q(QM31 x) {
    if (MODE == PASS_ALL || (MODE == PASS_LOGUP && kl >= LO && kl < HI)) acc += ldq(coeff + 4 * (n_base + kl)) * x;
    kl++;
  }
  __device__ __forceinline__ QM31 combine(int r, const QM31* v, int n) {
    QM31 a;
#pragma unroll
    for (int i = 0; i < n; i++) a += rel_alpha(rw, r, i) * v[i];
    return a - rel_z(rw, r);
  }
  __device__ __forceinline__ QM31 ef_from(QM31 m) { return m; }
  __device__ __forceinline__ void on_entry(int, QM31, const QM31*, int) {}
  __device__ __forceinline__ QM31 ef4(const uint32_t* p, int stride) {   // combine_ef of four values `stride` QM31 apart
    const QM31 c4[4] = {ldq(p), ldq(p + 4 * stride), ldq(p + 8 * stride), ldq(p + 12 * stride)};
    return dev_combine_ef(c4);
  }
  __device__ __forceinline__ void emit_batch(bool last, QM31 num, QM31 den) {
    if (!last) {
      const QM31 cur = ef4(it + 4 * ii, 1);
      ii += 4;
      const QM31 diff = cur - prev_col;
      prev_col = cur;
      constraint_q(diff * den - num);
    } else {
      const QM31 pr = ef4(it + 4 * ii, 2), cu = ef4(it + 4 * ii + 4, 2);
      ii += 8;
      constraint_q((cu - pr - prev_col + cumsum_shift) * den - num);
    }
  }
};
template <class T, int MODE, int LO, int HI>
__device__ __forceinline__ QM31 point_eval_pass(const uint32_t* tr, const uint32_t* it, const uint32_t* pp, const uint32_t* rel,
                                                const uint32_t* coeff, uint32_t n_base, const uint32_t* shift) {
  PointEvalD<MODE, LO, HI> e;
  e.tr = tr; e.it = it; e.pp = pp; e.rw = rel; e.coeff = coeff; e.n_base = n_base; e.cumsum_shift = ldq(shift);
  T::eval(e);
  return e.acc;
}
constexpr int PASS_END = 1 << 30;
template <class T>
__device__ __forceinline__ QM31 point_eval_component(const uint32_t* tr, const uint32_t* it, const uint32_t* pp, const uint32_t* rel,
                                                     const uint32_t* coeff, uint32_t n_base, const uint32_t* shift) {
  if constexpr (std::is_same_v<T, air::ComponentOf<air::C_U32_STORE_DIV_FP_IMM>::type> ||
                std::is_same_v<T, air::ComponentOf<air::C_U32_STORE_DIV_FP_FP>::type>) {
    // 51 / 54 columns, 19 base constraints, 27 / 29 LogUp batches: in one pass they spill 61 / 73 VGPRs beyond all 512 registers
    QM31 s = point_eval_pass<T, PASS_BASE, 0, 10>(tr, it, pp, rel, coeff, n_base, shift);
    s += point_eval_pass<T, PASS_BASE, 10, PASS_END>(tr, it, pp, rel, coeff, n_base, shift);
    s += point_eval_pass<T, PASS_LOGUP, 0, 9>(tr, it, pp, rel, coeff, n_base, shift);
    s += point_eval_pass<T, PASS_LOGUP, 9, 18>(tr, it, pp, rel, coeff, n_base, shift);
    s += point_eval_pass<T, PASS_LOGUP, 18, PASS_END>(tr, it, pp, rel, coeff, n_base, shift);
    return s;
  } else {
    return point_eval_pass<T, PASS_ALL, 0, PASS_END>(tr, it, pp, rel, coeff, n_base, shift);
  }
}

template <int G>
__global__ __launch_bounds__(OODS_THREADS) void k_verify_oods(const uint32_t* __restrict__ blob, uint32_t* __restrict__ scr,
                                                              const uint32_t* __restrict__ jobs, uint32_t n_jobs) {
  const uint32_t i = blockIdx.x * OODS_THREADS + threadIdx.x;
  if (i >= n_jobs) return;
  const uint32_t* J = jobs + VP_OODS_JOB_WORDS * (size_t)i;
  const uint32_t cid = J[0];
  if (cid >= (uint32_t)air::N_COMPONENTS || verify_oods_group((int)cid) != G) return;   // another group's job, or padding (VP_NONE)
  const uint32_t *tr = blob + J[2], *it = blob + J[3], *pp = blob + J[4], *rel = blob + J[5], *coeff = blob + J[6], *shift = blob + J[7];
  const uint32_t n_base = J[1], log = J[8];
  QM31 num;
  switch (cid) {
#define CM_X(id, T)                                                                                                          \
  case air::id:                                                                                                              \
    if constexpr (verify_oods_group(air::id) == G) num = point_eval_component<air::T>(tr, it, pp, rel, coeff, n_base, shift); \
    break;
    AIR_ALL_COMPONENTS(CM_X)
#undef CM_X
    default: break;
  }
  if (log) {   // canonic_vanishing(log, oods) (verifier_common.hpp)
    QM31 x = ldq(blob + J[9]);
    for (uint32_t k = 1; k < log; k++) x = double_x(x);
    num = num * inv(x);
  }
  stq(scr + J[10], num);
}

}  // namespace

template <>
void launch_verify_oods_group<CM_OODS_GROUP>(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st) {
  hipLaunchKernelGGL(k_verify_oods<CM_OODS_GROUP>, dim3((n_jobs + OODS_THREADS - 1) / OODS_THREADS), dim3(OODS_THREADS), 0, st, blob, scr, jobs, n_jobs);
}

}  // namespace cm
