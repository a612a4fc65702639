// The prelude's arithmetic on the GPU (formats: verify_prelude.hpp): k_verify_public_sum (initial_logup_sum's per-entry terms)
// and k_verify_prelude_fin (the two verdicts of a proof) — k_verify_oods, the device twin of point_eval.hip's PointEvalH, is in
// verify_prelude_oods.inc, one kernel per component group — and the op-level entries that run them on caller-chosen words next
// to their host twins.
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "verifier_common.hpp"
#include "verify_prelude.hpp"
#include "abi.hpp"
#include <string.h>
#include <string>
#include <vector>

namespace cm {

namespace {

static_assert(CM_PUBLIC_SUM_ENTRIES == VP_SUM_THREADS && CM_RELATIONS_WORDS == VP_REL_WORDS && CM_N_PREPROCESSED == air::N_PREPROC,
              "cairom_hip.h restates the prelude kernels' constants");
constexpr uint32_t FIN_THREADS = 64;

__device__ __forceinline__ QM31 ldq(const uint32_t* p) { return QM31::from_u32(p); }
__device__ __forceinline__ void stq(uint32_t* p, const QM31& v) { v.to_u32(p); }
__device__ __forceinline__ QM31 rel_z(const uint32_t* rel, int r) { return ldq(rel + 4 * r); }
__device__ __forceinline__ QM31 rel_alpha(const uint32_t* rel, int r, int i) { return ldq(rel + 4 * air::N_RELATIONS + 4 * (r * air::MAX_REL_SIZE + i)); }
// sum alpha^i * v_i - z over M31 values (verifier_common.hpp combine)
template <int N>
__device__ __forceinline__ QM31 combine_m(const uint32_t* rel, int r, const M31 (&v)[N]) {
  QM31 a;
#pragma unroll
  for (int i = 0; i < N; i++) a += rel_alpha(rel, r, i) * v[i];
  return a - rel_z(rel, r);
}
__device__ __forceinline__ QM31 dev_combine_ef(const QM31* c4) {
  return c4[0] + c4[1] * QM31(M31(0), M31(1), M31(0), M31(0)) + c4[2] * QM31(M31(0), M31(0), M31(1), M31(0)) +
         c4[3] * QM31(M31(0), M31(0), M31(0), M31(1));
}
__device__ __forceinline__ QM31 wave_sum(QM31 v) {
  uint32_t w[4];
  v.to_u32(w);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
    for (int k = 0; k < 4; k++) w[k] = (M31(w[k]) + M31((uint32_t)__shfl_down((int)w[k], d, 64))).v;
  }
  return QM31::from_u32(w);
}

// One workgroup per chunk of one public list, one thread per entry: the memory tuple and the four Merkle leaves of
// initial_logup_sum with its signs (program / input emit under initial_root, output consumes under final_root), their five
// inverses from ONE Fermat inverse (Montgomery's trick; a zero denominator is taken out of the product and contributes 0, as
// inv(0) = 0 does on the host), summed across the wave's lanes and then across the waves through LDS.
__global__ __launch_bounds__(VP_SUM_THREADS) void k_verify_public_sum(const uint32_t* __restrict__ blob, uint32_t* __restrict__ scr,
                                                                      const uint32_t* __restrict__ jobs) {
  __shared__ uint32_t red[4 * (VP_SUM_THREADS / 64)];
  const uint32_t tid = threadIdx.x;
  const uint32_t* J = jobs + VP_SUM_JOB_WORDS * (size_t)blockIdx.x;
  const uint32_t n = J[1] < VP_SUM_THREADS ? J[1] : VP_SUM_THREADS;
  const bool emit = J[2] != 0;
  const uint32_t* rel = blob + J[4];
  QM31 part;
  if (tid < n) {
    const uint32_t* e = blob + J[0] + 7 * (size_t)tid;
    if (e[0]) {
      const M31 addr(e[1]), clock(e[6]), root(J[3]), height(air::TREE_HEIGHT), four(4);
      const M31 val[4] = {M31(e[2]), M31(e[3]), M31(e[4]), M31(e[5])};
      QM31 den[5], pre[5];
      bool zero[5];
      {
        const M31 t[6] = {addr, clock, val[0], val[1], val[2], val[3]};
        den[0] = combine_m(rel, air::REL_MEMORY, t);
      }
#pragma unroll
      for (uint32_t k = 0; k < 4; k++) {
        const M31 t[4] = {four * addr + M31(k), height, val[k], root};
        den[1 + k] = combine_m(rel, air::REL_MERKLE, t);
      }
      QM31 run = QM31(M31(1));
#pragma unroll
      for (int k = 0; k < 5; k++) {
        zero[k] = den[k].is_zero();
        if (zero[k]) den[k] = QM31(M31(1));
        pre[k] = run;
        run = run * den[k];
      }
      QM31 iv = inv(run);
#pragma unroll
      for (int k = 4; k >= 0; k--) {
        QM31 f = iv * pre[k];
        iv = iv * den[k];
        if (zero[k]) f = QM31();
        if (k == 0 && emit) part += f;
        else part -= f;
      }
    }
  }
  part = wave_sum(part);
  if ((tid & 63u) == 0) stq(red + 4 * (tid >> 6), part);
  __syncthreads();
  if (tid == 0) {
    QM31 s = ldq(red);
#pragma unroll
    for (uint32_t w = 1; w < VP_SUM_THREADS / 64; w++) s += ldq(red + 4 * w);
    stq(scr + J[5], s);
  }
}

// One thread per proof: the two verdicts.  LogUp: the chunks' partial sums, the four fixed terms of initial_logup_sum (two
// register tuples, two roots) and the claimed sums must add to zero.  OODS: the components' quotients must add to combine_ef of
// the composition's four sampled values.
__global__ __launch_bounds__(FIN_THREADS) void k_verify_prelude_fin(const uint32_t* __restrict__ blob, uint32_t* __restrict__ scr,
                                                                    uint32_t* __restrict__ flags, const uint32_t* __restrict__ jobs, uint32_t n_jobs) {
  const uint32_t i = blockIdx.x * FIN_THREADS + threadIdx.x;
  if (i >= n_jobs) return;
  const uint32_t* J = jobs + VP_FIN_JOB_WORDS * (size_t)i;
  if (J[VPF_DO_LOGUP]) {
    const uint32_t* h = blob + J[VPF_HEAD];
    const uint32_t* rel = blob + J[VPF_REL];
    const M31 one(1), zero;
    QM31 s;
    for (uint32_t p = 0; p < J[VPF_N_PARTS]; p++) s += ldq(scr + J[VPF_PARTS] + 4 * (size_t)p);
    {
      const M31 t[3] = {M31(h[0]), M31(h[1]), one};
      s += inv(combine_m(rel, air::REL_REGISTERS, t));
    }
    {
      const M31 t[3] = {M31(h[2]), M31(h[3]), M31(h[4]) + one};
      s -= inv(combine_m(rel, air::REL_REGISTERS, t));
    }
    {
      const M31 t[4] = {zero, zero, M31(h[5]), M31(h[5])};
      s += inv(combine_m(rel, air::REL_MERKLE, t));
    }
    {
      const M31 t[4] = {zero, zero, M31(h[6]), M31(h[6])};
      s += inv(combine_m(rel, air::REL_MERKLE, t));
    }
    stq(scr + J[VPF_SUM_OUT], s);
    for (uint32_t c = 0; c < J[VPF_N_CLAIMED]; c++) s += ldq(blob + J[VPF_CLAIMED] + 4 * (size_t)c);
    if (J[VPF_LOGUP_FLAG] != VP_NONE && !s.is_zero()) flags[J[VPF_LOGUP_FLAG]] = 1;
  }
  if (J[VPF_DO_OODS]) {
    QM31 s;
    for (uint32_t c = 0; c < J[VPF_N_QUOT]; c++) s += ldq(scr + J[VPF_QUOT] + 4 * (size_t)c);
    const uint32_t* C4 = blob + J[VPF_COMPOSITION];
    const QM31 c4[4] = {ldq(C4), ldq(C4 + 4), ldq(C4 + 8), ldq(C4 + 12)};
    if (J[VPF_OODS_FLAG] != VP_NONE && s != dev_combine_ef(c4)) flags[J[VPF_OODS_FLAG]] = 1;
  }
}

}  // namespace

void launch_verify_public_sum(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st) {
  if (n_jobs) hipLaunchKernelGGL(k_verify_public_sum, dim3(n_jobs), dim3(VP_SUM_THREADS), 0, st, blob, scr, jobs);
}
void launch_verify_oods(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st) {
  if (!n_jobs) return;
  static_assert(VP_OODS_GROUPS == 4, "one launch per component group");
  launch_verify_oods_group<0>(blob, scr, jobs, n_jobs, st);
  launch_verify_oods_group<1>(blob, scr, jobs, n_jobs, st);
  launch_verify_oods_group<2>(blob, scr, jobs, n_jobs, st);
  launch_verify_oods_group<3>(blob, scr, jobs, n_jobs, st);
}
void launch_verify_prelude_fin(const uint32_t* blob, uint32_t* scr, uint32_t* flags, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st) {
  if (n_jobs) hipLaunchKernelGGL(k_verify_prelude_fin, dim3((n_jobs + FIN_THREADS - 1) / FIN_THREADS), dim3(FIN_THREADS), 0, st, blob, scr, flags, jobs, n_jobs);
}

}  // namespace cm

// ================================================================= op-level entries
using namespace cm;

namespace {
constexpr uint32_t OP_MAX_JOBS = 1u << 16, OP_MAX_LIST = 1u << 24;
void need_device(const char* who) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) throw CmError(3, std::string(who) + ": no HIP device available (libcairom_hip has no CPU fallback)");
  bind_thread_to_library_device();
}
bool words_below_p(const uint32_t* w, size_t n) {
  for (size_t i = 0; i < n; i++) if (w[i] >= P) return false;
  return true;
}
// blob and scratch of an op call (the put / scratch of verify_device.hip's Planner)
struct OpSink {
  std::vector<uint32_t> blob;
  uint64_t scr_words = 0;
  uint32_t put(const uint32_t* p, size_t n) {
    const size_t off = blob.size();
    if (n) blob.insert(blob.end(), p, p + n);
    return (uint32_t)off;
  }
  uint32_t scratch(size_t n) {
    const uint64_t off = scr_words;
    scr_words += n;
    return (uint32_t)off;
  }
};

void check_sum_job(const std::string& who, const cm_public_sum_job& j) {
  CM_CHECK(j.rel_words, who + ": a job without rel_words");
  CM_CHECK(j.n_program <= OP_MAX_LIST && j.n_input <= OP_MAX_LIST && j.n_output <= OP_MAX_LIST, who + ": a list of more than 2^24 entries");
  const size_t n = (size_t)j.n_program + j.n_input + j.n_output;
  CM_CHECK(j.entries || !n, who + ": a job without entries");
  CM_CHECK(words_below_p(j.head, 7), who + ": a head word is not below P");
  CM_CHECK(words_below_p(j.rel_words, VP_REL_WORDS), who + ": a relation word is not below P");
  for (size_t e = 0; e < n; e++) {
    CM_CHECK(j.entries[7 * e] <= 1, who + ": an entry's present word is above 1");
    CM_CHECK(words_below_p(j.entries + 7 * e + 1, 6), who + ": an entry word is not below P");
  }
}
PublicData sum_job_data(const cm_public_sum_job& j) {
  PublicData d;
  d.initial_pc = j.head[0]; d.initial_fp = j.head[1]; d.final_pc = j.head[2]; d.final_fp = j.head[3];
  d.clock = j.head[4]; d.initial_root = j.head[5]; d.final_root = j.head[6];
  const uint32_t* e = j.entries;
  std::vector<PublicEntry>* lists[3] = {&d.program, &d.input, &d.output};
  const uint32_t len[3] = {j.n_program, j.n_input, j.n_output};
  for (int k = 0; k < 3; k++)
    for (uint32_t i = 0; i < len[k]; i++, e += 7) lists[k]->push_back(PublicEntry{e[0], e[1], {e[2], e[3], e[4], e[5]}, e[6]});
  return d;
}
HostRelations relations_from_words(const uint32_t* w) {
  HostRelations rel;
  for (int r = 0; r < air::N_RELATIONS; r++) rel.z[r] = QM31::from_u32(w + 4 * r);
  for (int r = 0; r < air::N_RELATIONS; r++)
    for (int i = 0; i < air::MAX_REL_SIZE; i++) rel.alpha_pow[r][i] = QM31::from_u32(w + 4 * air::N_RELATIONS + 4 * (r * air::MAX_REL_SIZE + i));
  return rel;
}
void check_eval_job(const std::string& who, const cm_point_eval_job& j) {
  CM_CHECK(j.component < (uint32_t)air::N_COMPONENTS, who + ": component id out of range");
  const air::ComponentInfo& info = air::component_info((int)j.component);
  CM_CHECK(j.tr && j.it && j.pp && j.rel_words && j.coeff, who + ": null argument in a job");
  CM_CHECK(j.n_tr_words == 4u * (uint32_t)info.n_trace, who + ": n_tr_words does not match the component's trace columns");
  CM_CHECK(j.n_it_words == 4u * (uint32_t)(info.n_interaction + 4), who + ": n_it_words does not match the component's interaction samples");
  CM_CHECK(j.n_coeff_words == 4u * (uint32_t)info.n_constraints, who + ": n_coeff_words does not match the component's constraints");
  CM_CHECK(words_below_p(j.tr, j.n_tr_words) && words_below_p(j.it, j.n_it_words) && words_below_p(j.pp, 4 * air::N_PREPROC),
           who + ": a mask word is not below P");
  CM_CHECK(words_below_p(j.rel_words, VP_REL_WORDS), who + ": a relation word is not below P");
  CM_CHECK(words_below_p(j.coeff, j.n_coeff_words), who + ": a coefficient word is not below P");
  CM_CHECK(words_below_p(j.shift, 4), who + ": a shift word is not below P");
}
// download n values of 4 words each from scratch offsets
void run_and_fetch(OpSink& sk, const std::vector<uint32_t>& offs, uint32_t* out, hipStream_t st,
                   const std::function<void(const uint32_t*, uint32_t*)>& launch) {
  CM_CHECK(sk.blob.size() < (1u << 30) && sk.scr_words < (1u << 30), "the call is too large (2^30 plan words): split it");
  DevBuf d_blob = upload(sk.blob, st), d_scr(4 * (size_t)std::max<uint64_t>(sk.scr_words, 1));
  launch(d_blob.u32(), d_scr.u32());
  CM_HIP(hipGetLastError());
  std::vector<uint32_t> h((size_t)sk.scr_words);
  CM_HIP(hipMemcpyAsync(h.data(), d_scr.p, 4 * h.size(), hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
  for (size_t k = 0; k < offs.size(); k++) memcpy(out + 4 * k, h.data() + offs[k], 16);
}
}  // namespace

extern "C" {

int32_t cm_public_logup_sum_host(const cm_public_sum_job* job, uint32_t out4[4]) {
  return abi_guard([&] {
    CM_CHECK(job && out4, "cm_public_logup_sum_host: null argument");
    check_sum_job("cm_public_logup_sum_host", *job);
    verif::initial_logup_sum(sum_job_data(*job), relations_from_words(job->rel_words)).to_u32(out4);
  });
}

int32_t cm_public_logup_sum_op(const cm_public_sum_job* jobs, uint32_t n_jobs, cm_stream_t s, uint32_t* out) {
  return abi_guard([&] {
    CM_CHECK(jobs && out, "cm_public_logup_sum_op: null argument");
    CM_CHECK(n_jobs >= 1 && n_jobs <= OP_MAX_JOBS, "cm_public_logup_sum_op: n_jobs outside 1..65536");
    for (uint32_t j = 0; j < n_jobs; j++) check_sum_job("cm_public_logup_sum_op", jobs[j]);
    need_device("cm_public_logup_sum_op");
    OpSink sk;
    std::vector<uint32_t> sum_jobs, fin_jobs, offs;
    for (uint32_t j = 0; j < n_jobs; j++) {
      uint32_t fin[VP_FIN_JOB_WORDS] = {0};
      const uint32_t rel_off = sk.put(jobs[j].rel_words, VP_REL_WORDS);
      plan_public_sum(sk, sum_job_data(jobs[j]), rel_off, sum_jobs, fin);
      fin[VPF_LOGUP_FLAG] = VP_NONE;
      fin_jobs.insert(fin_jobs.end(), fin, fin + VP_FIN_JOB_WORDS);
      offs.push_back(fin[VPF_SUM_OUT]);
    }
    const uint32_t n_sum = (uint32_t)(sum_jobs.size() / VP_SUM_JOB_WORDS);
    const uint32_t sum_off = sk.put(sum_jobs.data(), sum_jobs.size()), fin_off = sk.put(fin_jobs.data(), fin_jobs.size());
    const hipStream_t st = as_stream(s);
    run_and_fetch(sk, offs, out, st, [&](const uint32_t* blob, uint32_t* scr) {
      launch_verify_public_sum(blob, scr, blob + sum_off, n_sum, st);
      launch_verify_prelude_fin(blob, scr, nullptr, blob + fin_off, n_jobs, st);
    });
  });
}

int32_t cm_point_eval_host(const cm_point_eval_job* job, uint32_t out4[4]) {
  return abi_guard([&] {
    CM_CHECK(job && out4, "cm_point_eval_host: null argument");
    check_eval_job("cm_point_eval_host", *job);
    const air::ComponentInfo& info = air::component_info((int)job->component);
    auto felts = [](const uint32_t* w, size_t n_words) {
      std::vector<QM31> v(n_words / 4);
      for (size_t k = 0; k < v.size(); k++) v[k] = QM31::from_u32(w + 4 * k);
      return v;
    };
    const std::vector<QM31> tr = felts(job->tr, job->n_tr_words), it = felts(job->it, job->n_it_words), pp = felts(job->pp, 4 * air::N_PREPROC),
                            coeff = felts(job->coeff, job->n_coeff_words);
    point_eval((int)job->component, tr.data(), it.data(), pp.data(), relations_from_words(job->rel_words), coeff.data(), info.n_base_constraints,
               QM31::from_u32(job->shift)).to_u32(out4);
  });
}

int32_t cm_point_eval_op(const cm_point_eval_job* jobs, uint32_t n_jobs, cm_stream_t s, uint32_t* out) {
  return abi_guard([&] {
    CM_CHECK(jobs && out, "cm_point_eval_op: null argument");
    CM_CHECK(n_jobs >= 1 && n_jobs <= OP_MAX_JOBS, "cm_point_eval_op: n_jobs outside 1..65536");
    for (uint32_t j = 0; j < n_jobs; j++) check_eval_job("cm_point_eval_op", jobs[j]);
    need_device("cm_point_eval_op");
    OpSink sk;
    std::vector<uint32_t> oods_jobs, offs;
    for (uint32_t j = 0; j < n_jobs; j++) {
      const cm_point_eval_job& q = jobs[j];
      const uint32_t job[VP_OODS_JOB_WORDS] = {q.component, (uint32_t)air::component_info((int)q.component).n_base_constraints,
                                               sk.put(q.tr, q.n_tr_words), sk.put(q.it, q.n_it_words), sk.put(q.pp, 4 * air::N_PREPROC),
                                               sk.put(q.rel_words, VP_REL_WORDS), sk.put(q.coeff, q.n_coeff_words), sk.put(q.shift, 4),
                                               0, 0, sk.scratch(4), 0};
      oods_jobs.insert(oods_jobs.end(), job, job + VP_OODS_JOB_WORDS);
      offs.push_back(job[10]);
    }
    const uint32_t jobs_off = sk.put(oods_jobs.data(), oods_jobs.size());
    const hipStream_t st = as_stream(s);
    run_and_fetch(sk, offs, out, st, [&](const uint32_t* blob, uint32_t* scr) { launch_verify_oods(blob, scr, blob + jobs_off, n_jobs, st); });
  });
}

}  // extern "C"
