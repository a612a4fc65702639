// cm_verify_many: the query phase of verify_cairo_m for a whole batch of proofs on the GPU (plan format: verify_device.hpp).
// Host: verify_prelude + a symbolic walk of merkle_verify / rebuild_evals per proof.  Device: k_verify_answers (DEEP quotients),
// k_verify_fri (pairs, folds, last layer), k_verify_merkle (every tree of every proof), k_verify_reduce (lowest failed check).
// With CM_VERIFY_ARITH_ON_DEVICE the prelude's LogUp sum and OODS check are deferred into the first two slots (verify_prelude.hpp).
// cm_verify_plan_stats and cm_verify_many_detail read what the same Planner built (shapes; every slot's own flag) for the tests.
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "blake2s_dev.hpp"
#include "verifier_common.hpp"
#include "verify_device.hpp"
#include "verify_prelude.hpp"
#include <chrono>
#include <memory>

namespace cm {

namespace {

constexpr uint32_t REF_SCRATCH = 0x80000000u;   // bit 31 of a reference: scratch buffer (or, for a child, hash witness) instead
constexpr uint32_t ANS_THREADS = 256, FRI_THREADS = 128, MERKLE_THREADS = 256;
// FRI program header words
enum : uint32_t { VF_N_GROUPS = 0, VF_GROUPS, VF_N_LAYERS, VF_LAYERS, VF_CIRCLE_ALPHA, VF_DO_LAST = 8, VF_LAST_NPOS, VF_LAST_POS, VF_LAST_LOG,
                  VF_POLY, VF_POLY_LOG, VF_LAST_FLAG, VF_EV0, VF_EV1, VF_N_EV0, VF_WORDS };
constexpr uint32_t VF_GROUP_WORDS = 6, VF_LAYER_WORDS = 12;

// ================================================================= device
__device__ __forceinline__ QM31 ldq(const uint32_t* p) { return QM31::from_u32(p); }
__device__ __forceinline__ void stq(uint32_t* p, const QM31& v) { v.to_u32(p); }
__device__ __forceinline__ const uint32_t* ref_ptr(const uint32_t* blob, const uint32_t* scr, uint32_t ref) {
  return (ref & REF_SCRATCH) ? scr + (ref & ~REF_SCRATCH) : blob + ref;
}
__device__ __forceinline__ CPoint<M31> dev_domain_point(uint32_t log, uint32_t row) {
  return point_at_index(domain_index_at(log, bit_reverse(row, log)));
}
// x of LineDomain(half_odds(log)) at bit-reversed position pos
__device__ __forceinline__ M31 dev_line_x(uint32_t log, uint32_t pos) {
  const uint32_t idx = subgroup_gen_index(log + 2) + subgroup_gen_index(log) * bit_reverse(pos, log);
  return point_at_index(idx).x;
}
// sum of one QM31 per thread over the workgroup; the total is returned to thread 0 (red: 4 words per thread)
template <uint32_t N>
__device__ __forceinline__ QM31 block_sum(QM31 v, uint32_t* red, uint32_t tid) {
  __syncthreads();   // the previous use of `red` is over
  stq(red + 4 * tid, v);
  __syncthreads();
  for (uint32_t s = N / 2; s > 0; s >>= 1) {
    if (tid < s) stq(red + 4 * tid, ldq(red + 4 * tid) + ldq(red + 4 * (tid + s)));
    __syncthreads();
  }
  return ldq(red);
}

// One workgroup per (proof, size group, query row): Stwo's accumulate_row_quotients for that row (verifier_common.hpp
// row_quotient), the numerator of a batch summed across the columns by the workgroup, one denominator inverse per (row, batch).
__global__ __launch_bounds__(ANS_THREADS) void k_verify_answers(const uint32_t* __restrict__ blob, uint32_t* __restrict__ scr,
                                                                const uint32_t* __restrict__ jobs) {
  __shared__ uint32_t red[4 * ANS_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t* J = jobs + 8 * (size_t)blockIdx.x;
  const uint32_t* G = blob + J[0];
  const uint32_t n_batches = G[0];
  const QM31 alpha = ldq(G + 1);
  const CPoint<M31> p = dev_domain_point(J[5], J[6]);
  const QM31 pw0 = qpow(alpha, tid + 1), step = qpow(alpha, ANS_THREADS);
  QM31 acc;
  for (uint32_t b = 0; b < n_batches; b++) {
    const uint32_t* B = G + 5 + 10 * b;
    const QM31 ptx = ldq(B), pty = ldq(B + 4);
    const uint32_t n = B[8];
    const uint32_t* E = blob + B[9];
    const QM31 cdiff = conj_u(pty) - pty;
    QM31 num, pw = pw0;
    for (uint32_t e = tid; e < n; e += ANS_THREADS) {
      const uint32_t* X = E + 5 * (size_t)e;
      const uint32_t tk = X[0];
      const QM31 v = ldq(X + 1);
      const M31 rv(blob[J[1 + (tk >> 28)] + (tk & 0x0fffffffu)]);
      const QM31 a = conj_u(v) - v;
      const QM31 bb = v * cdiff - a * pty;
      num += pw * (cdiff * rv - (a * p.y + bb));
      pw = pw * step;
    }
    const QM31 total = block_sum<ANS_THREADS>(num, red, tid);
    if (tid == 0) {
      const CM31 den = (ptx.a - CM31(p.x)) * pty.b - (pty.a - CM31(p.y)) * ptx.b;
      acc = acc * qpow(alpha, n) + mul_cm31(total, inv(den));
    }
  }
  if (tid == 0) stq(scr + J[7], acc);
}

// One workgroup per proof walks the FRI layers: first-layer pairs from answers and witness, folded with circle_alpha; every inner
// layer accumulates the folded columns of its size, rebuilds its pairs, folds with its alpha.  Every layer's pair values are written
// out (they are the leaf values of that layer's tree: k_verify_merkle); the last layer's polynomial is evaluated at what is left.
__global__ __launch_bounds__(FRI_THREADS) void k_verify_fri(const uint32_t* __restrict__ blob, uint32_t* scr, uint32_t* __restrict__ flags,
                                                            const uint32_t* __restrict__ jobs) {
  __shared__ uint32_t red[4 * FRI_THREADS];
  const uint32_t tid = threadIdx.x;
  const uint32_t* F = blob + jobs[blockIdx.x];
  const QM31 circle_alpha = ldq(F + VF_CIRCLE_ALPHA);
  const QM31 a2 = circle_alpha * circle_alpha;
  const uint32_t n_groups = F[VF_N_GROUPS], n_layers = F[VF_N_LAYERS];
  for (uint32_t g = 0; g < n_groups; g++) {
    const uint32_t* GR = blob + F[VF_GROUPS] + VF_GROUP_WORDS * g;
    const uint32_t log = GR[0], n_pairs = GR[1];
    const uint32_t* slots = blob + GR[2];
    for (uint32_t s = tid; s < n_pairs; s += FRI_THREADS) {
      const QM31 v0 = ldq(ref_ptr(blob, scr, slots[3 * s + 1])), v1 = ldq(ref_ptr(blob, scr, slots[3 * s + 2]));
      stq(scr + GR[3] + 8 * s, v0);
      stq(scr + GR[3] + 8 * s + 4, v1);
      const CPoint<M31> p = dev_domain_point(log, slots[3 * s]);
      stq(scr + GR[4] + 4 * s, (v0 + v1) + circle_alpha * ((v0 - v1) * inv(p.y)));
    }
  }
  for (uint32_t i = tid; i < F[VF_N_EV0]; i += FRI_THREADS) stq(scr + F[VF_EV0] + 4 * i, QM31());
  __syncthreads();
  for (uint32_t li = 0; li < n_layers; li++) {
    const uint32_t* LR = blob + F[VF_LAYERS] + VF_LAYER_WORDS * li;
    uint32_t* ev = scr + F[(li & 1) ? VF_EV1 : VF_EV0];
    uint32_t* nxt = scr + F[(li & 1) ? VF_EV0 : VF_EV1];
    const uint32_t layer_log = LR[0], n_pairs = LR[1], n_add = LR[8], add_first = LR[9], n_evals = LR[10];
    if (n_add) {
      for (uint32_t i = tid; i < n_evals; i += FRI_THREADS) {
        QM31 e = ldq(ev + 4 * i);
        for (uint32_t k = 0; k < n_add; k++) {
          const uint32_t* GR = blob + F[VF_GROUPS] + VF_GROUP_WORDS * (add_first + k);
          e = e * a2 + ldq(scr + GR[4] + 4 * i);
        }
        stq(ev + 4 * i, e);
      }
      __syncthreads();
    }
    const uint32_t* slots = blob + LR[2];
    const QM31 alpha = ldq(LR + 4);
    for (uint32_t s = tid; s < n_pairs; s += FRI_THREADS) {
      const QM31 v0 = ldq(ref_ptr(blob, scr, slots[3 * s + 1])), v1 = ldq(ref_ptr(blob, scr, slots[3 * s + 2]));
      stq(scr + LR[3] + 8 * s, v0);
      stq(scr + LR[3] + 8 * s + 4, v1);
      const M31 x = dev_line_x(layer_log, slots[3 * s]);
      stq(nxt + 4 * s, (v0 + v1) + alpha * ((v0 - v1) * inv(x)));
    }
    __syncthreads();
  }
  if (!F[VF_DO_LAST]) return;
  const uint32_t* ev = scr + F[(n_layers & 1) ? VF_EV1 : VF_EV0];
  const uint32_t n_pos = F[VF_LAST_NPOS], last_log = F[VF_LAST_LOG], poly_log = F[VF_POLY_LOG];
  const uint32_t* poly = blob + F[VF_POLY];
  for (uint32_t i = 0; i < n_pos; i++) {
    const M31 x = dev_line_x(last_log, blob[F[VF_LAST_POS] + i]);
    QM31 part;
    for (uint32_t j = tid; j < (1u << poly_log); j += FRI_THREADS) {
      QM31 term = ldq(poly + 4 * (size_t)j);
      M31 cur = x;
      for (uint32_t b = 0; b < poly_log; b++) { if ((j >> (poly_log - 1 - b)) & 1) term = term * cur; cur = double_x(cur); }
      part += term;
    }
    const QM31 v = block_sum<FRI_THREADS>(part, red, tid);
    if (tid == 0 && v != ldq(ev + 4 * i)) flags[F[VF_LAST_FLAG]] = 1;
  }
}

// One workgroup per (proof, tree) — the four commitment trees, the first FRI layer's tree and every inner layer's — walks its
// node list from the largest layer to the root: a thread per node, both levels' hashes in LDS, a barrier between levels.  A
// node's compressions depend on each other in both framings (chained state), so the parallelism is across nodes, trees and proofs.
template <bool RFC>
__global__ __launch_bounds__(MERKLE_THREADS) void k_verify_merkle(const uint32_t* __restrict__ blob, const uint32_t* __restrict__ scr,
                                                                  uint32_t* __restrict__ flags, const uint32_t* __restrict__ jobs, uint32_t cap) {
  extern __shared__ uint32_t lds[];   // 2 levels x cap nodes x 8 words
  const uint32_t tid = threadIdx.x;
  const uint32_t* J = jobs + 8 * (size_t)blockIdx.x;
  const uint32_t n_levels = J[0];
  uint32_t* prev = lds;
  uint32_t* cur = lds + 8 * (size_t)cap;
  for (uint32_t lv = 0; lv < n_levels; lv++) {
    const uint32_t* L = blob + J[1] + 4 * lv;
    const uint32_t n = L[0], nc = L[2];
    const bool has_prev = L[3] != 0;
    const uint32_t* nodes = blob + L[1];
    for (uint32_t i = tid; i < n; i += MERKLE_THREADS) {
      const uint32_t* R = nodes + 3 * (size_t)i;
      NodeFrame<RFC> fr(has_prev, nc);
      uint32_t h[8], m[16];
      fr.init(h);
      if (has_prev) {
        const uint32_t* l = (R[0] & REF_SCRATCH) ? blob + (R[0] & ~REF_SCRATCH) : prev + 8 * R[0];
        const uint32_t* r = (R[1] & REF_SCRATCH) ? blob + (R[1] & ~REF_SCRATCH) : prev + 8 * R[1];
#pragma unroll
        for (int k = 0; k < 8; k++) { m[k] = l[k]; m[8 + k] = r[k]; }
        fr.absorb(h, m, 64);
      }
      const uint32_t* v = ref_ptr(blob, scr, R[2]);
      for (uint32_t c0 = 0; c0 < nc; c0 += 16) {
#pragma unroll
        for (uint32_t k = 0; k < 16; k++) m[k] = c0 + k < nc ? v[c0 + k] : 0u;
        fr.absorb(h, m, 4 * (nc - c0 < 16 ? nc - c0 : 16));
      }
#pragma unroll
      for (int k = 0; k < 8; k++) cur[8 * i + k] = h[k];
    }
    __syncthreads();
    uint32_t* t = prev; prev = cur; cur = t;
  }
  if (tid == 0) {
    const uint32_t* root = blob + J[2];
    bool same = true;
    for (int k = 0; k < 8; k++) same = same && prev[k] == root[k];
    if (!same) flags[J[3]] = 1;
  }
}

// per proof: the lowest raised flag (its slot number), or 0xffffffff
__global__ void k_verify_reduce(const uint32_t* __restrict__ flags, const uint32_t* __restrict__ jobs, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t base = jobs[2 * i], cnt = jobs[2 * i + 1];
  uint32_t r = 0xffffffffu;
  for (uint32_t k = cnt; k-- > 0;) if (flags[base + k]) r = k;
  out[i] = r;
}

// ================================================================= host: the plan
using namespace verif;

struct Slot { int32_t check; std::string message; };
struct ProofPlan {
  std::vector<Slot> slots;     // the checks of the query phase in the host verifier's order; slot k owns flag flag_base + k
  int fail_slot = -1;          // the slot that failed while planning (always the last one)
  uint32_t flag_base = 0;
  VerifyOutcome early;         // a failure in front of the queries
  bool decided_early = false;
};

struct Planner {
  std::vector<uint32_t> blob;
  uint64_t scr_words = 0;
  uint32_t n_flags = 0, max_level_nodes = 1;
  std::vector<uint32_t> ans_jobs, fri_jobs, tree_jobs;
  PreludeMarks* marks = nullptr;   // cm_verify_plan_stats under CM_VERIFY_PLAN_MARKS; null everywhere else
  std::vector<uint32_t> sum_jobs, fin_jobs, oods_jobs[air::N_COMPONENTS];   // the deferred arithmetic; oods jobs are sent component-major

  uint32_t put(const uint32_t* p, size_t n) {
    const size_t off = blob.size();
    blob.insert(blob.end(), p, p + n);
    return (uint32_t)off;
  }
  uint32_t put(const std::vector<uint32_t>& v) { return put(v.data(), v.size()); }
  uint32_t put_q(const QM31* p, size_t n) {
    static_assert(sizeof(QM31) == 16, "QM31 is four canonical words");
    return put(reinterpret_cast<const uint32_t*>(p), 4 * n);
  }
  uint32_t put_hash(const Hash32& h) {
    uint32_t w[8];
    memcpy(w, h.data(), 32);
    return put(w, 8);
  }
  uint32_t scratch(size_t n) {
    const uint64_t off = scr_words;
    scr_words += n;
    return (uint32_t)off;
  }
  struct DecRef { uint32_t hw_off, n_hw, cw_off, n_cw; };
  DecRef put_dec(const MerkleDecommitment& d) {
    DecRef r;
    r.n_hw = (uint32_t)d.hash_witness.size();
    r.hw_off = put(reinterpret_cast<const uint32_t*>(d.hash_witness.data()), 8 * d.hash_witness.size());
    r.n_cw = (uint32_t)d.column_witness.size();
    r.cw_off = put(d.column_witness);
    return r;
  }

  // merkle_verify (verifier_common.hpp) without the hashes: the node list of the tree, or the structural failure
  std::string plan_tree(const std::vector<uint32_t>& col_logs, const std::map<uint32_t, std::vector<uint32_t>>& queries, size_t n_qv,
                        uint32_t qv_ref, const DecRef& d, uint32_t root_off, uint32_t flag) {
    if (col_logs.empty()) return "empty tree";
    const uint32_t max_log = *std::max_element(col_logs.begin(), col_logs.end());
    std::map<uint32_t, uint32_t> n_cols;
    for (auto l : col_logs) n_cols[l]++;
    size_t qi = 0, hi = 0, ci = 0;
    std::vector<uint32_t> last, cur, recs, levels;
    for (int log = (int)max_log; log >= 0; log--) {
      const uint32_t nc = n_cols.count((uint32_t)log) ? n_cols[(uint32_t)log] : 0;
      static const std::vector<uint32_t> none;
      auto it = queries.find((uint32_t)log);
      const std::vector<uint32_t>& colq = (nc && it != queries.end()) ? it->second : none;
      cur.clear();
      recs.clear();
      size_t pi = 0, cq = 0;
      const bool has_prev = log < (int)max_log;
      while (pi < last.size() || cq < colq.size()) {
        uint32_t node;
        if (pi < last.size() && cq < colq.size()) node = std::min(last[pi] / 2, colq[cq]);
        else if (pi < last.size()) node = last[pi] / 2;
        else node = colq[cq];
        uint32_t l = 0, r = 0, v;
        if (has_prev) {
          if (pi < last.size() && last[pi] == 2 * node) l = (uint32_t)pi++;
          else { if (hi >= d.n_hw) return "WitnessTooShort"; l = REF_SCRATCH | (uint32_t)(d.hw_off + 8 * hi++); }
          if (pi < last.size() && last[pi] == 2 * node + 1) r = (uint32_t)pi++;
          else { if (hi >= d.n_hw) return "WitnessTooShort"; r = REF_SCRATCH | (uint32_t)(d.hw_off + 8 * hi++); }
        }
        const bool isq = cq < colq.size() && colq[cq] == node;
        if (isq) {
          cq++;
          if (qi + nc > n_qv) return "TooFewQueriedValues";
          v = qv_ref + (uint32_t)qi;
          qi += nc;
        } else {
          if (ci + nc > d.n_cw) return "WitnessTooShort";
          v = d.cw_off + (uint32_t)ci;
          ci += nc;
        }
        cur.push_back(node);
        recs.push_back(l); recs.push_back(r); recs.push_back(v);
      }
      max_level_nodes = std::max<uint32_t>(max_level_nodes, (uint32_t)cur.size());
      const uint32_t nodes_off = put(recs);
      levels.push_back((uint32_t)cur.size()); levels.push_back(nodes_off); levels.push_back(nc); levels.push_back(has_prev ? 1u : 0u);
      last.swap(cur);
    }
    if (hi != d.n_hw || ci != d.n_cw) return "WitnessTooLong";
    if (qi != n_qv) return "TooManyQueriedValues";
    if (last.size() != 1) return "RootMismatch";
    const uint32_t levels_off = put(levels);
    const uint32_t job[8] = {(uint32_t)(levels.size() / 4), levels_off, root_off, flag, 0, 0, 0, 0};
    tree_jobs.insert(tree_jobs.end(), job, job + 8);
    return "";
  }

  // rebuild_evals (verifier_common.hpp) over references: slots = [start, source of value 0, source of value 1] per pair
  static bool plan_rebuild(const std::vector<uint32_t>& queries, uint32_t evals_ref, size_t n_witness, uint32_t wit_off, size_t& wi,
                           std::vector<uint32_t>& positions, std::vector<uint32_t>& slots) {
    size_t i = 0;
    while (i < queries.size()) {
      const uint32_t start = (queries[i] >> 1) << 1;
      size_t j = i;
      while (j < queries.size() && (queries[j] >> 1) == (queries[i] >> 1)) j++;
      size_t qi = i;
      slots.push_back(start);
      for (uint32_t k = 0; k < 2; k++) {
        positions.push_back(start + k);
        if (qi < j && queries[qi] == start + k) slots.push_back(evals_ref + 4 * (uint32_t)qi++);
        else { if (wi >= n_witness) return false; slots.push_back(wit_off + 4 * (uint32_t)wi++); }
      }
      i = j;
    }
    return true;
  }

  // The OODS composition check as one job per component (verify_prelude.hpp) and the OODS half of the proof's fin job.  The
  // coefficient powers are the host's table, built as verify_prelude builds it; the sampled values have their shape (stage 2).
  void plan_oods(const ProofData& pf, const DeferredArith& da, uint32_t rel_off, uint32_t flag, uint32_t* fin) {
    size_t total = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) total += air::component_info(c).n_constraints;
    std::vector<QM31> powers(total), flat;
    QM31 cur(M31(1));
    for (size_t g = total; g-- > 0;) { powers[g] = cur; cur = cur * da.random_coeff; }
    const uint32_t coeff_off = put_q(powers.data(), powers.size());
    for (int i = 0; i < air::N_PREPROC; i++) flat.push_back(pf.sampled_values[0][i][0]);
    const uint32_t pp_off = put_q(flat.data(), flat.size());
    flat.clear();
    for (auto& col : pf.sampled_values[1]) flat.push_back(col[0]);
    const uint32_t tr_off = put_q(flat.data(), flat.size());
    flat.clear();
    std::vector<uint32_t> it_first(pf.sampled_values[2].size());   // a column's first sample in the flat list
    for (size_t k = 0; k < pf.sampled_values[2].size(); k++) {
      it_first[k] = (uint32_t)flat.size();
      for (auto& v : pf.sampled_values[2][k]) flat.push_back(v);
    }
    const uint32_t it_off = put_q(flat.data(), flat.size());
    flat.clear();
    for (int c = 0; c < air::N_COMPONENTS; c++) flat.push_back(pf.claimed_sums[c] * inv(M31::from_u32(1u << pf.claim_log_sizes[c])));
    const uint32_t shift_off = put_q(flat.data(), flat.size());
    const uint32_t oods_off = put_q(&da.oods.x, 1);
    const QM31 c4[4] = {pf.sampled_values[3][0][0], pf.sampled_values[3][1][0], pf.sampled_values[3][2][0], pf.sampled_values[3][3][0]};
    const uint32_t quot = scratch(4 * air::N_COMPONENTS);
    size_t g = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      const air::ComponentInfo& info = air::component_info(c);
      const uint32_t job[VP_OODS_JOB_WORDS] = {(uint32_t)c, (uint32_t)info.n_base_constraints, tr_off + 4 * (uint32_t)da.tr0[c],
                                               it_off + 4 * it_first[da.it0[c]], pp_off, rel_off, coeff_off + 4 * (uint32_t)g,
                                               shift_off + 4 * (uint32_t)c, pf.claim_log_sizes[c], oods_off, quot + 4 * (uint32_t)c, 0};
      oods_jobs[c].insert(oods_jobs[c].end(), job, job + VP_OODS_JOB_WORDS);
      g += info.n_constraints;
    }
    fin[VPF_DO_OODS] = 1;
    fin[VPF_QUOT] = quot;
    fin[VPF_N_QUOT] = air::N_COMPONENTS;
    fin[VPF_COMPOSITION] = put_q(c4, 4);
    fin[VPF_OODS_FLAG] = flag;
  }

  // arith_on_device: the LogUp sum and the OODS check are the proof's first two slots, decided by the prelude kernels
  void plan_proof(const ProofData& pf, const cm_pcs_config& cfg, ProofPlan& pp, bool arith_on_device = false) {
    VerifyPrelude pre;
    std::unique_ptr<DeferredArith> deferred(arith_on_device ? new DeferredArith() : nullptr);   // the default mode builds none
    int32_t check = 0;
    const std::string err = verify_prelude(pf, cfg, pre, &check, deferred.get(), marks);
    const int stage = deferred ? deferred->stage : 0;
    if (!err.empty() && stage == 0) { pp.decided_early = true; pp.early.check = check; pp.early.message = err; return; }
    const auto& logs = pre.logs;
    const auto& pts = pre.pts;
    const auto& q_logs = pre.q_logs;
    auto& qpos = pre.qpos;
    pp.flag_base = n_flags;
    auto device_slot = [&](int32_t check, const std::string& msg) { pp.slots.push_back(Slot{check, msg}); return n_flags++; };
    auto host_fail = [&](int32_t check, const std::string& msg) { pp.fail_slot = (int)pp.slots.size(); pp.slots.push_back(Slot{check, msg}); n_flags++; };
    if (stage >= 1) {
      const DeferredArith& da = *deferred;
      uint32_t fin[VP_FIN_JOB_WORDS] = {0};
      uint32_t rel_words[VP_REL_WORDS];
      relations_words(da.rel, rel_words);
      const uint32_t rel_off = put(rel_words, VP_REL_WORDS);
      plan_public_sum(*this, pf.public_data, rel_off, sum_jobs, fin);
      fin[VPF_CLAIMED] = put_q(pf.claimed_sums.data(), pf.claimed_sums.size());
      fin[VPF_N_CLAIMED] = (uint32_t)pf.claimed_sums.size();
      fin[VPF_LOGUP_FLAG] = device_slot(CM_VERIFY_LOGUP_SUM, "InvalidLogupSum");
      if (da.stage >= 2) plan_oods(pf, da, rel_off, device_slot(CM_VERIFY_OODS, "OodsNotMatching"), fin);
      fin_jobs.insert(fin_jobs.end(), fin, fin + VP_FIN_JOB_WORDS);
      if (!err.empty()) return host_fail(check, err);   // a host check behind a deferred one: nothing more is sent
    }

    // ---- the four commitment trees
    uint32_t qv_off[4];
    for (int t = 0; t < 4; t++) qv_off[t] = put(pf.queried_values[t]);
    for (int t = 0; t < 4; t++) {
      std::vector<uint32_t> e;
      for (auto l : logs[t]) e.push_back(l + cfg.log_blowup_factor);
      const DecRef d = put_dec(pf.decommitments[t]);
      const uint32_t root = put_hash(pf.commitments[t]);
      const std::string name = "Merkle(tree " + std::to_string(t) + "): ";
      const std::string err = plan_tree(e, qpos, pf.queried_values[t].size(), qv_off[t], d, root, n_flags);
      if (!err.empty()) return host_fail(CM_VERIFY_MERKLE, name + err);
      device_slot(CM_VERIFY_MERKLE, name + "RootMismatch");
    }
    // ---- fri_answers: one job per (size group, query row)
    std::vector<size_t> cursor(4, 0);
    std::vector<uint32_t> ans_off(q_logs.size());
    for (size_t k = 0; k < q_logs.size(); k++) {
      const uint32_t l = q_logs[k];
      std::vector<std::vector<Sample>> cols;
      std::vector<uint32_t> col_tk;
      std::vector<size_t> ncols(4, 0);
      for (int t = 0; t < 4; t++)
        for (size_t c = 0; c < logs[t].size(); c++)
          if (logs[t][c] + cfg.log_blowup_factor == l) {
            col_tk.push_back(((uint32_t)t << 28) | (uint32_t)ncols[t]);
            ncols[t]++;
            std::vector<Sample> s;
            for (size_t j = 0; j < pts[t][c].size(); j++) s.push_back(Sample{pts[t][c][j], pf.sampled_values[t][c][j]});
            cols.push_back(s);
          }
      const std::vector<SampleBatch> batches = sample_batches(cols);
      std::vector<uint32_t> table(5 + 10 * batches.size());
      table[0] = (uint32_t)batches.size();
      pre.qcoeff.to_u32(&table[1]);
      for (size_t b = 0; b < batches.size(); b++) {
        std::vector<uint32_t> ent(5 * batches[b].entries.size());
        for (size_t e = 0; e < batches[b].entries.size(); e++) {
          ent[5 * e] = col_tk[batches[b].entries[e].first];
          batches[b].entries[e].second.to_u32(&ent[5 * e + 1]);
        }
        uint32_t* B = &table[5 + 10 * b];
        batches[b].pt.x.to_u32(B);
        batches[b].pt.y.to_u32(B + 4);
        B[8] = (uint32_t)batches[b].entries.size();
        B[9] = put(ent);
      }
      const uint32_t table_off = put(table);
      ans_off[k] = scratch(4 * qpos[l].size());
      for (size_t i = 0; i < qpos[l].size(); i++) {
        uint32_t job[8] = {table_off, 0, 0, 0, 0, l, qpos[l][i], ans_off[k] + 4 * (uint32_t)i};
        for (int t = 0; t < 4; t++) {
          if (cursor[t] + ncols[t] > pf.queried_values[t].size()) return host_fail(CM_VERIFY_QUERIED_VALUES, "InvalidStructure(queried values)");
          job[1 + t] = qv_off[t] + (uint32_t)cursor[t];
          cursor[t] += ncols[t];
        }
        ans_jobs.insert(ans_jobs.end(), job, job + 8);
      }
    }
    // ---- FRI first layer
    std::vector<uint32_t> fri(VF_WORDS, 0), groups, layers;
    std::vector<uint32_t> group_pairs;
    pre.circle_alpha.to_u32(&fri[VF_CIRCLE_ALPHA]);
    auto finish_fri = [&]() {   // the program as far as it was planned
      fri[VF_N_GROUPS] = (uint32_t)(groups.size() / VF_GROUP_WORDS);
      fri[VF_GROUPS] = put(groups);
      fri[VF_N_LAYERS] = (uint32_t)(layers.size() / VF_LAYER_WORDS);
      fri[VF_LAYERS] = put(layers);
      fri_jobs.push_back(put(fri));
    };
    {
      size_t wi = 0, n_pairs_total = 0;
      const uint32_t wit_off = put_q(pf.fri_first.fri_witness.data(), pf.fri_first.fri_witness.size());
      std::map<uint32_t, std::vector<uint32_t>> dpos;
      std::vector<uint32_t> col_logs;
      std::vector<std::vector<uint32_t>> slots(q_logs.size());
      for (size_t k = 0; k < q_logs.size(); k++) {
        const uint32_t l = q_logs[k];
        std::vector<uint32_t> positions;
        if (!plan_rebuild(qpos[l], REF_SCRATCH | ans_off[k], pf.fri_first.fri_witness.size(), wit_off, wi, positions, slots[k]))
          return host_fail(CM_VERIFY_FRI_FIRST_EVALS, "Fri(FirstLayerEvaluationsInvalid)");
        dpos[l] = positions;
        col_logs.insert(col_logs.end(), 4, l);
        n_pairs_total += slots[k].size() / 3;
      }
      if (wi != pf.fri_first.fri_witness.size()) return host_fail(CM_VERIFY_FRI_FIRST_EVALS, "Fri(FirstLayerEvaluationsInvalid)");
      const uint32_t dvals = scratch(8 * n_pairs_total);
      size_t done = 0;
      for (size_t k = 0; k < q_logs.size(); k++) {
        const uint32_t np = (uint32_t)(slots[k].size() / 3);
        const uint32_t g[VF_GROUP_WORDS] = {q_logs[k], np, put(slots[k]), dvals + 8 * (uint32_t)done, scratch(4 * (size_t)np), 0};
        groups.insert(groups.end(), g, g + VF_GROUP_WORDS);
        group_pairs.push_back(np);
        done += np;
      }
      const DecRef d = put_dec(pf.fri_first.decommitment);
      const uint32_t root = put_hash(pf.fri_first.commitment);
      const std::string err = plan_tree(col_logs, dpos, 8 * n_pairs_total, REF_SCRATCH | dvals, d, root, n_flags);
      if (!err.empty()) return host_fail(CM_VERIFY_FRI_FIRST_COMMITMENT, "Fri(FirstLayerCommitmentInvalid): " + err);
      device_slot(CM_VERIFY_FRI_FIRST_COMMITMENT, "Fri(FirstLayerCommitmentInvalid): RootMismatch");
    }
    // ---- inner layers
    FoldQueries lq = pre.queries.fold(1);
    size_t n_evals = lq.positions.size(), col = 0;
    uint32_t layer_log = q_logs[0] - 1;
    {
      size_t cap = n_evals;   // the evaluations only shrink from layer to layer
      fri[VF_EV0] = scratch(4 * cap);
      fri[VF_EV1] = scratch(4 * cap);
      fri[VF_N_EV0] = (uint32_t)n_evals;
    }
    for (size_t li = 0; li < pf.fri_inner.size(); li++, layer_log--) {
      const size_t add_first = col;
      while (col < q_logs.size() && q_logs[col] - 1 == layer_log) {
        if (group_pairs[col] != n_evals) { finish_fri(); return host_fail(CM_VERIFY_FRI_INNER_EVALS, "Fri(InnerLayerEvaluationsInvalid)"); }
        col++;
      }
      const FriLayerProofData& lp = pf.fri_inner[li];
      size_t wi = 0;
      std::vector<uint32_t> positions, slots;
      const uint32_t wit_off = put_q(lp.fri_witness.data(), lp.fri_witness.size());
      if (!plan_rebuild(lq.positions, REF_SCRATCH | fri[(li & 1) ? VF_EV1 : VF_EV0], lp.fri_witness.size(), wit_off, wi, positions, slots) ||
          wi != lp.fri_witness.size()) {
        finish_fri();
        return host_fail(CM_VERIFY_FRI_INNER_EVALS, "Fri(InnerLayerEvaluationsInvalid)");
      }
      const uint32_t np = (uint32_t)(slots.size() / 3);
      const uint32_t dvals = scratch(8 * (size_t)np);
      std::map<uint32_t, std::vector<uint32_t>> dpos;
      dpos[layer_log] = positions;
      const DecRef d = put_dec(lp.decommitment);
      const uint32_t root = put_hash(lp.commitment);
      const std::string name = "Fri(InnerLayerCommitmentInvalid " + std::to_string(li) + "): ";
      const std::string err = plan_tree(std::vector<uint32_t>(4, layer_log), dpos, 8 * (size_t)np, REF_SCRATCH | dvals, d, root, n_flags);
      if (!err.empty()) { finish_fri(); return host_fail(CM_VERIFY_FRI_INNER_COMMITMENT, name + err); }
      device_slot(CM_VERIFY_FRI_INNER_COMMITMENT, name + "RootMismatch");
      uint32_t L[VF_LAYER_WORDS] = {layer_log, np, put(slots), dvals, 0, 0, 0, 0, (uint32_t)(col - add_first), (uint32_t)add_first, (uint32_t)n_evals, 0};
      pre.alphas[li].to_u32(&L[4]);
      layers.insert(layers.end(), L, L + VF_LAYER_WORDS);
      n_evals = np;
      lq = lq.fold(1);
    }
    if (col != q_logs.size()) { finish_fri(); return host_fail(CM_VERIFY_FRI_STRUCTURE, "Fri(InvalidNumFriLayers)"); }
    // ---- last layer
    fri[VF_DO_LAST] = 1;
    fri[VF_LAST_NPOS] = (uint32_t)lq.positions.size();
    fri[VF_LAST_POS] = put(lq.positions);
    fri[VF_LAST_LOG] = layer_log;
    fri[VF_POLY] = put_q(pf.last_layer_poly.data(), pf.last_layer_poly.size());
    fri[VF_POLY_LOG] = pf.last_layer_log_size;
    fri[VF_LAST_FLAG] = device_slot(CM_VERIFY_FRI_LAST_EVALS, "Fri(LastLayerEvaluationsInvalid)");
    finish_fri();
  }
};

struct Timing { double ms[4] = {0, 0, 0, 0}; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr}; };
Timing& timing() {
  static thread_local Timing* t = nullptr;
  if (!t) {
    t = new Timing();
    Timing* own = t;
    at_thread_exit([own] { for (auto e : own->ev) if (e) (void)hipEventDestroy(e); delete own; });
  }
  return *t;
}

}  // namespace

void verify_many_timing(double ms[4]) { for (int i = 0; i < 4; i++) ms[i] = timing().ms[i]; }

// What the kernels would walk for this planner's proofs, read back from its tables (verify_device.hpp: the plan format)
static void read_plan_stats(const Planner& pl, cm_verify_stats& s) {
  const uint32_t* B = pl.blob.data();
  s.n_answer_jobs = (uint32_t)(pl.ans_jobs.size() / 8);
  for (size_t j = 0; j < pl.ans_jobs.size(); j += 8) {
    const uint32_t* G = B + pl.ans_jobs[j];
    for (uint32_t b = 0; b < G[0]; b++) s.max_batch_entries = std::max(s.max_batch_entries, G[5 + 10 * b + 8]);
  }
  for (uint32_t off : pl.fri_jobs) {
    const uint32_t* F = B + off;
    for (uint32_t g = 0; g < F[VF_N_GROUPS]; g++) s.max_first_pairs = std::max(s.max_first_pairs, B[F[VF_GROUPS] + VF_GROUP_WORDS * g + 1]);
    for (uint32_t li = 0; li < F[VF_N_LAYERS]; li++) s.max_inner_pairs = std::max(s.max_inner_pairs, B[F[VF_LAYERS] + VF_LAYER_WORDS * li + 1]);
  }
  s.n_tree_jobs = (uint32_t)(pl.tree_jobs.size() / 8);
  for (size_t j = 0; j < pl.tree_jobs.size(); j += 8)
    for (uint32_t lv = 0; lv < pl.tree_jobs[j]; lv++) s.max_level_nodes = std::max(s.max_level_nodes, B[pl.tree_jobs[j + 1] + 4 * lv]);
  s.merkle_lds_bytes = s.n_tree_jobs ? (uint32_t)verify_merkle_lds_bytes(s.max_level_nodes) : 0u;
  s.blob_words = pl.blob.size();
  s.scratch_words = pl.scr_words;
}

void verify_plan_stats(const ProofData* const* proofs, uint32_t n, const cm_pcs_config& cfg, cm_verify_stats* out) {
  FramingUse framing_use;
  // CM_VERIFY_PLAN_MARKS=1 (tools/verify_bench.py --plan-split): where planning a proof spends its time, on stderr
  const char* want_marks = getenv("CM_VERIFY_PLAN_MARKS");
  for (uint32_t i = 0; i < n; i++) {
    Planner pl;
    ProofPlan pp;
    PreludeMarks marks;
    double plan_ms = 0;
    if (want_marks && want_marks[0] == '1') pl.marks = &marks;
    {
      MarkTimer t(&plan_ms);
      pl.plan_proof(*proofs[i], cfg, pp);
    }
    if (want_marks && want_marks[0] == '1')
      fprintf(stderr, "cm_verify_plan_stats: proof %u: plan %.4f ms = replay and host checks %.4f + public LogUp sum %.4f + OODS evaluation %.4f + tables %.4f\n",
              i, plan_ms, marks.total_ms - marks.logup_ms - marks.oods_ms, marks.logup_ms, marks.oods_ms, plan_ms - marks.total_ms);
    cm_verify_stats s;
    memset(&s, 0, sizeof(s));
    s.struct_size = sizeof(s);
    if (pp.decided_early) s.early_check = pp.early.check;
    else {
      read_plan_stats(pl, s);
      s.n_slots = (uint32_t)pp.slots.size();
    }
    out[i] = s;
  }
}

void verify_many_device(const ProofData* const* proofs, uint32_t n, const cm_pcs_config& cfg, std::vector<VerifyOutcome>& out, hipStream_t st,
                        std::vector<std::vector<VerifySlotDetail>>* detail, uint32_t flags_in) {
  CM_CHECK((flags_in & ~CM_VERIFY_ARITH_ON_DEVICE) == 0, "cm_verify_many: unknown flag bit");
  const bool arith_on_device = (flags_in & CM_VERIFY_ARITH_ON_DEVICE) != 0;
  {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
      throw CmError(3, "cm_verify_many: no HIP device available (libcairom_hip has no CPU fallback)");
  }
  bind_thread_to_library_device();
  FramingUse framing_use;   // one framing for the whole batch
  Timing& tm = timing();
  const auto t0 = std::chrono::steady_clock::now();
  Planner pl;
  std::vector<ProofPlan> plans(n);
  for (uint32_t i = 0; i < n; i++) {
    pl.plan_proof(*proofs[i], cfg, plans[i], arith_on_device);
    CM_CHECK(pl.blob.size() < (1u << 30) && pl.scr_words < (1u << 30), "cm_verify_many: the batch is too large for one call (2^30 plan words): split it");
  }
  CM_CHECK(pl.max_level_nodes <= VERIFY_MAX_LEVEL_NODES, "cm_verify_many: more than 1024 nodes in one level of a tree (n_queries above 512) is not supported on the device");
  std::vector<uint32_t> reduce_jobs(2 * (size_t)n);
  for (uint32_t i = 0; i < n; i++) {
    reduce_jobs[2 * i] = plans[i].flag_base;
    reduce_jobs[2 * i + 1] = plans[i].decided_early ? 0u : (uint32_t)plans[i].slots.size() - (plans[i].fail_slot >= 0 ? 1u : 0u);
  }
  const uint32_t n_ans = (uint32_t)(pl.ans_jobs.size() / 8), n_fri = (uint32_t)pl.fri_jobs.size(), n_tree = (uint32_t)(pl.tree_jobs.size() / 8);
  const uint32_t ans_off = pl.put(pl.ans_jobs), fri_off = pl.put(pl.fri_jobs), tree_off = pl.put(pl.tree_jobs), red_off = pl.put(reduce_jobs);
  std::vector<uint32_t> oods_jobs;
  for (auto& v : pl.oods_jobs) {   // component-major, every component's jobs padded to whole waves: a wave runs ONE arm of the evaluator's switch
    oods_jobs.insert(oods_jobs.end(), v.begin(), v.end());
    const size_t n_jobs = v.size() / VP_OODS_JOB_WORDS;
    oods_jobs.insert(oods_jobs.end(), ((n_jobs + 63) / 64 * 64 - n_jobs) * VP_OODS_JOB_WORDS, VP_NONE);
  }
  const uint32_t n_sum = (uint32_t)(pl.sum_jobs.size() / VP_SUM_JOB_WORDS), n_oods = (uint32_t)(oods_jobs.size() / VP_OODS_JOB_WORDS),
                 n_fin = (uint32_t)(pl.fin_jobs.size() / VP_FIN_JOB_WORDS);
  const uint32_t sum_off = pl.put(pl.sum_jobs), oods_off = pl.put(oods_jobs), fin_off = pl.put(pl.fin_jobs);
  CM_CHECK(pl.blob.size() < (1u << 30), "cm_verify_many: the batch is too large for one call (2^30 plan words): split it");
  tm.ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();

  for (auto& e : tm.ev) if (!e) CM_HIP(hipEventCreate(&e));
  DevBuf d_blob(4 * pl.blob.size()), d_scr(4 * (size_t)std::max<uint64_t>(pl.scr_words, 1)), d_flags(4 * ((size_t)pl.n_flags + n));
  uint32_t* d_out = d_flags.u32() + pl.n_flags;
  CM_HIP(hipEventRecord(tm.ev[0], st));
  stage_upload(d_blob.p, pl.blob.data(), 4 * pl.blob.size(), st);
  CM_HIP(hipMemsetAsync(d_flags.p, 0, 4 * ((size_t)pl.n_flags + n), st));
  CM_HIP(hipEventRecord(tm.ev[1], st));
  const uint32_t* blob = d_blob.u32();
  if (n_ans) hipLaunchKernelGGL(k_verify_answers, dim3(n_ans), dim3(ANS_THREADS), 0, st, blob, d_scr.u32(), blob + ans_off);
  if (n_fri) hipLaunchKernelGGL(k_verify_fri, dim3(n_fri), dim3(FRI_THREADS), 0, st, blob, d_scr.u32(), d_flags.u32(), blob + fri_off);
  if (n_tree) {
    const uint32_t cap = pl.max_level_nodes;
    const size_t lds = verify_merkle_lds_bytes(cap);
    if (framing().hash_node_rfc)
      hipLaunchKernelGGL(k_verify_merkle<true>, dim3(n_tree), dim3(MERKLE_THREADS), lds, st, blob, (const uint32_t*)d_scr.u32(), d_flags.u32(), blob + tree_off, cap);
    else
      hipLaunchKernelGGL(k_verify_merkle<false>, dim3(n_tree), dim3(MERKLE_THREADS), lds, st, blob, (const uint32_t*)d_scr.u32(), d_flags.u32(), blob + tree_off, cap);
  }
  launch_verify_public_sum(blob, d_scr.u32(), blob + sum_off, n_sum, st);
  launch_verify_oods(blob, d_scr.u32(), blob + oods_off, n_oods, st);
  launch_verify_prelude_fin(blob, d_scr.u32(), d_flags.u32(), blob + fin_off, n_fin, st);
  hipLaunchKernelGGL(k_verify_reduce, dim3((n + 63) / 64), dim3(64), 0, st, (const uint32_t*)d_flags.u32(), blob + red_off, n, d_out);
  CM_HIP(hipGetLastError());
  CM_HIP(hipEventRecord(tm.ev[2], st));
  // (detail: the flag words sit in front of the verdicts in one buffer, and come down with them)
  const uint32_t* flags = detail ? (const uint32_t*)stage_download_async(d_flags.p, 4 * ((size_t)pl.n_flags + n), st) : nullptr;
  const uint32_t* res = detail ? flags + pl.n_flags : (const uint32_t*)stage_download_async(d_out, 4 * (size_t)n, st);
  CM_HIP(hipEventRecord(tm.ev[3], st));
  CM_HIP(hipStreamSynchronize(st));
  for (int k = 0; k < 3; k++) {
    float ms = 0;
    CM_HIP(hipEventElapsedTime(&ms, tm.ev[k], tm.ev[k + 1]));
    tm.ms[k + 1] = ms;
  }
  out.assign(n, VerifyOutcome());
  for (uint32_t i = 0; i < n; i++) {
    const ProofPlan& pp = plans[i];
    if (pp.decided_early) { out[i] = pp.early; continue; }
    int slot = pp.fail_slot;
    if (res[i] != 0xffffffffu) slot = (int)res[i];   // a raised flag is always in front of the slot that failed while planning (the last one, also behind deferred slots)
    if (slot >= 0) { out[i].check = pp.slots[slot].check; out[i].message = pp.slots[slot].message; }
  }
  if (!detail) return;
  detail->assign(n, std::vector<VerifySlotDetail>());
  for (uint32_t i = 0; i < n; i++) {
    const ProofPlan& pp = plans[i];
    for (size_t k = 0; k < pp.slots.size(); k++) {
      const bool planned = (int)k == pp.fail_slot;
      (*detail)[i].push_back(VerifySlotDetail{pp.slots[k].check, pp.slots[k].message, !planned, planned || flags[pp.flag_base + k] != 0});
    }
  }
}

}  // namespace cm
