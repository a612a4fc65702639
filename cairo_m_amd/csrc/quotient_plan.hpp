// Host half of compute_fri_quotients, shared by the single-GPU prover (prover.hip) and the sharded one (prover_sharded.inc):
// size groups, sample-point batches, and ONE blob for the device — per group, 16-byte aligned, [column pointers | out pointers |
// col_index | entry column pointers | sample_idx | coef_c | batches], then the QuotientCoefJob table (k_quotient_coeffs fills coef_c
// and the batch sums).  Three steps — the single-GPU prover plans and uploads while the OODS evaluations run and launches a phase
// later: build() (no sampled value needed), bind() once the blob has its device address, quotient_args() for the launches.
#pragma once
#include "prover_common.hpp"

namespace cm {
// the rows a prover computes: all of them, or rank `rank`'s 1 / 2^log_ranks of every column (output columns and launch arguments)
struct QuotientWindow { int log_ranks = -1; uint32_t rank = 0; uint32_t shift() const { return log_ranks < 0 ? 0u : (uint32_t)log_ranks; } };
struct QuotientCol { int t; uint32_t c; uint32_t lde_log; const uint32_t* ptr; };   // ptr: the column's rows [row0, ..) of the LDE
struct QuotientGroup {
  uint32_t log = 0, n_batches = 0;        // LDE log of the group's columns
  std::vector<const uint32_t*> cols;
  ColumnSet out;                          // the four coordinate columns (rows of the window only)
  size_t o_cols = 0, o_out = 0, o_ci = 0, o_ep = 0, o_si = 0, o_cc = 0, o_qb = 0;   // offsets in the blob
};
struct QuotientPlan {
  std::vector<QuotientGroup> groups;      // largest first
  std::vector<uint8_t> blob;
  size_t o_jobs = 0, n_jobs = 0;
  size_t put(const void* ptr, size_t bytes) {
    const size_t o = (blob.size() + 15) & ~(size_t)15;
    blob.resize(o + bytes);
    if (bytes && ptr) memcpy(blob.data() + o, ptr, bytes);
    return o;
  }
  // `cols` in tree-major order; masks[t][c] = 1 ([oods]) or 2 ([previous row, oods]) sampled values; sidx_* = index of a column's
  // sampled value in the device array k_quotient_coeffs reads; prev_points by TRACE log (= lde_log - log_blowup; a size that is
  // missing there throws); the output columns hold the window's rows
  void build(const std::vector<QuotientCol>& cols, const std::vector<std::vector<SampleVec>>& masks,
             const std::vector<std::vector<uint32_t>>& sidx_cur, const std::vector<std::vector<uint32_t>>& sidx_prev, const CPoint<QM31>& oods,
             const std::map<uint32_t, CPoint<QM31>>& prev_points, uint32_t log_blowup, const QuotientWindow& win, hipStream_t st) {
    std::map<uint32_t, std::vector<const QuotientCol*>, std::greater<uint32_t>> by_size;
    for (auto& qc : cols) by_size[qc.lde_log].push_back(&qc);
    struct Batch { CPoint<QM31> pt; std::vector<std::pair<uint32_t, uint32_t>> entries; };   // (column in group, sample index)
    for (auto& kv : by_size) {
      QuotientGroup g;
      g.log = kv.first;
      std::vector<Batch> batches;
      for (uint32_t i = 0; i < kv.second.size(); i++) {
        const QuotientCol& r = *kv.second[i];
        g.cols.push_back(r.ptr);
        const size_t ns = masks[r.t][r.c].size();
        for (size_t k = 0; k < ns; k++) {
          const bool is_prev = ns == 2 && k == 0;   // sample points: [oods] or [prev, oods]
          const CPoint<QM31> pt = is_prev ? prev_points.at(r.lde_log - log_blowup) : oods;
          size_t bi = 0;
          for (; bi < batches.size(); bi++) if (batches[bi].pt.x == pt.x && batches[bi].pt.y == pt.y) break;
          if (bi == batches.size()) batches.push_back(Batch{pt, {}});
          batches[bi].entries.push_back({i, is_prev ? sidx_prev[r.t][r.c] : sidx_cur[r.t][r.c]});
        }
      }
      if (framing().sample_batch_sorted)   // ColumnSampleBatch::new_vec as a BTreeMap keyed by point (framing.hpp)
        std::stable_sort(batches.begin(), batches.end(), [](const Batch& a, const Batch& b) { return secure_point_less(a.pt, b.pt); });
      std::vector<uint32_t> ci, si;
      std::vector<const uint32_t*> ep;   // per entry: the column pointer itself (the two-rows kernel's scalar loads)
      std::vector<QuotientBatch> qb(batches.size());
      for (size_t bi = 0; bi < batches.size(); bi++) {
        memset(&qb[bi], 0, sizeof(QuotientBatch));
        qb[bi].begin = (uint32_t)ci.size();
        for (auto& en : batches[bi].entries) { ci.push_back(en.first); si.push_back(en.second); ep.push_back(g.cols[en.first]); }
        qb[bi].end = (uint32_t)ci.size();
        batches[bi].pt.x.to_u32(qb[bi].point);   // words = (Pr.x, Pi.x): QM31 = (a.a, a.b, b.a, b.b)
        batches[bi].pt.y.to_u32(qb[bi].point + 4);
      }
      g.n_batches = (uint32_t)qb.size();
      g.out.alloc(std::vector<uint32_t>(4, g.log - win.shift()), st, false);
      g.o_cols = put(g.cols.data(), g.cols.size() * sizeof(void*));
      g.o_out = put(g.out.ptrs.data(), 4 * sizeof(void*));
      g.o_ci = put(ci.data(), ci.size() * 4);
      g.o_ep = put(ep.data(), ep.size() * sizeof(void*));
      g.o_si = put(si.data(), si.size() * 4);
      g.o_cc = put(nullptr, ci.size() * 16);                           // filled by k_quotient_coeffs
      g.o_qb = put(qb.data(), qb.size() * sizeof(QuotientBatch));      // sums / batch coefficient filled on the device
      n_jobs += qb.size();
      groups.push_back(std::move(g));
    }
    o_jobs = put(nullptr, n_jobs * sizeof(QuotientCoefJob));
  }
  // the job table points into the device copy of the blob: call with its address, then upload the blob
  void bind(uint8_t* base) {
    QuotientCoefJob* qj = (QuotientCoefJob*)(blob.data() + o_jobs);
    size_t k = 0;
    for (auto& g : groups)
      for (uint32_t bi = 0; bi < g.n_batches; bi++, k++) {
        qj[k].qb = (QuotientBatch*)(base + g.o_qb) + bi;
        qj[k].coef_c = (uint32_t*)(base + g.o_cc);
        qj[k].sample_idx = (const uint32_t*)(base + g.o_si);
      }
  }
};
// (launch arguments, columns) per group, for the window the plan was built with
inline std::vector<std::pair<QuotientArgs, double>> quotient_args(const std::vector<QuotientGroup>& groups, const uint8_t* base, const Twiddles& tw,
                                                                  const QuotientWindow& win = QuotientWindow()) {
  std::vector<std::pair<QuotientArgs, double>> qargs;
  for (auto& g : groups) {
    QuotientArgs a;
    a.tw = view(tw); a.log_size = g.log;
    a.cols = (const uint32_t* const*)(base + g.o_cols);
    a.out = (uint32_t* const*)(base + g.o_out);
    a.col_index = (const uint32_t*)(base + g.o_ci);
    a.entry_cols = (const uint32_t* const*)(base + g.o_ep);
    a.coef_c = (const uint32_t*)(base + g.o_cc);
    a.batches = (const QuotientBatch*)(base + g.o_qb);
    a.n_batches = g.n_batches;
    if (win.log_ranks >= 0) { a.n_rows = 1u << (g.log - win.shift()); a.row0 = win.rank * a.n_rows; }
    qargs.push_back({a, (double)g.cols.size()});
  }
  return qargs;
}
// "quot_leaf": may the kernel of the LARGEST size group (strictly larger than the next) hash the FRI first-layer tree's leaf layer?
inline bool quotient_leaf_wanted(const std::vector<std::pair<QuotientArgs, double>>& qargs) {
  return tune(T_QUOT_LEAF) != 0 && !qargs.empty() && (qargs.size() == 1 || qargs[1].first.log_size < qargs[0].first.log_size) &&
         quotient_leaf_serves(qargs[0].first);
}
}  // namespace cm
