// What the host verifier (verifier.hip) and the batched device verifier (verify_device.hip) share: the Merkle / FRI / DEEP-quotient
// helpers of Stwo's verify, the public data's transcript framing and LogUp sum, and `verify_prelude` — everything
// `verify_cairo_m` does before it looks at a queried value (config and structure, transcript replay, both proofs of work, the
// LogUp sum, the OODS composition check, the FRI layer count, the query draw).  Host code only.
#pragma once
#include "../../include/cairom_hip.h"
#include "host_channel.hpp"
#include "point_eval.hpp"
#include "proof.hpp"
#include "framing.hpp"
#include "air/components.hpp"
#include <algorithm>
#include <chrono>
#include <functional>
#include <map>
#include <set>
#include <string>

namespace cm {
namespace verif {

using hostch::Channel;

// ---- Merkle (Stwo MerkleVerifier::verify over Blake2sMerkleHasher) ------------------------------------------
inline Hash32 hash_node(const Hash32* left, const Hash32* right, const uint32_t* vals, size_t n) {
  if (framing().hash_node_rfc) {   // framing.hpp `hash_node=rfc`: Blake2s-256 of left || right || le32(values)
    std::vector<uint8_t> buf((left ? 64 : 0) + 4 * n);
    if (left) { memcpy(buf.data(), left->data(), 32); memcpy(buf.data() + 32, right->data(), 32); }
    if (n) memcpy(buf.data() + (left ? 64 : 0), vals, 4 * n);
    return hostch::blake2s256(buf.data(), buf.size());
  }
  uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m[16];
  if (left) {
    memcpy(m, left->data(), 32);
    memcpy(m + 8, right->data(), 32);
    hostch::compress(st, m, 0, 0);
  }
  for (size_t c0 = 0; c0 < n; c0 += 16) {
    for (size_t k = 0; k < 16; k++) m[k] = c0 + k < n ? vals[c0 + k] : 0u;
    hostch::compress(st, m, 0, 0);
  }
  Hash32 out;
  memcpy(out.data(), st, 32);
  return out;
}
// col_logs: log size of every column of the tree in commitment order; queries: log -> sorted unique positions
inline std::string merkle_verify(const Hash32& root, const std::vector<uint32_t>& col_logs, const std::map<uint32_t, std::vector<uint32_t>>& queries,
                          const std::vector<uint32_t>& queried_values, const MerkleDecommitment& d) {
  if (col_logs.empty()) return "empty tree";
  uint32_t max_log = *std::max_element(col_logs.begin(), col_logs.end());
  std::map<uint32_t, uint32_t> n_cols;
  for (auto l : col_logs) n_cols[l]++;
  size_t qi = 0, hi = 0, ci = 0;
  std::vector<std::pair<uint32_t, Hash32>> last;
  for (int log = (int)max_log; log >= 0; log--) {
    const uint32_t nc = n_cols.count((uint32_t)log) ? n_cols[(uint32_t)log] : 0;
    static const std::vector<uint32_t> none;
    auto it = queries.find((uint32_t)log);
    const std::vector<uint32_t>& colq = (nc && it != queries.end()) ? it->second : none;
    std::vector<std::pair<uint32_t, Hash32>> cur;
    size_t pi = 0, cq = 0;
    const bool has_prev = log < (int)max_log;
    while (pi < last.size() || cq < colq.size()) {
      uint32_t node;
      if (pi < last.size() && cq < colq.size()) node = std::min(last[pi].first / 2, colq[cq]);
      else if (pi < last.size()) node = last[pi].first / 2;
      else node = colq[cq];
      Hash32 l, r;
      if (has_prev) {
        if (pi < last.size() && last[pi].first == 2 * node) l = last[pi++].second;
        else { if (hi >= d.hash_witness.size()) return "WitnessTooShort"; l = d.hash_witness[hi++]; }
        if (pi < last.size() && last[pi].first == 2 * node + 1) r = last[pi++].second;
        else { if (hi >= d.hash_witness.size()) return "WitnessTooShort"; r = d.hash_witness[hi++]; }
      }
      std::vector<uint32_t> vals(nc);
      const bool isq = cq < colq.size() && colq[cq] == node;
      if (isq) {
        cq++;
        if (qi + nc > queried_values.size()) return "TooFewQueriedValues";
        for (uint32_t k = 0; k < nc; k++) vals[k] = queried_values[qi++];
      } else {
        if (ci + nc > d.column_witness.size()) return "WitnessTooShort";
        for (uint32_t k = 0; k < nc; k++) vals[k] = d.column_witness[ci++];
      }
      cur.push_back({node, hash_node(has_prev ? &l : nullptr, has_prev ? &r : nullptr, vals.data(), nc)});
    }
    last.swap(cur);
  }
  if (hi != d.hash_witness.size() || ci != d.column_witness.size()) return "WitnessTooLong";
  if (qi != queried_values.size()) return "TooManyQueriedValues";
  if (last.size() != 1 || last[0].second != root) return "RootMismatch";
  return "";
}

// ---- public data: transcript framing and LogUp contribution (public_data.rs:291-412) --------------------------
inline void mix_public_data(const PublicData& d, Channel& ch) {
  uint32_t w[7] = {d.initial_pc, d.initial_fp, d.final_pc, d.final_fp, d.clock, d.initial_root, d.final_root};
  ch.mix_u32s(w, 7);
  uint32_t lens[3] = {(uint32_t)d.program.size(), (uint32_t)d.input.size(), (uint32_t)d.output.size()};
  ch.mix_u32s(lens, 3);
  for (const auto* v : {&d.program, &d.input, &d.output}) {
    std::vector<uint32_t> words;
    for (auto& e : *v) if (e.present) { words.push_back(e.addr); for (int k = 0; k < 4; k++) words.push_back(e.value[k]); words.push_back(e.clock); }
    ch.mix_u32s(words.data(), words.size());
  }
}
inline QM31 combine(const HostRelations& rel, int r, std::initializer_list<M31> vals) {
  QM31 a;
  int i = 0;
  for (M31 v : vals) a += rel.alpha_pow[r][i++] * v;
  return a - rel.z[r];
}
// per_relation (optional): the same sum split by relation (registers, merkle, memory; the other relations stay zero) — the AIR
// check (check.hip) reports it next to the components' relation sums
inline QM31 initial_logup_sum(const PublicData& d, const HostRelations& rel, QM31* per_relation = nullptr) {
  const M31 one(1), zero;
  std::vector<std::pair<int, QM31>> dens;   // (relation, denominator of a +1 entry)
  dens.push_back({air::REL_REGISTERS, combine(rel, air::REL_REGISTERS, {M31(d.initial_pc), M31(d.initial_fp), one})});
  dens.push_back({air::REL_REGISTERS, -combine(rel, air::REL_REGISTERS, {M31(d.final_pc), M31(d.final_fp), M31(d.clock) + one})});
  dens.push_back({air::REL_MERKLE, combine(rel, air::REL_MERKLE, {zero, zero, M31(d.initial_root), M31(d.initial_root)})});
  dens.push_back({air::REL_MERKLE, combine(rel, air::REL_MERKLE, {zero, zero, M31(d.final_root), M31(d.final_root)})});
  auto add = [&](const std::vector<PublicEntry>& es, bool emit) {
    const M31 root(emit ? d.initial_root : d.final_root), height(air::TREE_HEIGHT), four(4);
    for (auto& e : es) {
      if (!e.present) continue;
      QM31 mem = combine(rel, air::REL_MEMORY, {M31(e.addr), M31(e.clock), M31(e.value[0]), M31(e.value[1]), M31(e.value[2]), M31(e.value[3])});
      dens.push_back({air::REL_MEMORY, emit ? mem : -mem});
      for (uint32_t k = 0; k < 4; k++) dens.push_back({air::REL_MERKLE, -combine(rel, air::REL_MERKLE, {four * M31(e.addr) + M31(k), height, M31(e.value[k]), root})});
    }
  };
  add(d.program, true);
  add(d.input, true);
  add(d.output, false);
  QM31 s;
  if (per_relation)
    for (int r = 0; r < air::N_RELATIONS; r++) per_relation[r] = QM31();
  for (auto& x : dens) {
    const QM31 f = inv(x.second);
    s += f;
    if (per_relation) per_relation[x.first] += f;
  }
  return s;
}

inline CPoint<QM31> into_ef(CPoint<M31> p) { return CPoint<QM31>{QM31(p.x), QM31(p.y)}; }
// vanishing polynomial of CanonicCoset(log).coset at a QM31 point (shift is zero for a canonic coset)
inline QM31 canonic_vanishing(uint32_t log, CPoint<QM31> p) {
  QM31 x = p.x;
  for (uint32_t i = 1; i < log; i++) x = double_x(x);
  return x;
}
inline CPoint<M31> domain_point(uint32_t log, uint32_t row) { return point_at_index(domain_index_at(log, bit_reverse(row, log))); }

struct Sample { CPoint<QM31> pt; QM31 value; };
// ColumnSampleBatch::new_vec: the samples of a size group by point, in the order of the framing in force; entries = (column, value)
struct SampleBatch { CPoint<QM31> pt; std::vector<std::pair<size_t, QM31>> entries; };
inline std::vector<SampleBatch> sample_batches(const std::vector<std::vector<Sample>>& cols) {
  std::vector<SampleBatch> batches;
  for (size_t c = 0; c < cols.size(); c++)
    for (auto& s : cols[c]) {
      size_t b = 0;
      for (; b < batches.size(); b++) if (batches[b].pt.x == s.pt.x && batches[b].pt.y == s.pt.y) break;
      if (b == batches.size()) batches.push_back(SampleBatch{s.pt, {}});
      batches[b].entries.push_back({c, s.value});
    }
  if (framing().sample_batch_sorted)
    std::stable_sort(batches.begin(), batches.end(), [](const SampleBatch& a, const SampleBatch& b) { return secure_point_less(a.pt, b.pt); });
  return batches;
}
// DEEP quotient of one queried row (Stwo accumulate_row_quotients): cols[c] = samples of column c of the size group
inline QM31 row_quotient(const std::vector<std::vector<Sample>>& cols, QM31 random_coeff, const std::vector<uint32_t>& row, CPoint<M31> p) {
  const std::vector<SampleBatch> batches = sample_batches(cols);
  QM31 acc;
  for (auto& b : batches) {
    QM31 alpha(M31(1)), num;
    const QM31 cdiff = conj_u(b.pt.y) - b.pt.y;
    for (auto& e : b.entries) {
      alpha = alpha * random_coeff;
      QM31 a = conj_u(e.second) - e.second;
      QM31 bb = e.second * cdiff - a * b.pt.y;
      num += alpha * (cdiff * M31(row[e.first]) - (a * p.y + bb));
    }
    CM31 prx = b.pt.x.a, pix = b.pt.x.b, pry = b.pt.y.a, piy = b.pt.y.b;
    CM31 den = (prx - CM31(p.x)) * piy - (pry - CM31(p.y)) * pix;
    acc = acc * qpow(random_coeff, b.entries.size()) + mul_cm31(num, inv(den));
  }
  return acc;
}

struct FoldQueries {
  std::vector<uint32_t> positions;
  FoldQueries fold(uint32_t n) const {
    FoldQueries q;
    for (auto p : positions) { uint32_t f = p >> n; if (q.positions.empty() || q.positions.back() != f) q.positions.push_back(f); }
    return q;
  }
};
// compute_decommitment_positions_and_rebuild_evals (fold step 1)
inline bool rebuild_evals(const std::vector<uint32_t>& queries, const std::vector<QM31>& query_evals, const std::vector<QM31>& witness, size_t& wi,
                   std::vector<uint32_t>& positions, std::vector<std::array<QM31, 2>>& pairs, std::vector<uint32_t>& starts) {
  size_t i = 0;
  while (i < queries.size()) {
    uint32_t start = (queries[i] >> 1) << 1;
    size_t j = i;
    while (j < queries.size() && (queries[j] >> 1) == (queries[i] >> 1)) j++;
    size_t qi = i;
    std::array<QM31, 2> pr;
    for (uint32_t k = 0; k < 2; k++) {
      positions.push_back(start + k);
      if (qi < j && queries[qi] == start + k) pr[k] = query_evals[qi++];
      else { if (wi >= witness.size()) return false; pr[k] = witness[wi++]; }
    }
    pairs.push_back(pr);
    starts.push_back(start);
    i = j;
  }
  return true;
}

// What verify_prelude leaves for the query phase
struct VerifyPrelude {
  std::vector<std::vector<uint32_t>> logs;                        // column log sizes per tree (preprocessed, trace, interaction, composition)
  std::vector<std::vector<std::vector<CPoint<QM31>>>> pts;        // mask points per tree and column
  QM31 qcoeff, circle_alpha;
  std::vector<QM31> alphas;                                       // one per inner FRI layer
  std::vector<uint32_t> q_logs;                                   // distinct extended log sizes, descending
  FoldQueries queries;
  std::map<uint32_t, std::vector<uint32_t>> qpos;                 // log -> sorted unique positions
};

// What verify_prelude records when its two pure-arithmetic checks are deferred (verify_device.hip decides them on the GPU):
// `stage` says how far the record goes when the prelude fails behind a deferred check.
struct DeferredArith {
  int stage = 0;           // 0: nothing yet; 1: rel (the LogUp sum can be checked); 2: all of it (and the sampled values have their shape)
  HostRelations rel;       // the relation challenges
  QM31 random_coeff;
  CPoint<QM31> oods;
  std::vector<size_t> tr0, it0;   // per component: its first column in trees 1 and 2
};

// Where verify_prelude spends its time: filled when the caller hands one in (only cm_verify_plan_stats under
// CM_VERIFY_PLAN_MARKS does: tools/verify_bench.py --plan-split)
struct PreludeMarks { double total_ms = 0, logup_ms = 0, oods_ms = 0; };
struct MarkTimer {
  double* into;
  std::chrono::steady_clock::time_point t0;
  explicit MarkTimer(double* d) : into(d) { if (into) t0 = std::chrono::steady_clock::now(); }
  ~MarkTimer() { if (into) *into += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// Every check of verify_cairo_m in front of the queries, in its order.  "" = passed (`o` is filled); otherwise the name of the
// failed check, with its CM_VERIFY_* id in *check.  `cfg` is the verifier's own PcsConfig.  The caller holds a FramingUse.
// defer != nullptr: InvalidLogupSum and OodsNotMatching are not decided here (the transcript does not depend on them) and
// *defer records what deciding them needs; every other check stays, in its place.
inline std::string verify_prelude(const ProofData& pf, const cm_pcs_config& cfg, VerifyPrelude& o, int32_t* check = nullptr,
                                  DeferredArith* defer = nullptr, PreludeMarks* marks = nullptr) {
  auto fail = [&](int32_t id, const char* msg) { if (check) *check = id; return std::string(msg); };
  MarkTimer whole(marks ? &marks->total_ms : nullptr);
  if (pf.config.pow_bits != cfg.pow_bits || pf.config.log_blowup_factor != cfg.log_blowup_factor ||
      pf.config.n_queries != cfg.n_queries || pf.config.log_last_layer_degree_bound != cfg.log_last_layer_degree_bound)
    return fail(CM_VERIFY_STRUCTURE, "InvalidStructure(config): the proof was made under a different PcsConfig than the verifier's");
  if (pf.claim_log_sizes.size() != (size_t)air::N_COMPONENTS || pf.claimed_sums.size() != (size_t)air::N_COMPONENTS ||
      pf.commitments.size() != 4 || pf.sampled_values.size() != 4 || pf.decommitments.size() != 4 || pf.queried_values.size() != 4)
    return fail(CM_VERIFY_STRUCTURE, "InvalidStructure");
  for (auto l : pf.claim_log_sizes) if (l < 4 || l > 26) return fail(CM_VERIFY_STRUCTURE, "InvalidStructure(log size)");
  if (cfg.log_blowup_factor < 1 || cfg.log_blowup_factor > 4 || cfg.n_queries == 0 || cfg.n_queries > 4096 || cfg.pow_bits > 64 ||
      cfg.log_last_layer_degree_bound > 20) return fail(CM_VERIFY_STRUCTURE, "InvalidStructure(config)");
  Channel ch;
  ch.mix_u64(cfg.pow_bits);
  ch.mix_u64(cfg.log_blowup_factor);
  if (framing().pcs_mix_blq) { ch.mix_u64(cfg.log_last_layer_degree_bound); ch.mix_u64(cfg.n_queries); }
  else { ch.mix_u64(cfg.n_queries); ch.mix_u64(cfg.log_last_layer_degree_bound); }
  mix_public_data(pf.public_data, ch);
  // column log sizes per tree (preprocessed, trace, interaction, composition)
  std::vector<std::vector<uint32_t>>& logs = o.logs;
  logs.assign(4, {});
  for (int i = 0; i < air::N_PREPROC; i++) logs[0].push_back(air::PREPROC_LOG[i]);
  std::vector<size_t> tr0(air::N_COMPONENTS), it0(air::N_COMPONENTS);
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    tr0[c] = logs[1].size(); it0[c] = logs[2].size();
    logs[1].insert(logs[1].end(), info.n_trace, pf.claim_log_sizes[c]);
    logs[2].insert(logs[2].end(), info.n_interaction, pf.claim_log_sizes[c]);
  }
  ch.mix_root(pf.commitments[0]);
  for (auto l : pf.claim_log_sizes) ch.mix_u64(l);
  ch.mix_root(pf.commitments[1]);
  ch.mix_u64(pf.interaction_pow);
  if (ch.trailing_zeros() < INTERACTION_POW_BITS) return fail(CM_VERIFY_POW_INTERACTION, "ProofOfWork(interaction)");  // relations::INTERACTION_POW_BITS (verifier.rs:55-58)
  HostRelations rel;
  for (int r = 0; r < air::N_RELATIONS; r++) {
    QM31 z, alpha;
    ch.draw_two_felts(z, alpha);
    rel.z[r] = z;
    QM31 cur(M31(1));
    for (int i = 0; i < air::MAX_REL_SIZE; i++) { rel.alpha_pow[r][i] = cur; cur = cur * alpha; }
  }
  if (defer) { defer->rel = rel; defer->stage = 1; }
  else {
    MarkTimer t(marks ? &marks->logup_ms : nullptr);
    QM31 s = initial_logup_sum(pf.public_data, rel);  // verifier.rs:69-77
    for (auto& c : pf.claimed_sums) s += c;
    if (!s.is_zero()) return fail(CM_VERIFY_LOGUP_SUM, "InvalidLogupSum");
  }
  for (auto& c : pf.claimed_sums) ch.mix_felts(&c, 1);
  ch.mix_root(pf.commitments[2]);
  // ---- stwo verify ----
  const QM31 random_coeff = ch.draw_felt();
  uint32_t max_log = *std::max_element(pf.claim_log_sizes.begin(), pf.claim_log_sizes.end());
  logs[3].assign(4, max_log + 1);
  ch.mix_root(pf.commitments[3]);
  CPoint<QM31> oods;
  {
    QM31 t = ch.draw_felt();
    QM31 t2 = t * t;
    QM31 iv = inv(t2 + M31(1));
    oods.x = (QM31(M31(1)) - t2) * iv;
    oods.y = (t + t) * iv;
  }
  // mask points: every column at the OODS point; the last LogUp column group of a component also one step back
  std::vector<std::vector<std::vector<CPoint<QM31>>>>& pts = o.pts;
  pts.assign(4, {});
  for (int t = 0; t < 4; t++) pts[t].assign(logs[t].size(), {oods});
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    int ni = air::component_info(c).n_interaction;
    CPoint<M31> step = point_at_index(subgroup_gen_index(pf.claim_log_sizes[c]));
    CPoint<QM31> prev = cadd(oods, CPoint<QM31>{QM31(step.x), QM31(-step.y)});
    for (int k = ni - 4; k < ni; k++) pts[2][it0[c] + k] = {prev, oods};
  }
  for (int t = 0; t < 4; t++) {
    if (pf.sampled_values[t].size() != logs[t].size()) return fail(CM_VERIFY_STRUCTURE, "InvalidStructure(sampled columns)");
    for (size_t c = 0; c < logs[t].size(); c++) if (pf.sampled_values[t][c].size() != pts[t][c].size()) return fail(CM_VERIFY_STRUCTURE, "InvalidStructure(samples)");
  }
  if (defer) { defer->random_coeff = random_coeff; defer->oods = oods; defer->tr0 = tr0; defer->it0 = it0; defer->stage = 2; }
  else {  // composition OODS value == sum_c constraints_c(mask) / vanishing_c(oods)
    MarkTimer t(marks ? &marks->oods_ms : nullptr);
    size_t total = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) total += air::component_info(c).n_constraints;
    std::vector<QM31> powers(total);
    QM31 cur(M31(1));
    for (size_t g = total; g-- > 0;) { powers[g] = cur; cur = cur * random_coeff; }
    QM31 c4[4] = {pf.sampled_values[3][0][0], pf.sampled_values[3][1][0], pf.sampled_values[3][2][0], pf.sampled_values[3][3][0]};
    QM31 ppv[air::N_PREPROC];
    for (int i = 0; i < air::N_PREPROC; i++) ppv[i] = pf.sampled_values[0][i][0];
    QM31 sum;
    size_t g = 0;
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      const air::ComponentInfo& info = air::component_info(c);
      std::vector<QM31> tr, it;
      for (int k = 0; k < info.n_trace; k++) tr.push_back(pf.sampled_values[1][tr0[c] + k][0]);
      for (int k = 0; k < info.n_interaction; k++) for (auto& s : pf.sampled_values[2][it0[c] + k]) it.push_back(s);
      QM31 shift = pf.claimed_sums[c] * inv(M31::from_u32(1u << pf.claim_log_sizes[c]));
      QM31 num = point_eval(c, tr.data(), it.data(), ppv, rel, &powers[g], info.n_base_constraints, shift);
      sum += num * inv(canonic_vanishing(pf.claim_log_sizes[c], oods));
      g += info.n_constraints;
    }
    if (sum != combine_ef(c4)) return fail(CM_VERIFY_OODS, "OodsNotMatching");
  }
  {
    std::vector<QM31> flat;
    for (auto& t : pf.sampled_values) for (auto& c : t) for (auto& s : c) flat.push_back(s);
    ch.mix_felts(flat.data(), flat.size());
  }
  o.qcoeff = ch.draw_felt();
  std::set<uint32_t, std::greater<uint32_t>> ext;
  for (int t = 0; t < 4; t++) for (auto l : logs[t]) ext.insert(l + cfg.log_blowup_factor);
  o.q_logs.assign(ext.begin(), ext.end());
  const std::vector<uint32_t>& q_logs = o.q_logs;
  // FRI commit phase replay
  ch.mix_root(pf.fri_first.commitment);
  o.circle_alpha = ch.draw_felt();
  const uint32_t last_log = cfg.log_last_layer_degree_bound + cfg.log_blowup_factor;
  if (q_logs[0] < last_log + 1 || pf.fri_inner.size() != (size_t)(q_logs[0] - 1 - last_log)) return fail(CM_VERIFY_FRI_STRUCTURE, "Fri(InvalidNumFriLayers)");
  std::vector<QM31>& alphas = o.alphas;
  alphas.clear();
  for (auto& l : pf.fri_inner) { ch.mix_root(l.commitment); alphas.push_back(ch.draw_felt()); }
  if (pf.last_layer_poly.size() != ((size_t)1 << cfg.log_last_layer_degree_bound) ||
      pf.last_layer_log_size != cfg.log_last_layer_degree_bound) return fail(CM_VERIFY_FRI_STRUCTURE, "Fri(LastLayerDegreeInvalid)");
  ch.mix_felts(pf.last_layer_poly.data(), pf.last_layer_poly.size());
  ch.mix_u64(pf.proof_of_work);
  if (ch.trailing_zeros() < cfg.pow_bits) return fail(CM_VERIFY_POW, "ProofOfWork");
  FoldQueries& queries = o.queries;
  queries.positions.clear();
  {
    std::set<uint32_t> s;
    uint32_t cnt = 0;
    const uint32_t mask = (1u << q_logs[0]) - 1;
    bool done = false;
    while (!done) {
      hostch::Hash32 b = ch.draw_random_bytes();
      for (int k = 0; k < 8 && !done; k++) {
        uint32_t wv;
        memcpy(&wv, b.data() + 4 * k, 4);
        s.insert(wv & mask);
        if (++cnt == cfg.n_queries) done = true;
      }
    }
    queries.positions.assign(s.begin(), s.end());
  }
  std::map<uint32_t, std::vector<uint32_t>>& qpos = o.qpos;
  qpos.clear();
  for (auto l : q_logs) qpos[l] = queries.fold(q_logs[0] - l).positions;
  return "";
}

}  // namespace verif
}  // namespace cm
