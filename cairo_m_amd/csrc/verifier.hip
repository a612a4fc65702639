// Product-side verifier: `verify_cairo_m::<Blake2sMerkleChannel>` (/root/reference/crates/prover/src/verifier.rs:17-95)
// and the Stwo `verify` it calls (CommitmentSchemeVerifier::verify_values, fri_answers, FriVerifier,
// MerkleVerifier).  Host code only — verification touches O(queries * log n) values —
// so `cm_verify_proof*` also work on a machine without a GPU (a BATCH of proofs is another matter: verify_device.hip).  Written against the product's own
// types (host_channel.hpp, field.hpp, proof.hpp, point_eval.hpp); the CPU oracle has its own, separate verifier.
#include "../../include/cairom_hip.h"
#include "verifier_common.hpp"

namespace cm {

using namespace verif;   // the helpers shared with the device verifier (verifier_common.hpp)

// ---- words -> ProofData (inverse of proof_to_words) ---------------------------------------------------------
bool proof_from_words(const uint32_t* w, uint64_t n, ProofData& p, std::string& err) {
  uint64_t i = 0;
  bool ok = true;
  auto u = [&]() -> uint32_t { if (i >= n) { ok = false; return 0; } return w[i++]; };
  auto cnt = [&](uint64_t unit_words) -> uint32_t {  // a length field followed by that many records
    uint32_t c = u();
    if (ok && (uint64_t)c * unit_words > n - i) ok = false;
    return ok ? c : 0;
  };
  auto u64 = [&]() -> uint64_t { uint64_t lo = u(); uint64_t hi = u(); return lo | (hi << 32); };
  auto q = [&]() -> QM31 { uint32_t t[4]; for (int k = 0; k < 4; k++) t[k] = u(); for (int k = 0; k < 4; k++) if (t[k] >= P) ok = false; return QM31::from_u32(t); };
  auto h = [&]() -> Hash32 { uint32_t t[8]; for (int k = 0; k < 8; k++) t[k] = u(); Hash32 x; memcpy(x.data(), t, 32); return x; };
  auto dec = [&](MerkleDecommitment& d) {
    uint32_t nh = cnt(8);
    for (uint32_t k = 0; k < nh; k++) d.hash_witness.push_back(h());
    uint32_t nc = cnt(1);
    for (uint32_t k = 0; k < nc; k++) { uint32_t v = u(); if (v >= P) ok = false; d.column_witness.push_back(v); }
  };
  auto layer = [&](FriLayerProofData& l) {
    uint32_t nw = cnt(4);
    for (uint32_t k = 0; k < nw; k++) l.fri_witness.push_back(q());
    dec(l.decommitment);
    l.commitment = h();
  };
  auto entries = [&](std::vector<PublicEntry>& v) {
    uint32_t c = cnt(7);
    for (uint32_t k = 0; k < c; k++) {
      PublicEntry e;
      e.present = u(); e.addr = u();
      for (int j = 0; j < 4; j++) e.value[j] = u();
      e.clock = u();
      if (e.present > 1 || e.addr >= P || e.clock >= P) ok = false;      // canonical M31 words only (M31(x) needs x < P)
      for (int j = 0; j < 4; j++) if (e.value[j] >= P) ok = false;
      v.push_back(e);
    }
  };
  if (u() != 0x434d5031u) { err = "not a proof word stream (bad magic)"; return false; }
  p.config.pow_bits = u(); p.config.log_blowup_factor = u(); p.config.log_last_layer_degree_bound = u(); p.config.n_queries = u();
  uint32_t nc = cnt(5);
  for (uint32_t k = 0; k < nc; k++) p.claim_log_sizes.push_back(u());
  for (uint32_t k = 0; k < nc; k++) p.claimed_sums.push_back(q());
  PublicData& d = p.public_data;
  d.initial_pc = u(); d.initial_fp = u(); d.final_pc = u(); d.final_fp = u(); d.clock = u(); d.initial_root = u(); d.final_root = u();
  for (uint32_t w : {d.initial_pc, d.initial_fp, d.final_pc, d.final_fp, d.clock, d.initial_root, d.final_root}) if (w >= P) ok = false;
  entries(d.program); entries(d.input); entries(d.output);
  p.interaction_pow = u64();
  uint32_t nt = cnt(8);
  for (uint32_t k = 0; k < nt; k++) p.commitments.push_back(h());
  p.sampled_values.resize(nt);
  for (uint32_t t = 0; t < nt && ok; t++) {
    uint32_t ncol = cnt(1);
    p.sampled_values[t].resize(ncol);
    for (uint32_t c = 0; c < ncol && ok; c++) {
      uint32_t ns = cnt(4);
      for (uint32_t s = 0; s < ns; s++) p.sampled_values[t][c].push_back(q());
    }
  }
  p.decommitments.resize(nt);
  for (uint32_t t = 0; t < nt && ok; t++) dec(p.decommitments[t]);
  p.queried_values.resize(nt);
  for (uint32_t t = 0; t < nt && ok; t++) {
    uint32_t nv = cnt(1);
    for (uint32_t k = 0; k < nv; k++) { uint32_t v = u(); if (v >= P) ok = false; p.queried_values[t].push_back(v); }
  }
  p.proof_of_work = u64();
  layer(p.fri_first);
  uint32_t nl = cnt(1);
  p.fri_inner.resize(nl);
  for (uint32_t k = 0; k < nl && ok; k++) layer(p.fri_inner[k]);
  uint32_t np = cnt(4);
  for (uint32_t k = 0; k < np; k++) p.last_layer_poly.push_back(q());
  p.last_layer_log_size = u();
  if (!ok || i != n) { err = "malformed proof word stream"; return false; }
  return true;
}

// the public data's LogUp sum, split by relation, for the AIR check (check.hip; declared in segment_input.hpp)
QM31 public_logup_sum(const PublicData& d, const HostRelations& rel, QM31* per_relation) { return initial_logup_sum(d, rel, per_relation); }

// "" = the proof verifies; otherwise the name of the failed check
// `expected` is the verifier's OWN PcsConfig (verify_cairo_m takes it from the caller, defaulting to REGULAR_96_BITS,
// verifier.rs:17-31): the security level is never read from the proof.  A proof made under another config fails.
std::string verify_proof(const ProofData& pf, const cm_pcs_config& expected) {
  FramingUse framing_use;   // (see Prover: one framing for the whole verification)
  const cm_pcs_config& cfg = expected;
  VerifyPrelude pre;        // everything in front of the queries (verifier_common.hpp)
  {
    std::string err = verify_prelude(pf, cfg, pre);
    if (!err.empty()) return err;
  }
  const std::vector<std::vector<uint32_t>>& logs = pre.logs;
  const std::vector<std::vector<std::vector<CPoint<QM31>>>>& pts = pre.pts;
  const QM31 qcoeff = pre.qcoeff, circle_alpha = pre.circle_alpha;
  const std::vector<QM31>& alphas = pre.alphas;
  const std::vector<uint32_t>& q_logs = pre.q_logs;
  const FoldQueries& queries = pre.queries;
  std::map<uint32_t, std::vector<uint32_t>>& qpos = pre.qpos;
  for (int t = 0; t < 4; t++) {
    std::vector<uint32_t> e;
    for (auto l : logs[t]) e.push_back(l + cfg.log_blowup_factor);
    std::string err = merkle_verify(pf.commitments[t], e, qpos, pf.queried_values[t], pf.decommitments[t]);
    if (!err.empty()) return "Merkle(tree " + std::to_string(t) + "): " + err;
  }
  // fri_answers: DEEP quotient of every size group at its query positions
  std::vector<size_t> cursor(4, 0);
  std::vector<std::vector<QM31>> answers;
  for (auto l : q_logs) {
    std::vector<std::vector<Sample>> cols;
    std::vector<size_t> ncols(4, 0);
    for (int t = 0; t < 4; t++)
      for (size_t c = 0; c < logs[t].size(); c++)
        if (logs[t][c] + cfg.log_blowup_factor == l) {
          ncols[t]++;
          std::vector<Sample> s;
          for (size_t k = 0; k < pts[t][c].size(); k++) s.push_back(Sample{pts[t][c][k], pf.sampled_values[t][c][k]});
          cols.push_back(s);
        }
    std::vector<QM31> ans;
    for (uint32_t qx : qpos[l]) {
      std::vector<uint32_t> row;
      for (int t = 0; t < 4; t++)
        for (size_t k = 0; k < ncols[t]; k++) {
          if (cursor[t] >= pf.queried_values[t].size()) return "InvalidStructure(queried values)";
          row.push_back(pf.queried_values[t][cursor[t]++]);
        }
      ans.push_back(row_quotient(cols, qcoeff, row, domain_point(l, qx)));
    }
    answers.push_back(ans);
  }
  // FRI first layer: rebuild the pairs, check their decommitment, fold every column into the line domain
  std::vector<std::vector<QM31>> folded_first;
  {
    size_t wi = 0;
    std::map<uint32_t, std::vector<uint32_t>> dpos;
    std::vector<uint32_t> dvals, col_logs;
    for (size_t k = 0; k < q_logs.size(); k++) {
      const uint32_t l = q_logs[k];
      std::vector<uint32_t> positions, starts;
      std::vector<std::array<QM31, 2>> pairs;
      if (!rebuild_evals(qpos[l], answers[k], pf.fri_first.fri_witness, wi, positions, pairs, starts)) return "Fri(FirstLayerEvaluationsInvalid)";
      dpos[l] = positions;
      for (auto& pr : pairs) for (auto& v : pr) { uint32_t w4[4]; v.to_u32(w4); dvals.insert(dvals.end(), w4, w4 + 4); }
      col_logs.insert(col_logs.end(), 4, l);
      std::vector<QM31> f;
      for (size_t s = 0; s < pairs.size(); s++) {
        CPoint<M31> p = domain_point(l, starts[s]);
        f.push_back((pairs[s][0] + pairs[s][1]) + circle_alpha * ((pairs[s][0] - pairs[s][1]) * inv(p.y)));
      }
      folded_first.push_back(f);
    }
    if (wi != pf.fri_first.fri_witness.size()) return "Fri(FirstLayerEvaluationsInvalid)";
    std::string err = merkle_verify(pf.fri_first.commitment, col_logs, dpos, dvals, pf.fri_first.decommitment);
    if (!err.empty()) return "Fri(FirstLayerCommitmentInvalid): " + err;
  }
  // inner layers
  FoldQueries lq = queries.fold(1);
  std::vector<QM31> evals(lq.positions.size());
  size_t col = 0;
  uint32_t layer_log = q_logs[0] - 1;
  const QM31 a2 = circle_alpha * circle_alpha;
  for (size_t li = 0; li < pf.fri_inner.size(); li++, layer_log--) {
    while (col < q_logs.size() && q_logs[col] - 1 == layer_log) {
      if (folded_first[col].size() != evals.size()) return "Fri(InnerLayerEvaluationsInvalid)";
      for (size_t i = 0; i < evals.size(); i++) evals[i] = evals[i] * a2 + folded_first[col][i];
      col++;
    }
    const FriLayerProofData& lp = pf.fri_inner[li];
    size_t wi = 0;
    std::vector<uint32_t> positions, starts;
    std::vector<std::array<QM31, 2>> pairs;
    if (!rebuild_evals(lq.positions, evals, lp.fri_witness, wi, positions, pairs, starts) || wi != lp.fri_witness.size())
      return "Fri(InnerLayerEvaluationsInvalid)";
    std::vector<uint32_t> dvals;
    for (auto& pr : pairs) for (auto& v : pr) { uint32_t w4[4]; v.to_u32(w4); dvals.insert(dvals.end(), w4, w4 + 4); }
    std::map<uint32_t, std::vector<uint32_t>> dpos;
    dpos[layer_log] = positions;
    std::string err = merkle_verify(lp.commitment, std::vector<uint32_t>(4, layer_log), dpos, dvals, lp.decommitment);
    if (!err.empty()) return "Fri(InnerLayerCommitmentInvalid " + std::to_string(li) + "): " + err;
    std::vector<QM31> nxt;
    for (size_t s = 0; s < pairs.size(); s++) {
      // LineDomain(half_odds(layer_log)) at bit-reversed position starts[s]
      uint32_t idx = subgroup_gen_index(layer_log + 2) + subgroup_gen_index(layer_log) * bit_reverse(starts[s], layer_log);
      M31 x = point_at_index(idx).x;
      nxt.push_back((pairs[s][0] + pairs[s][1]) + alphas[li] * ((pairs[s][0] - pairs[s][1]) * inv(x)));
    }
    evals = nxt;
    lq = lq.fold(1);
  }
  if (col != q_logs.size()) return "Fri(InvalidNumFriLayers)";
  {  // last layer: evaluate the line polynomial at the remaining query points
    const size_t n = pf.last_layer_poly.size();
    for (size_t i = 0; i < lq.positions.size(); i++) {
      uint32_t idx = subgroup_gen_index(layer_log + 2) + subgroup_gen_index(layer_log) * bit_reverse(lq.positions[i], layer_log);
      M31 x = point_at_index(idx).x;
      QM31 v;
      for (size_t j = 0; j < n; j++) {
        QM31 term = pf.last_layer_poly[j];
        M31 cur = x;
        for (uint32_t b = 0; b < pf.last_layer_log_size; b++) { if ((j >> (pf.last_layer_log_size - 1 - b)) & 1) term = term * cur; cur = double_x(cur); }
        v += term;
      }
      if (v != evals[i]) return "Fri(LastLayerEvaluationsInvalid)";
    }
  }
  return "";
}

}  // namespace cm
