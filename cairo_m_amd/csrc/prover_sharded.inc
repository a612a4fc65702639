// Intra-proof sharding: `world` ranks (one process per GPU) prove ONE segment (SURVEY §8e-2, BASELINE configs[3]).
// Included by prover.hip (same translation unit: it reuses ColumnSet / CommittedTree / Prover); the driver is `ShardedProver` at the
// end of this file, phase by phase like prover.hip's SegmentProver.  Reference units being sharded: the components of `Components::provers()` (components/mod.rs:420-431) for
// everything that is per-component in prove_cairo_m (write_trace, write_interaction_trace, interpolate / evaluate,
// evaluate_constraint_quotients_on_domain, eval_at_point), and ROW RANGES of the evaluation domain for what needs every
// column of a row (Merkle leaf hashing, accumulate_quotients).
//
//   phase                         ownership          exchange (through cm_comm, host-provided: RCCL / gloo / ...)
//   trace gen + histograms        component          all-gather of the 4 partial multiplicity tables (5.4 MB), summed
//   IFFT, LDE (trees 1, 2)        component          all-to-all: column owner -> row-range owner (each rank keeps 1/N rows)
//   Merkle (trees 1, 2)           row range          all-gather of the N sub-roots (32 B); top log2 N levels on every rank
//   LogUp                         component          all-gather of the claimed sums
//   constraints -> composition    component          partial composition coefficients: reduce-scatter + all-gather (sum mod P)
//   OODS sampling                 component          all-gather of the sampled values (~27 KB)
//   DEEP quotients                row range          none: the quotient slices feed the row-sharded FRI layers directly
//   FRI, layers above 2^16 rows   row range          first-layer tree over the quotient slices and every large inner layer: folds are
//                                                    pair-local (no exchange), a tree = local subtree + all-gather of N sub-roots (32 B)
//   FRI, layers <= 2^16, PoW      replicated         one all-gather of the current layer + the small quotient groups, then
//                                                    FriPhase::commit (device-side transcript, k_fri_tail) resumes on every rank
//   decommitment                  row range          one all-gather of the queried values / witness hashes / FRI witness evaluations
//   tree 0, tree 3                columns replicated (cheap transforms), Merkle hashing by row range like trees 1, 2
// The transcript runs identically on every rank (same roots, sums, samples), every rank assembles the same proof, and the
// proof equals the single-GPU one bit for bit (tests/test_gpu_sharded.py: 2 / 4 / 8 ranks on one GPU over gloo;
// tests/test_gpu_sharded_one_rank.py: one rank over the in-library RCCL communicator, inside the test process).
// Transcript steps (round 6): behind every tree the root is hashed from the gathered sub-roots ON THE DEVICE and the single-GPU
// prover's step kernels run right there ("shard_tree_stream" for the four commitment trees, "shard_fri_stream" for the FRI
// layers); the host replays them at the three waits a proof has left — the claimed sums, root 3 (an event in front of the OODS
// evaluations), the sampled values — and once more behind the replicated FRI layers' enqueue.

struct ShardComm {
  const cm_comm* c;
  hipStream_t st;
  uint32_t N, r, logN;
  void need(uint64_t words) const {
    if (words > c->buf_words) throw CmError(1, "cm_prove_sharded: staging buffers too small (" + std::to_string(words) + " words needed, cm_shard_plan reports the size)");
  }
  // Blocking comm (host-provided, e.g. torch.distributed): the collectives run on the host side's own stream — drain ours
  // first; they return when the data has landed.  Stream-ordered comm (CM_COMM_STREAM_ORDERED, e.g. the in-library RCCL one):
  // the collective is enqueued on OUR stream, no host synchronisation on either side.
  bool ordered() const { return (c->flags & CM_COMM_STREAM_ORDERED) != 0; }
  void bind() const { if (ordered() && c->set_stream) c->set_stream(c->ctx, (cm_stream_t)(uintptr_t)st); }
  void all_gather(uint64_t words_per_rank) const {
    need(words_per_rank * N);
    if (!ordered()) CM_HIP(hipStreamSynchronize(st));
    if (c->all_gather(c->ctx, words_per_rank) != 0) throw CmError(1, "cm_prove_sharded: all_gather callback failed");
  }
  void all_to_all_v(const std::vector<uint64_t>& send_words, const std::vector<uint64_t>& recv_words) const {
    if (!ordered()) CM_HIP(hipStreamSynchronize(st));
    if (c->all_to_all_v(c->ctx, send_words.data(), recv_words.data()) != 0) throw CmError(1, "cm_prove_sharded: all_to_all_v callback failed");
  }
  // host words -> every rank's copy, rank-major
  std::vector<uint32_t> gather_host(const std::vector<uint32_t>& mine) const {
    if (N == 1) return mine;   // a lone rank: its own words are everybody's (no staging copy, no collective, no round trip)
    need((uint64_t)mine.size() * N);
    // (pageable source: the copy is staged before the call returns, so `mine` may die; ordered on our stream)
    if (!mine.empty()) CM_HIP(hipMemcpyAsync(c->send_buf, mine.data(), mine.size() * 4, hipMemcpyHostToDevice, st));
    all_gather(mine.size());
    std::vector<uint32_t> all(mine.size() * N);
    if (!all.empty()) {
      CM_HIP(hipMemcpyAsync(all.data(), c->recv_buf, all.size() * 4, hipMemcpyDeviceToHost, st));
      CM_HIP(hipStreamSynchronize(st));
    }
    return all;
  }
};

// ---- the ownership plan --------------------------------------------------------------------------------------------------
// Unit of ownership = the reference's own: a component of `Components::provers()` (components/mod.rs:420-431).  But one component
// can be most of the proof (fibonacci_loop: store_fp_imm alone is 38 % of the cells), so LARGE opcode components are SPLIT:
//   * by ROW RANGE for what is row-local — write_trace (store_fp_imm.rs:147-296 and its siblings: a row is a function of its
//     bundle), the lookup histograms, write_interaction_trace, the constraint quotients: rank r takes rows [r, r+1) * 2^log / N;
//   * by COLUMN for the transforms (IFFT / LDE need whole columns), the LogUp prefix sum (the four cumulative-sum columns of a
//     component stay together) and the OODS sampling: every column of a split component is an item of its own in the packing.
// A rows -> columns transpose (exchange_to_cols) sits between the two.  Everything is a pure function of the component sizes
// and the rank count, so every rank computes the same plan (cm_shard_plan exposes it to the host side).
// Packing: longest processing time first over the items (whole components, or single columns of split components), weight =
// cells (columns x rows, trace + interaction); ties go to the lowest rank.  A component is split when it is an opcode component
// of at least 2^split_min_log rows and heavier than an eighth of a fair share: LPT then keeps every rank within ~1.1 x the mean.
// (struct ShardPlan: prover_api.hpp)
static uint32_t shard_split_min_log() {   // tests lower it so that small proofs exercise the split (CM_SHARD_SPLIT_MIN_LOG; 99 = never split)
  static const uint32_t v = getenv("CM_SHARD_SPLIT_MIN_LOG") ? (uint32_t)atoi(getenv("CM_SHARD_SPLIT_MIN_LOG")) : 12u;
  return v;
}
ShardPlan make_shard_plan(const uint32_t* clog, uint32_t world, bool allow_split) {
  ShardPlan p;
  uint32_t logN = 0;
  while ((1u << logN) < world) logN++;
  p.tr0.assign(air::N_COMPONENTS, 0);
  p.it0.assign(air::N_COMPONENTS, 0);
  uint64_t total = 0;
  std::vector<uint64_t> w(air::N_COMPONENTS);
  size_t ntr = 0, nit = 0;
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    p.tr0[c] = ntr; p.it0[c] = nit;
    ntr += info.n_trace; nit += info.n_interaction;
    w[c] = (uint64_t)(info.n_trace + info.n_interaction) << clog[c];
    total += w[c];
  }
  p.tr_owner.assign(ntr, 0);
  p.it_owner.assign(nit, 0);
  const uint32_t min_log = std::max(shard_split_min_log(), logN + 2);   // a slice keeps at least four rows
  struct Item { uint64_t w; int c; int kind; uint32_t col; };   // kind 0 = whole component, 1 = trace column, 2 = interaction column, 3 = the 4 cumsum columns
  std::vector<Item> items;
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    const bool split = allow_split && world > 1 && c < air::N_OPCODE_COMPONENTS && clog[c] >= min_log && w[c] * 8 * world > total;
    p.owner[c] = split ? -1 : 0;
    if (!split) { items.push_back(Item{w[c], c, 0, 0}); continue; }
    const uint64_t cw = (uint64_t)1 << clog[c];
    for (int k = 0; k < info.n_trace; k++) items.push_back(Item{cw, c, 1, (uint32_t)k});
    for (int k = 0; k + 4 < info.n_interaction; k++) items.push_back(Item{cw, c, 2, (uint32_t)k});
    items.push_back(Item{4 * cw, c, 3, (uint32_t)(info.n_interaction - 4)});
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.w > b.w; });
  for (const Item& it : items) {
    uint32_t best = 0;
    for (uint32_t k = 1; k < world; k++) if (p.load[k] < p.load[best]) best = k;
    p.load[best] += it.w;
    const air::ComponentInfo& info = air::component_info(it.c);
    if (it.kind == 0) {
      p.owner[it.c] = (int)best;
      for (int k = 0; k < info.n_trace; k++) p.tr_owner[p.tr0[it.c] + k] = (int)best;
      for (int k = 0; k < info.n_interaction; k++) p.it_owner[p.it0[it.c] + k] = (int)best;
    } else if (it.kind == 1) p.tr_owner[p.tr0[it.c] + it.col] = (int)best;
    else if (it.kind == 2) p.it_owner[p.it0[it.c] + it.col] = (int)best;
    else for (int k = 0; k < 4; k++) p.it_owner[p.it0[it.c] + it.col + k] = (int)best;
  }
  return p;
}
// staging words a sharded proof needs (upper bound over the exchanges of cm_prove_sharded)
uint64_t shard_staging_words(const uint32_t* clog, const ShardPlan& p, uint32_t world) {
  uint64_t best = 0, max_log = 0;
  for (int c = 0; c < air::N_COMPONENTS; c++) max_log = std::max<uint64_t>(max_log, clog[c]);
  std::vector<uint64_t> tr(world, 0), it(world, 0);
  uint64_t all_tr = 0, all_it = 0, quot = 0, cum = 0;
  std::set<uint32_t> logs;
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    for (int k = 0; k < info.n_trace; k++) tr[p.tr_owner[p.tr0[c] + k]] += (uint64_t)2 << clog[c];
    for (int k = 0; k < info.n_interaction; k++) it[p.it_owner[p.it0[c] + k]] += (uint64_t)2 << clog[c];
    all_tr += (uint64_t)info.n_trace << (clog[c] + 1);
    all_it += (uint64_t)info.n_interaction << (clog[c] + 1);
    if (p.split(c)) cum += (uint64_t)8 << clog[c];        // all-gather of the four cumulative-sum LDE columns
    logs.insert(clog[c] + 1);
  }
  for (uint32_t k = 0; k < world; k++) best = std::max(best, std::max(tr[k], it[k]));   // send side: the rank's own LDE columns
  logs.insert((uint32_t)max_log + 2);
  for (int i = 0; i < air::N_PREPROC; i++) logs.insert(air::PREPROC_LOG[i] + 1);
  for (auto l : logs) quot += (uint64_t)4 << l;
  best = std::max(best, std::max(all_tr, all_it) / world + 1024);       // receive side: 1/N of every column
  best = std::max(best, quot);                                            // all-gather of the quotient columns
  best = std::max(best, cum);
  best = std::max(best, (uint64_t)4 << (max_log + 1));                    // composition coefficients
  best = std::max(best, (uint64_t)world * ((1u << 8) + (1u << 16) + (1u << 20) + (1u << 18)));
  return best + (1u << 20);                                               // + decommitment items, small gathers
}

static Hash32 hash_pair_host(const Hash32& l, const Hash32& r) {
  uint32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0}, m[16];
  memcpy(m, l.data(), 32);
  memcpy(m + 8, r.data(), 32);
  hostch::compress(st, m, 0, 0);
  Hash32 o;
  memcpy(o.data(), st, 32);
  return o;
}

// A committed tree whose LDE columns this rank holds as ROW SLICES (rows [r, r+1) * 2^log / N of every column).
struct SlicedTree {
  std::vector<uint32_t> lde_logs;            // every column of the tree, commitment order
  std::vector<const uint32_t*> slice;        // this rank's slice of each column
  DevBuf arena;                              // slice storage (trees 1 / 2: what the column -> row exchange delivered)
  MerkleTree local;                          // Merkle subtree over the slices (layer k of it = global layer k + logN)
  std::vector<std::vector<Hash32>> top;      // top[k]: the 2^k nodes of global layer k, k <= logN (top[logN] = sub-roots)
  Hash32 root;
  // decommitment planning (filled by sliced_subtree while the GPU hashes): columns sorted by size (stable), like MerkleTree::prepare —
  // layer `log` owns positions [lay_c0[log], lay_c0[log] + lay_n[log]) of the sorted column table
  uint32_t max_log = 0;
  std::vector<uint32_t> lay_c0, lay_n;
  bool leaf_done = false;   // the kernel that produced the largest columns wrote the subtree's leaf layer too
  std::vector<MerkleTree::CommitLaunch> plan;   // the subtree's launches (sliced_prepare), so that such a kernel can be given the leaf layer
  bool planned = false;
};

// Merkle subtree over the rows this rank owns (an ordinary mixed-degree tree whose columns are the slices), sub-roots to
// every rank, top log2(N) levels on the host (they have no columns: every column has at least 2^5 > N rows).
// `later` (tree 0): the sub-roots travel to pinned words behind the collective and the host part (top levels, root) is done by
// complete_sliced() at the caller's next synchronisation point instead of stopping the stream here
struct SlicedLater { hipEvent_t ev = nullptr; uint32_t* land = nullptr; bool pending = false; };
static void complete_sliced(const ShardComm& cm, SlicedTree& out, const uint32_t* sub) {
  const uint32_t N = cm.N, logN = cm.logN;
  out.top.assign(logN + 1, {});
  out.top[logN].resize(N);
  for (uint32_t k = 0; k < N; k++) memcpy(out.top[logN][k].data(), &sub[8 * k], 32);
  for (int k = (int)logN - 1; k >= 0; k--) {
    out.top[k].resize((size_t)1 << k);
    for (size_t i = 0; i < out.top[k].size(); i++) out.top[k][i] = hash_pair_host(out.top[k + 1][2 * i], out.top[k + 1][2 * i + 1]);
  }
  out.root = out.top[0][0];
}
static void complete_sliced(const ShardComm& cm, SlicedTree& out, SlicedLater& later) {
  CM_CHECK(later.pending, "sharding: no sliced tree is waiting for its sub-roots");
  CM_HIP(hipEventSynchronize(later.ev));
  later.pending = false;
  complete_sliced(cm, out, later.land);
}
// the device half: local subtree over the slices, sub-roots to every rank — cm.c->recv_buf holds the N sub-roots (8 words each,
// rank-major) in stream order when this returns
// (two halves: the subtree may be hashed on another stream than the one the collectives live on — tree 0 on its side stream)
// sliced_prepare: column order, the device column table, every layer's buffer and the launch plan — no hashing yet.  A kernel that
// produces the tree's largest columns may then hash the leaf layer itself (local.layers[max local log]) when the plan starts with a
// launch of that layer alone (sliced_leaf_target), and set leaf_done.
static void sliced_prepare(const ShardComm& cm, SlicedTree& out, hipStream_t st) {
  const uint32_t logN = cm.logN;
  std::vector<uint32_t> local_logs(out.lde_logs);
  for (auto& l : local_logs) { CM_CHECK(l >= logN, "sharding: a column is smaller than the rank count"); l -= logN; }
  out.local.prepare(out.slice, local_logs);
  out.local.d_cols = upload(out.local.cols, st);
  out.plan = out.local.plan_commit();   // (adopts local.leaf_prealloc as the leaf layer when one was handed in)
  out.planned = true;
  // (host work behind the launches) the per-layer column ranges the decommitment plan walks — it used to sort the columns again
  // between the proof of work and the gather, with the GPU idle
  out.max_log = 0;
  for (auto l : out.lde_logs) out.max_log = std::max(out.max_log, l);
  out.lay_c0.assign(out.max_log + 1, 0);
  out.lay_n.assign(out.max_log + 1, 0);
  for (auto l : out.lde_logs) out.lay_n[l]++;
  for (int l = (int)out.max_log, c = 0; l >= 0; l--) { out.lay_c0[l] = (uint32_t)c; c += (int)out.lay_n[l]; }
}
// the leaf layer of a prepared subtree if the plan hashes it in a launch of its own (null otherwise)
static uint32_t* sliced_leaf_target(SlicedTree& out) {
  const int nl = (int)out.local.col_logs[0];
  return out.planned && out.plan.size() > 1 && out.plan[0].hi == nl && out.plan[0].lo == nl ? out.local.layers[nl].u32() : nullptr;
}
static void sliced_subtree(const ShardComm& cm, SlicedTree& out, hipStream_t st) {
  if (!out.planned) sliced_prepare(cm, out, st);
  // leaf_done: the DEEP-quotient kernel of the largest size group (k_quotients_rows<.., LEAF>, into local.leaf_prealloc) or the fold
  // that produced the layer (k_fold_leaf) hashed the rows itself: the plan starts at its second launch, as FriPhase::commit does
  if (out.leaf_done) CM_CHECK(sliced_leaf_target(out) != nullptr && !out.local.leaf_prealloc.p, "sharding: the subtree's plan does not start with a launch of the leaf layer alone");
  for (size_t k = out.leaf_done ? 1 : 0; k < out.plan.size(); k++) out.local.run_launch(out.plan[k], st);
}
static void sliced_gather(const ShardComm& cm, SlicedTree& out) {
  CM_HIP(hipMemcpyAsync(cm.c->send_buf, out.local.layers[0].p, 32, hipMemcpyDeviceToDevice, cm.st));
  cm.all_gather(8);
}
static void enqueue_sliced(const ShardComm& cm, SlicedTree& out) {
  sliced_subtree(cm, out, cm.st);
  sliced_gather(cm, out);
}
// the gathered sub-roots -> pinned words behind an event (complete_sliced(cm, out, later) waits for it)
static void sliced_land_later(const ShardComm& cm, SlicedLater& later) {
  static thread_local hipEvent_t ev = nullptr;
  later.ev = thread_event(ev);
  later.land = pinned_words() + PIN_LAST_LAYER + 128;   // (8 N <= 64 words; the FRI phase, much later, owns the slot again)
  CM_HIP(hipMemcpyAsync(later.land, cm.c->recv_buf, 8 * cm.N * 4, hipMemcpyDeviceToHost, cm.st));   // behind the collective
  CM_HIP(hipEventRecord(ev, cm.st));
  later.pending = true;
}
static void finish_sliced(const ShardComm& cm, SlicedTree& out, SlicedLater* later = nullptr) {
  const uint32_t N = cm.N;
  enqueue_sliced(cm, out);
  if (later) { sliced_land_later(cm, *later); return; }
  std::vector<uint32_t> sub(8 * N);
  CM_HIP(hipMemcpyAsync(sub.data(), cm.c->recv_buf, sub.size() * 4, hipMemcpyDeviceToHost, cm.st));   // behind the collective
  CM_HIP(hipStreamSynchronize(cm.st));
  complete_sliced(cm, out, sub.data());
}

// column owner -> row-range owner.  `mine` = (global column index, full LDE column pointer) of the columns this rank
// computed, ascending global index; col_owner / lde_logs cover every column of the tree.
static void exchange_to_rows(const ShardComm& cm, const std::vector<uint32_t>& lde_logs, const std::vector<int>& col_owner,
                             const std::vector<std::pair<uint32_t, const uint32_t*>>& mine, SlicedTree& out, bool enqueue_only = false) {
  // enqueue_only ("shard_tree_stream"): subtree + sub-root all-gather are left on the stream (cm.c->recv_buf holds the N sub-roots in
  // stream order); the caller hashes the top levels on the device (shard_top) and completes the host half at its next synchronisation
  const uint32_t N = cm.N, logN = cm.logN;
  out.lde_logs = lde_logs;
  if (N == 1) {   // a lone rank already holds every row of every column: the slices ARE the columns (no pack, no exchange, no unpack —
                  // three passes over 3.2 GB of LDE per proof of the metric segment)
    out.slice.assign(lde_logs.size(), nullptr);
    for (auto& m : mine) out.slice[m.first] = m.second;
    for (auto* p : out.slice) CM_CHECK(p != nullptr, "sharding: a lone rank owns every column");
    if (enqueue_only) enqueue_sliced(cm, out); else finish_sliced(cm, out);
    return;
  }
  std::vector<uint64_t> send_words(N, 0), recv_words(N, 0);
  uint64_t my_total = 0;
  for (auto& m : mine) my_total += (uint64_t)1 << (lde_logs[m.first] - logN);
  for (uint32_t d = 0; d < N; d++) send_words[d] = my_total;
  for (size_t j = 0; j < lde_logs.size(); j++) recv_words[col_owner[j]] += (uint64_t)1 << (lde_logs[j] - logN);
  uint64_t recv_total = 0;
  std::vector<uint64_t> recv_off(N, 0);
  for (uint32_t s = 0; s < N; s++) { recv_off[s] = recv_total; recv_total += recv_words[s]; }
  cm.need(my_total * N);
  cm.need(recv_total);
  std::vector<CopySeg> segs;
  for (uint32_t d = 0; d < N; d++) {
    uint64_t off = (uint64_t)d * my_total;
    for (auto& m : mine) {
      const uint64_t sl = (uint64_t)1 << (lde_logs[m.first] - logN);
      segs.push_back(CopySeg{m.second + (uint64_t)d * sl, cm.c->send_buf + off, sl});
      off += sl;
    }
  }
  copy_segments(segs, cm.st);
  cm.all_to_all_v(send_words, recv_words);
  out.arena.alloc(recv_total * 4 + 16);
  CM_HIP(hipMemcpyAsync(out.arena.p, cm.c->recv_buf, recv_total * 4, hipMemcpyDeviceToDevice, cm.st));
  out.slice.assign(lde_logs.size(), nullptr);
  std::vector<uint64_t> cur(recv_off);
  for (size_t j = 0; j < lde_logs.size(); j++) {
    out.slice[j] = out.arena.u32() + cur[col_owner[j]];
    cur[col_owner[j]] += (uint64_t)1 << (lde_logs[j] - logN);
  }
  if (enqueue_only) enqueue_sliced(cm, out); else finish_sliced(cm, out);
}
// Row slices of columns every rank holds in full (trees 0 and 3 are replicated): no exchange, the slices point into the
// rank's own copy; only the Merkle hashing is divided.
static void slice_replicated(const ShardComm& cm, const ColumnSet& lde, SlicedTree& out, SlicedLater* later = nullptr, bool enqueue_only = false) {
  out.lde_logs = lde.logs;
  out.slice.resize(lde.size());
  for (size_t j = 0; j < lde.size(); j++) out.slice[j] = lde.ptrs[j] + (uint64_t)cm.r * ((uint64_t)1 << (lde.logs[j] - cm.logN));
  if (enqueue_only) enqueue_sliced(cm, out); else finish_sliced(cm, out, later);
}

// rows -> columns: the transpose behind the row-split phases of a split component (trace generation, LogUp).  Every rank holds
// rows [r, r+1) * 2^(log - logN) of each listed column (`slice`); the column's owner receives all N slices and assembles the
// full column at `full` (only read on the owner).  The list is identical on every rank (same plan), ascending global order.
struct ColMove { uint32_t slog; const uint32_t* slice; int owner; uint32_t* full; };
static void exchange_to_cols(const ShardComm& cm, const std::vector<ColMove>& cols) {
  if (cols.empty()) return;
  const uint32_t N = cm.N, R = cm.r;
  std::vector<uint64_t> send_words(N, 0), recv_words(N, 0);
  uint64_t mine_total = 0, send_total = 0;
  for (auto& c : cols) {
    send_words[c.owner] += (uint64_t)1 << c.slog;
    send_total += (uint64_t)1 << c.slog;
    if ((uint32_t)c.owner == R) mine_total += (uint64_t)1 << c.slog;
  }
  for (uint32_t s = 0; s < N; s++) recv_words[s] = mine_total;
  cm.need(send_total);
  cm.need(mine_total * N);
  std::vector<CopySeg> segs;
  uint64_t off = 0;
  for (uint32_t d = 0; d < N; d++)
    for (auto& c : cols)
      if ((uint32_t)c.owner == d) { segs.push_back(CopySeg{c.slice, cm.c->send_buf + off, (uint64_t)1 << c.slog}); off += (uint64_t)1 << c.slog; }
  copy_segments(segs, cm.st);
  cm.all_to_all_v(send_words, recv_words);
  segs.clear();
  for (uint32_t s = 0; s < N; s++) {
    off = (uint64_t)s * mine_total;
    for (auto& c : cols)
      if ((uint32_t)c.owner == R) { segs.push_back(CopySeg{cm.c->recv_buf + off, c.full + ((uint64_t)s << c.slog), (uint64_t)1 << c.slog}); off += (uint64_t)1 << c.slog; }
  }
  if (!segs.empty()) copy_segments(segs, cm.st);
}

// Decommitment of a row-sharded tree.  The walk (Stwo MerkleProver::decommit, = MerkleTree::plan_decommit) depends only on
// the query positions and the column sizes, so every rank replays it; an item (child hash / column values of a node) is
// fetched by the rank that owns the node's row range, everything is all-gathered once, and a second replay pulls the items
// from the owners' queues in order.
struct ShardedDecommit {
  struct Item { uint8_t kind; uint8_t owner; uint8_t is_query; uint32_t count; };   // kind 0 = hash (count 8), 1 = values, 2 = hash known on the host (count = index into host_hashes), 3 = FRI witness
  std::vector<Item> script;
  std::vector<Hash32> host_hashes;
  std::vector<uint64_t> words_of;   // per rank: words it contributes
};
static void plan_sharded_decommit(const SlicedTree& t, const ShardComm& cm, const std::map<uint32_t, std::vector<uint32_t>>& queries_per_log,
                                  GatherBatch& gb, std::vector<std::pair<int, size_t>>& my_fetch /* (0 hash | 1 run, index) in order */,
                                  ShardedDecommit& sd) {
  const uint32_t logN = cm.logN;
  CM_CHECK(t.lay_n.size() == (size_t)t.max_log + 1, "sharded decommit: the tree has no layer table");
  const uint32_t max_log = t.max_log;
  sd.words_of.assign(cm.N, 0);
  size_t n_q = 0;
  for (auto& kv : queries_per_log) n_q = std::max(n_q, kv.second.size());
  sd.script.reserve(3 * n_q * (max_log + 1));
  my_fetch.reserve(my_fetch.size() + 3 * n_q * (max_log + 1));
  std::vector<uint32_t> last, total;
  last.reserve(n_q); total.reserve(n_q);
  for (int layer_log = (int)max_log; layer_log >= 0; layer_log--) {
    const size_t c0 = t.lay_c0[layer_log];
    const uint32_t ncols = t.lay_n[layer_log];
    const bool has_prev = layer_log < (int)max_log;
    static const std::vector<uint32_t> empty;
    auto it = queries_per_log.find((uint32_t)layer_log);
    const std::vector<uint32_t>& colq = it == queries_per_log.end() ? empty : it->second;
    total.clear();
    size_t pi = 0, qi = 0;
    auto want_hash = [&](uint32_t child_layer, uint32_t node) {
      ShardedDecommit::Item item{};
      item.count = 8;
      if (child_layer <= logN) { item.kind = 2; item.count = (uint32_t)sd.host_hashes.size(); sd.host_hashes.push_back(t.top[child_layer][node]); }
      else {
        const uint32_t sh = child_layer - logN;
        item.kind = 0;
        item.owner = (uint8_t)(node >> sh);
        sd.words_of[item.owner] += 8;
        if (item.owner == cm.r) { my_fetch.push_back({0, gb.add_hash(t.local.layers[sh].u32() + (size_t)(node & ((1u << sh) - 1)) * 8)}); }
      }
      sd.script.push_back(item);
    };
    while (pi < last.size() || qi < colq.size()) {
      uint32_t node;
      if (pi < last.size() && qi < colq.size()) node = std::min(last[pi] / 2, colq[qi]);
      else if (pi < last.size()) node = last[pi] / 2;
      else node = colq[qi];
      if (has_prev) {
        if (pi < last.size() && last[pi] == 2 * node) pi++;
        else want_hash((uint32_t)layer_log + 1, 2 * node);
        if (pi < last.size() && last[pi] == 2 * node + 1) pi++;
        else want_hash((uint32_t)layer_log + 1, 2 * node + 1);
      }
      const bool isq = qi < colq.size() && colq[qi] == node;
      if (isq) qi++;
      if (ncols) {
        CM_CHECK((uint32_t)layer_log >= logN, "sharded decommit: a column is smaller than the rank count");
        const uint32_t sh = (uint32_t)layer_log - logN;
        ShardedDecommit::Item item{};
        item.kind = 1; item.owner = (uint8_t)(node >> sh); item.is_query = isq ? 1 : 0; item.count = ncols;
        sd.words_of[item.owner] += ncols;
        if (item.owner == cm.r) {
          // the local tree keeps the slices sorted the same way: its column table positions [c0, ci) are this layer's columns
          my_fetch.push_back({1, gb.add_run(t.local.dcols() + c0, ncols, node & ((1u << sh) - 1))});
        }
        sd.script.push_back(item);
      }
      total.push_back(node);
    }
    last.swap(total);
  }
}

// compute_decommitment_positions_and_witness_evals of a ROW-SHARDED layer (plan_fri_positions with ownership): the witness
// evaluation at position p is fetched by the rank whose slice holds row p
static void plan_fri_positions_sharded(const ShardComm& cm, uint32_t log, uint32_t* const slice4[4], const std::vector<uint32_t>& queries,
                                       std::vector<uint32_t>& positions, GatherBatch& gb, std::vector<std::pair<int, size_t>>& my_fetch,
                                       ShardedDecommit& sd) {
  const uint32_t sh = log - cm.logN;
  sd.words_of.assign(cm.N, 0);
  positions.reserve(2 * queries.size());
  sd.script.reserve(2 * queries.size());
  my_fetch.reserve(my_fetch.size() + 2 * queries.size());
  size_t i = 0;
  while (i < queries.size()) {
    const uint32_t start = (queries[i] >> 1) << 1;
    size_t j = i;
    while (j < queries.size() && (queries[j] >> 1) == (queries[i] >> 1)) j++;
    size_t qi = i;
    for (uint32_t pos = start; pos < start + 2; pos++) {
      positions.push_back(pos);
      if (qi < j && queries[qi] == pos) { qi++; continue; }
      ShardedDecommit::Item item{};
      item.kind = 3; item.owner = (uint8_t)(pos >> sh); item.count = 4;
      sd.words_of[item.owner] += 4;
      if (item.owner == cm.r) {
        my_fetch.push_back({2, gb.word_addrs.size()});
        for (int k = 0; k < 4; k++) gb.add_word(slice4[k] + (pos & ((1u << sh) - 1)));
      }
      sd.script.push_back(item);
    }
    i = j;
  }
}
// one decommitment script and where its items go
struct ShardSection {
  ShardedDecommit sd;
  std::vector<std::pair<int, size_t>> fetch;   // this rank's items in script order: (0 hash | 1 run | 2 four words, index into the gather)
  const GatherBatch* gb = nullptr;             // the gather the indices refer to
  MerkleDecommitment* d = nullptr;             // hashes / column witness of a tree
  std::vector<uint32_t>* qv = nullptr;         // queried values of a tree (null: dropped — the FRI trees)
  std::vector<QM31>* wit = nullptr;            // FRI witness evaluations
};
// A FRI layer committed by ROW RANGE: every rank holds rows [r, r+1) * 2^log / N of the layer's four coordinate columns
struct ShardedFriLayer { uint32_t log = 0; ColumnSet slice; SlicedTree tree; };
// layers of at most 2^stop rows are gathered and finished by FriPhase::commit on every rank (A/B and tests: CM_SHARD_FRI_STOP_LOG;
// 99 = the replicated FRI of rounds 2-3)
static uint32_t shard_fri_stop_log() { return (uint32_t)tune(T_SHARD_FRI_STOP_LOG); }   // (tuning key "shard_fri_stop_log", default 16)

// One proof sharded over the ranks: the eight phases of prover.hip's SegmentProver, in transcript order.  Each phase enqueues its
// kernels and collectives and returns at the next point where the transcript needs a device result.  What crosses a phase boundary
// is a member, declared in the order in which it is made: members die in reverse order, and that order is behaviour (every Fork
// dies before `P`; see the guards).  The private methods named like the old lambdas (commit_own, sums_arrive, check_halo,
// fri_replay, check_flags) are where a later phase finishes an earlier phase's wait.
struct ShardedProver : ProofContext {
  HostTrace hm{"[shard]", 44, "CM_SHARD_MARKS"};   // host time between the marks of one sharded proof (development aid)
  const cm_comm& comm_c;
  AffinityScope cpu_scope;   // restored when the proof returns (pool.hip)
  Prover P;
  hipStream_t st; Channel& ch; ShardComm cm;
  const uint32_t N, R, B;                    // ranks, this rank, log_blowup_factor
  uint32_t logN = 0;
  ShardPlan plan;
  const std::vector<int>&tr_owner, &it_owner;   // plan.tr_owner / plan.it_owner
  bool tree_stream = false;   // "shard_tree_stream", see setup()
  // the device words of the tree_stream transcript steps (d_ts) ...
  enum : uint32_t { TS_CHAN = 0, TS_COEFF = 16, TS_ROOT2_LOG = 20, TS_ROOT1 = 32, TS_SUB1 = 40, TS_STEP1 = 104, TS_ROOT2 = 120, TS_SUB2 = 128,
                    TS_ROOT3 = 192, TS_SUB3 = 200, TS_STEP3 = 264, TS_WORDS = 280 };
  DevBuf d_ts; uint32_t* ts = nullptr;
  // ... and the pinned words their results land in: the sub-roots of trees 1 / 2 / 3 (tree 0's sit at + 128; the FRI phase, much
  // later, owns the slot again), the halo exchange's error word, and — dedicated, no other download of the thread lands there —
  // every rank's claimed sums (PIN_SHARD_SUMS, read by sums_arrive) and the sharded FRI layers' words (PIN_SHARD_FRI, fri_replay)
  enum : uint32_t { PIN_SUB1 = PIN_LAST_LAYER + 192, PIN_SUB2 = PIN_LAST_LAYER + 256, PIN_SUB3 = PIN_LAST_LAYER + 320, PIN_HALO_ERR = PIN_FLAG + 1,
                    SW = air::N_COMPONENTS * 4 + 2 /* a rank's words in the sums' exchange: sums, lookup flag, FRI plan */ };
  static_assert(PIN_SUB3 + 64 <= PIN_LAST_LAYER_END && PIN_LAST_LAYER_END <= PIN_SHARD_SUMS && PIN_SHARD_SUMS + SW * 8 <= PIN_SHARD_FRI && PIN_SHARD_FRI < PIN_WORDS, "pinned slot layout");
  uint32_t *pin_sub1 = nullptr, *pin_sub2 = nullptr, *pin_sub3 = nullptr, *pin_halo_err = nullptr;
  ProofTwiddles own_tw;
  std::unique_ptr<Fork> tw_fork; hipStream_t s0 = nullptr;   // twiddles, constant columns, tree 0's transforms (setup .. trace_commit)
  // An exception between a fork and its join must not hand the buffers declared in FRONT of these guards (own_tw, P.trees[0]) back
  // to the pool under the side stream's kernels: the guards are declared behind them, so they drain first.
  DrainOnExit s0_guard;
  std::unique_ptr<Fork> pp_fork; DrainOnExit pp_guard;   // tree_stream: tree 0's chain (IFFT, LDE, subtree) forks behind the trace kernels
  // ---- trace_commit ----
  SlicedTree sl0, sl1, sl2, sl3; SlicedLater sl0_later; ColumnSet pp_evals;
  std::vector<size_t> ltr0, lit0;   // first column of every component among this rank's own columns of trees 1 / 2 (global: tr0 / it0)
  std::vector<uint32_t> ltr_logs, lit_logs;
  std::vector<int> ltr_of, lit_of;      // global column -> index among this rank's own columns (-1: somebody else's)
  // split components: this rank's ROW slice of every trace / interaction column (trace domain, plain row order: row r = bundle r)
  struct SplitComp { int c; uint32_t slog; ColumnSet tr_slice, it_slice, cum_lde, cum_prev; };
  std::vector<std::unique_ptr<SplitComp>> splits;
  ColumnSet tr_evals;       // own components only (at least a dummy word when this rank owns nothing); released behind tree 2
  static constexpr size_t HW = ((size_t)1 << 8) + ((size_t)1 << 16) + ((size_t)1 << 20) + ((size_t)1 << 18);
  DevBuf hist, hist_sum, flag;   // (kept until the proof returns, as ever: the pool then hands later phases the same blocks)
  CommittedTree own1, own2;       // coefficients + full LDE of the OWN columns of trees 1 and 2
  DevBuf drel;
  // ---- interaction ----
  std::vector<int> my_comps; DevBuf d_sums;   // components whose cumulative-sum columns (and claimed sum) this rank computes
  std::vector<DevBuf> tail_scratch;     // scratch of the LogUp tail when it runs on a side stream: alive until the host has seen the sums
  Prover::DeferredCols late_cols;       // the running-sum columns of tree 2: transformed behind the tail (late_cols.ready)
  const uint32_t* sums_land = nullptr;   // pinned: this rank's sums (compact), or every rank's gathered words (sums_gathered)
  bool sums_gathered = false, halo_pending = false;
  hipEvent_t ev_sums = nullptr, ev_root3 = nullptr, ev_fri_back = nullptr;
  ColumnSet it_evals;
  DevBuf d_powers;                      // `powers` on the device
  // ---- oods_sampling / deep_quotients ----
  size_t n_cols_t[4] = {0, 0, 0, 0};
  DevBuf d_oods_out, d_oods_table, d_oods_tmp;   // (kept until the proof returns, like hist)
  std::vector<uint32_t> q_logs; std::vector<ColumnSet> quotients;
  std::vector<QuotientGroup> gs;   // the quotient size groups, largest first; out = this rank's rows of the four coordinate columns
  // ---- FRI: the row-sharded part (first-layer tree + the large inner layers), the replicated rest ----
  SlicedTree fri_first; std::vector<std::unique_ptr<ShardedFriLayer>> sfl; FriPhase fri;
  DevBuf d_qblob;                  // the DEEP-quotient plan on the device: released behind the quotient launches
  size_t o_qjobs = 0, n_qjobs = 0, qi_next = 0, fri_slot_words = 0;
  std::vector<std::pair<QuotientArgs, double>> qargs;
  uint32_t last_log = 0, layer_log = 0; QM31 alpha_c;
  ColumnSet cur;          // this rank's rows of the layer being built
  bool cur_valid = false, shard_fri = false, fri_stream = false;
  DevBuf d_fs;                              // {device channel, per tree: challenge, root, sub-roots}: alive until the proof returns
  const uint32_t* fri_back_land = nullptr;  // pinned: the slots of d_fs, valid behind ev_fri_back
  std::vector<SlicedTree*> fri_order; const uint32_t *rs_d_chan = nullptr, *rs_d_alpha_c = nullptr;
  ColumnSet full_layer;   // the hand-over layer, whole, on every rank
  ShardedProver(const DeviceInput& din_, const cm_pcs_config& cfg_, const cm_comm& comm_)
      : ProofContext(din_, cfg_), comm_c(comm_), st(nullptr), ch(P.ch),
        cm{&comm_, nullptr, comm_.world, comm_.rank, 0}, N(comm_.world), R(comm_.rank), B(cfg_.log_blowup_factor),
        tr_owner(plan.tr_owner), it_owner(plan.it_owner) {
    release_thread_parked();   // a single-GPU proof of this thread may have parked its FRI phase and quotient columns (prover.hip)
    start(P);
    st = cm.st = P.st;
  }
  ProofData* run() {
    setup();
    trace_commit();
    interaction();
    composition();
    oods_sampling();
    deep_quotients();
    fri_and_pow();
    decommit();
    finish_common(P);
    return out.release();
  }

 private:
  bool mine(int c) const { return plan.owner[c] == (int)R; }   // whole components of this rank
  bool split(int c) const { return plan.split(c); }            // the component is split over all ranks (ShardPlan)
  std::vector<uint32_t> lde_of(std::vector<uint32_t> v) const { for (auto& l : v) l += B; return v; }
  uint32_t col_log(int t, uint32_t c) const { return t == 0 ? air::PREPROC_LOG[c] : t == 1 ? tr_logs[c] : t == 2 ? it_logs[c] : comp_log; }
  int col_owner_of(int t, uint32_t c) const { return t == 1 ? tr_owner[c] : t == 2 ? it_owner[c] : 0; }
  // rank geometry, config checks, the ownership plan, twiddles (side stream), transcript setup (prover.rs:33-66)
  void setup() {
    cm.bind();   // a stream-ordered comm enqueues its collectives on this proof's stream
    CM_CHECK(cm.N >= 1 && cm.N <= 8 && (cm.N & (cm.N - 1)) == 0 && cm.r < cm.N, "cm_prove_sharded: world must be 1, 2, 4 or 8");
    while ((1u << cm.logN) < cm.N) cm.logN++;
    logN = cm.logN;
    // log_blowup_factor B: the commitment domain of a column of 2^log rows is CanonicCoset(log + B); the constraints are evaluated
    // on CanonicCoset(log + 1).  With B = 1 (REGULAR_96_BITS) that IS the committed LDE; with B > 1 every owner evaluates its
    // polynomials on the (log + 1) domain separately, as Stwo and the single-GPU prover do — and components stay whole (the
    // row-range constraints of a split component read the committed LDE slices the exchange leaves on every rank).
    CM_CHECK(B >= 1 && B <= 4, "PcsConfig: log_blowup_factor must be in 1..4");
    size_components();
    column_offsets();
    plan = make_shard_plan(clog, N, /*allow_split=*/B == 1);
    // (round 6) "shard_tree_stream": the commitment trees' transcript steps stay ON THE STREAM like the sharded FRI layers' — behind a
    // tree's sub-root all-gather k_shard_top hashes the top log2 N levels on the device and the single-GPU prover's transcript kernels
    // take the root from there: k_step_pow_relations behind tree 1 (mix_root, interaction proof of work, Relations::draw -> the LogUp
    // kernels start), k_chan_init_mix_root_draw + k_coeff_powers behind tree 2 (-> the constraint kernels start), k_chan_mix_root_draw
    // behind tree 3 (-> the OODS evaluations start from the felt in device memory).  The host rebuilds the top levels from the copied-
    // back sub-roots and replays every step at the two synchronisation points that are left before FRI (the claimed sums; the sampled
    // values), refusing the proof on any mismatch.  0 = the host-driven form: a round trip per root, the PoW and the halo check.
    tree_stream = tune(T_SHARD_TREE_STREAM) != 0 && !framing().hash_node_rfc;
    if (tree_stream) d_ts.alloc(TS_WORDS * 4);
    ts = d_ts.u32();
    pin_sub1 = pinned_words() + PIN_SUB1; pin_sub2 = pinned_words() + PIN_SUB2; pin_sub3 = pinned_words() + PIN_SUB3; pin_halo_err = pinned_words() + PIN_HALO_ERR;
    // (round 5) twiddles, constant columns and the transforms of tree 0 on a side stream, like the single-GPU prover: nothing of trace
    // generation reads them, and both are chains of short launches.  Joined — and tree 0 hashed by row range on the main stream,
    // where the collectives live — behind the trace kernels.
    tw_fork.reset(new Fork(st));
    s0_guard.s = s0 = tw_fork->stream(Fork::N - 1);
    own_tw.build(comp_log + cfg.log_blowup_factor, s0);
    P.tw = &own_tw.t;

    // ---- transcript setup (prover.rs:33-36, 62-66) ----
    pf.public_data = din.public_data;
    mix_config_and_public_data(ch, cfg, pf.public_data);
    P.tick("setup");
  }
  // every rank must agree on a failure of trace generation: the flags are gathered
  // ... and, in the same exchange, that every rank runs the same FRI plan: CM_SHARD_FRI_STOP_LOG is read per process, and ranks
  // that disagree on it would issue different collectives further down and dead-lock
  void check_flags(const std::vector<uint32_t>& all, size_t per_rank, size_t at) const {
    for (uint32_t k = 0; k < N; k++) {
      CM_CHECK(all[per_rank * k + at] == 0, "trace generation: a range-check / bitwise lookup value is out of range");
      CM_CHECK(all[per_rank * k + at + 1] == shard_fri_stop_log(), "cm_prove_sharded: CM_SHARD_FRI_STOP_LOG differs between the ranks");
    }
  }
  // IFFT + LDE of the own columns, then column owner -> row-range owner, Merkle subtree, sub-roots
  // (round 5) the transforms go through the single-GPU prover's commitment code without its Merkle half: fused inverse / forward
  // sweeps (k_fft_fused_rb), one launch for all small columns, tree 2 interpolated in place group by group — they used to be plain
  // interpolate + evaluate passes behind a separate in-place interpolation and two stream synchronisations
  void commit_own(CommittedTree& t, ColumnSet* evals, bool from_coeffs, bool evals_in_place, const std::vector<uint32_t>& all_logs,
                  const std::vector<int>& col_owner, SlicedTree& sl, const std::function<void()>& between = nullptr,
                  const Prover::DeferredCols* defer = nullptr) {
    P.commit_enqueue(t, evals, from_coeffs, st, /*with_merkle=*/false, evals_in_place, nullptr, defer);
    if (between) between();   // work that belongs behind the transforms just enqueued and in front of the tree's exchange
    std::vector<std::pair<uint32_t, const uint32_t*>> mine_cols;
    size_t li = 0;
    for (size_t j = 0; j < all_logs.size(); j++)
      if ((uint32_t)col_owner[j] == R) mine_cols.push_back({(uint32_t)j, t.lde.ptrs[li++]});
    exchange_to_rows(cm, lde_of(all_logs), col_owner, mine_cols, sl, /*enqueue_only=*/tree_stream);
  }
  // tree 0 (columns replicated, hashing row-sharded), tree 1 (own components), lookup flags, interaction PoW + relations (prover.rs:70-94)
  void trace_commit() {
    {
      std::vector<uint32_t> logs(air::PREPROC_LOG, air::PREPROC_LOG + air::N_PREPROC);
      pp_evals.alloc(logs, st);
      for (int i = 0; i < air::N_PREPROC; i++) launch_preproc(i, logs[i], pp_evals.ptrs[i], s0);
      // (tree 0's IFFT + LDE — on every rank, hashing by row range — are enqueued BEHIND the trace-generation launches below: issued
      // here, the host time of that chain of ~15 short launches delayed the first trace kernel by ~0.25 ms, round-6 timeline)
    }
    P.tick("preprocessed");

    // ---- column bookkeeping of trees 1 and 2: owner of every column (global order: column_offsets), local (own) column sets ----
    ltr0.assign(air::N_COMPONENTS, 0); lit0.assign(air::N_COMPONENTS, 0);
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      ltr0[c] = ltr_logs.size(); lit0[c] = lit_logs.size();   // (meaningful for whole components of this rank: their columns are consecutive)
      for (int k = 0; k < air::component_info(c).n_trace; k++) {
        const bool own = (uint32_t)tr_owner[tr0[c] + k] == R;
        ltr_of.push_back(own ? (int)ltr_logs.size() : -1);
        if (own) ltr_logs.push_back(clog[c]);
      }
      for (int k = 0; k < air::component_info(c).n_interaction; k++) {
        const bool own = (uint32_t)it_owner[it0[c] + k] == R;
        lit_of.push_back(own ? (int)lit_logs.size() : -1);
        if (own) lit_logs.push_back(clog[c]);
      }
    }
    for (int c = 0; c < air::N_COMPONENTS; c++)
      if (split(c)) { splits.emplace_back(new SplitComp()); splits.back()->c = c; splits.back()->slog = clog[c] - logN; }
    // ---- tree 1: execution trace of the own components ----
    tr_evals.alloc(ltr_logs, st);
    hist.alloc(HW * 4);
    flag.alloc(4);
    {
      CM_HIP(hipMemsetAsync(flag.p, 0, 4, st));
      CM_HIP(hipMemsetAsync(hist.p, 0, HW * 4, st));
      HistPtrs h;
      h.rc8 = hist.u32(); h.rc16 = h.rc8 + (1u << 8); h.rc20 = h.rc16 + (1u << 16); h.bitwise = h.rc20 + (1u << 20);
      h.error_flag = flag.u32();
      std::vector<SmallTraceJob> small_trace;
      for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++)
        if (mine(c) && clog[c] <= SMALL_COMPONENT_MAX_LOG)
          small_trace.push_back(SmallTraceJob{din.bundles[c].p, (uint32_t)in.n_bundles[c], tr_evals.dev(ltr0[c]), clog[c], c});
      DevBuf d_small_trace = upload(small_trace, st);
      {
        Fork fk(st);   // (round 5) whole components: trace + histogram in one launch each, on side streams (histogram adds commute)
        if (!small_trace.empty()) launch_trace_hist_small(d_small_trace.as<SmallTraceJob>(), (uint32_t)small_trace.size(), din.data_accesses.p, h, fk.stream(Fork::N - 2));
        int spos = 0;
        for (int c : by_size_all) {   // large components first: the largest on the main stream
          if (c >= air::N_OPCODE_COMPONENTS || !mine(c) || clog[c] <= SMALL_COMPONENT_MAX_LOG) continue;
          launch_opcode_trace_hist(c, din.bundles[c].p, (uint32_t)in.n_bundles[c], din.data_accesses.p, clog[c], tr_evals.dev(ltr0[c]), h,
                                   fk.stream(spos == 0 ? Fork::main_or(0) : spos % (Fork::N - 2)));
          spos++;
        }
        // the builtins' traces inside the region too (the single-GPU prover's placement): they ran one after the other on the main
        // stream behind the join, ~70 us of launch latency in the round-6 timeline
        if (mine(air::C_MEMORY))
          launch_memory_trace(din.init_mem.p, (uint32_t)in.n_initial_memory, din.fin_mem.p, (uint32_t)in.n_final_memory, in.initial_root, in.final_root,
                              clog[air::C_MEMORY], tr_evals.dev(ltr0[air::C_MEMORY]), fk.stream(air::C_MEMORY));
        if (mine(air::C_MERKLE))
          launch_merkle_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree, in.initial_root, in.final_root,
                              clog[air::C_MERKLE], tr_evals.dev(ltr0[air::C_MERKLE]), fk.stream(air::C_MERKLE));
        if (mine(air::C_CLOCK_UPDATE))
          launch_clock_update_trace(din.clock_updates.p, (uint32_t)in.n_clock_updates, clog[air::C_CLOCK_UPDATE], tr_evals.dev(ltr0[air::C_CLOCK_UPDATE]), fk.stream(air::C_CLOCK_UPDATE));
        if (mine(air::C_POSEIDON2))
          launch_poseidon2_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree, clog[air::C_POSEIDON2],
                                 tr_evals.dev(ltr0[air::C_POSEIDON2]), fk.stream(air::C_POSEIDON2));
        fk.join();
      }
      if (!tree_stream) P.commit_enqueue(P.trees[0], &pp_evals, false, s0, /*with_merkle=*/false);   // tree 0: IFFT + LDE, next to the trace kernels
      // split components: every rank writes the trace rows of ITS row range (a row is a function of its bundle) and counts their
      // lookups; the slices then travel to the column owners, which transform whole columns
      for (auto& sc : splits) {
        const int c = sc->c;
        sc->tr_slice.alloc(std::vector<uint32_t>(air::component_info(c).n_trace, sc->slog), st);
        const uint64_t row0 = (uint64_t)R << sc->slog, nb = in.n_bundles[c];
        const uint32_t n_local = nb > row0 ? (uint32_t)std::min<uint64_t>(nb - row0, (uint64_t)1 << sc->slog) : 0u;
        launch_opcode_trace(c, (const uint8_t*)din.bundles[c].p + row0 * sizeof(air::Bundle), n_local, din.data_accesses.p, sc->slog,
                            sc->tr_slice.dev(), st);
        launch_hist(c, (const uint32_t* const*)sc->tr_slice.dev(), sc->slog, h, st);
      }
      {
        std::vector<ColMove> mv;
        for (auto& sc : splits)
          for (int k = 0; k < air::component_info(sc->c).n_trace; k++) {
            const size_t j = tr0[sc->c] + k;
            mv.push_back(ColMove{sc->slog, sc->tr_slice.ptrs[k], tr_owner[j], ltr_of[j] >= 0 ? tr_evals.ptrs[ltr_of[j]] : nullptr});
          }
        exchange_to_cols(cm, mv);
      }
      // tree 0: its transforms have run next to the kernels above; hashing by row range + sub-root all-gather here, the host part
      // (top levels, root) at the synchronisation point below — nothing of trace generation needs root 0
      tw_fork->join();
      s0_guard.joined = true;
      if (tree_stream) {
        // tree 0 whole — transforms AND the Merkle subtree of this rank's rows — on a side stream forked HERE (twiddles joined, trace
        // kernels launched), next to tree 1's transforms as in the single-GPU prover; only the 32-byte all-gather of its sub-roots
        // goes on the main stream, behind those transforms (the collectives live there)
        pp_fork.reset(new Fork(st));
        hipStream_t s0b = pp_fork->stream(Fork::N - 1);
        pp_guard.s = s0b;
        P.commit_enqueue(P.trees[0], &pp_evals, false, s0b, /*with_merkle=*/false);
        sl0.lde_logs = P.trees[0].lde.logs;
        sl0.slice.resize(P.trees[0].lde.size());
        for (size_t j = 0; j < sl0.slice.size(); j++) sl0.slice[j] = P.trees[0].lde.ptrs[j] + (uint64_t)R * ((uint64_t)1 << (sl0.lde_logs[j] - logN));
        sliced_subtree(cm, sl0, s0b);
      } else slice_replicated(cm, P.trees[0].lde, sl0, &sl0_later);
      // multiplicity tables = sum of every rank's partial histogram (components/mod.rs:139-160 chains all opcode components)
      const uint32_t* hsum = hist.u32();   // (a lone rank's histogram IS the sum)
      if (N > 1) {
        cm.need(HW * N);
        hist_sum.alloc(HW * 4);
        CM_HIP(hipMemcpyAsync(comm_c.send_buf, hist.p, HW * 4, hipMemcpyDeviceToDevice, st));
        cm.all_gather(HW);
        sum_copies(comm_c.recv_buf, N, HW, HW, hist_sum.u32(), false, st);
        hsum = hist_sum.u32();
      }
      const size_t off[4] = {0, (size_t)1 << 8, ((size_t)1 << 8) + ((size_t)1 << 16), ((size_t)1 << 8) + ((size_t)1 << 16) + ((size_t)1 << 20)};
      const int rc[4] = {air::C_RC8, air::C_RC16, air::C_RC20, air::C_BITWISE};
      for (int k = 0; k < 4; k++)
        if (mine(rc[k])) CM_HIP(hipMemcpyAsync(tr_evals.ptrs[ltr0[rc[k]]], hsum + off[k], (size_t)4 << clog[rc[k]], hipMemcpyDeviceToDevice, st));
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_FLAG, flag.p, 4, hipMemcpyDeviceToHost, st));
      if (!tree_stream) {
        CM_HIP(hipStreamSynchronize(st));
        complete_sliced(cm, sl0, sl0_later);   // transcript order (prover.rs:70-82): root 0 in front of the claim and root 1
        P.trees[0].root = sl0.root;
        ch.mix_root(sl0.root);
        check_flags(cm.gather_host({pinned_words()[PIN_FLAG], shard_fri_stop_log()}), 2, 0);
      }
      // (tree_stream: the flag is read at the claimed sums' synchronisation point and travels with them; root 0 is waited for
      // below, with tree 1's transforms already enqueued)
    }
    P.tick("trace_gen");
    drel.alloc(sizeof(DevRelations));
    if (tree_stream) {
      commit_own(own1, &tr_evals, false, false, tr_logs, tr_owner, sl1, [&] {
        pp_fork->join();
        pp_guard.joined = true;
        sliced_gather(cm, sl0);
        sliced_land_later(cm, sl0_later);
      });
      complete_sliced(cm, sl0, sl0_later);   // root 0 arrives behind tree 1's transforms; the GPU is busy with tree 1's subtree
      P.trees[0].root = sl0.root;
      ch.mix_root(sl0.root);
      mix_claim(ch, pf, clog);
      // root 1 -> interaction proof of work -> relation challenges, all behind the all-gather (prover.hip trace_commit)
      static_assert(sizeof(DevRelations) == 4 * 4 * (air::N_RELATIONS + air::N_RELATIONS * air::MAX_REL_SIZE), "DevRelations layout");
      shard_top(comm_c.recv_buf, N, ts + TS_ROOT1, ts + TS_SUB1, st);
      uint32_t cw[9];
      channel_words(ch, cw);
      step_pow_relations(cw, ts + TS_ROOT1, INTERACTION_POW_BITS, air::N_RELATIONS, air::MAX_REL_SIZE, drel.u32(), drel.u32() + 4 * air::N_RELATIONS,
                         ts + TS_STEP1, st);
      CM_HIP(hipMemcpyAsync(pin_sub1, ts + TS_SUB1, 8 * N * 4, hipMemcpyDeviceToHost, st));
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_STEP1, ts + TS_STEP1, 16 * 4, hipMemcpyDeviceToHost, st));
      P.tick("trace_commit");
    } else {
      commit_own(own1, &tr_evals, false, false, tr_logs, tr_owner, sl1);
      // transcript order (prover.rs:70-82): root 0 (mixed above), claim, root 1
      mix_claim(ch, pf, clog);
      ch.mix_root(sl1.root);
      P.tick("trace_commit");

      // ---- interaction PoW + relations (prover.rs:90-94): replicated ----
      pf.interaction_pow = grind_gpu(ch.digest.data(), INTERACTION_POW_BITS, st);
      ch.mix_u64(pf.interaction_pow);
      DevRelations drel_h;
      draw_relations(ch, hrel, drel_h);
      stage_upload(drel.p, &drel_h, sizeof(DevRelations), st);
    }
  }
  // the LogUp columns of the own components: the fork region of their kernels (`jobs`: the tails that follow)
  void logup_launches(std::vector<LogupTailJob>& jobs, DevBuf& d_small) {
    // split components first: the LogUp rows of this rank's row range, then rows -> column owners
    for (auto& sc : splits) {
      const int c = sc->c;
      sc->it_slice.alloc(std::vector<uint32_t>(air::component_info(c).n_interaction, sc->slog), st);
      launch_logup(c, (const uint32_t* const*)sc->tr_slice.dev(), (const uint32_t* const*)pp_evals.dev(), sc->slog, drel.as<DevRelations>(),
                   sc->it_slice.dev(), st);
    }
    {
      std::vector<ColMove> mv;
      for (auto& sc : splits)
        for (int k = 0; k < air::component_info(sc->c).n_interaction; k++) {
          const size_t j = it0[sc->c] + k;
          mv.push_back(ColMove{sc->slog, sc->it_slice.ptrs[k], it_owner[j], lit_of[j] >= 0 ? it_evals.ptrs[lit_of[j]] : nullptr});
        }
      exchange_to_cols(cm, mv);
    }
    // the LogUp tail (claimed sum + prefix sum) of a component runs where its four cumulative-sum columns live: the owner of a
    // whole component, or the rank the plan gave those columns of a split one
    for (int c = 0; c < air::N_COMPONENTS; c++) if (plan.cum_owner(c) == (int)R) my_comps.push_back(c);
    jobs.resize(my_comps.size());
    std::vector<SmallLogupJob> small_jobs;
    uint32_t small_max_log = 0;
    for (int c : my_comps)
      if (!split(c) && clog[c] <= SMALL_COMPONENT_MAX_LOG) {
        small_jobs.push_back(SmallLogupJob{(const uint32_t* const*)tr_evals.dev(ltr0[c]), it_evals.dev(lit0[c]), clog[c], c});
        small_max_log = std::max(small_max_log, clog[c]);
      }
    d_small = upload(small_jobs, st);
    {
      // (round 5) the components' kernels are independent: side streams, the batched small components first (latency-bound, hidden
      // under the large ones), like the single-GPU prover's region
      // (round 6) launch order: the batched small components FIRST and on the main stream (275 us of pure latency on a handful of
      // CUs — on side stream 4 they shared a hardware queue with side stream 3 and the region's largest kernel queued behind them,
      // round-6 timeline), then the components by descending size alternating over side streams 1 and 2: three streams on four
      // hardware queues (with a third side stream one of them shared the main stream's queue in one session of two and a 0.1 ms
      // kernel waited for the small batch to finish)
      Fork fk(st);
      if (!small_jobs.empty())
        launch_logup_small(d_small.as<SmallLogupJob>(), (uint32_t)small_jobs.size(), small_max_log, (const uint32_t* const*)pp_evals.dev(), drel.as<DevRelations>(), fk.stream(Fork::MAIN));
      for (size_t k = 0; k < my_comps.size(); k++) {
        const int c = my_comps[k];
        const air::ComponentInfo& info = air::component_info(c);
        for (int q = 0; q < 4; q++) jobs[k].col[q] = it_evals.ptrs[lit_of[it0[c] + info.n_interaction - 4 + q]];
        jobs[k].log_size = clog[c];
      }
      int spos = 0;
      for (int c : by_size_all) {
        if (plan.cum_owner(c) != (int)R || split(c) || clog[c] <= SMALL_COMPONENT_MAX_LOG) continue;   // (split: generated above, by rows)
        launch_logup(c, (const uint32_t* const*)tr_evals.dev(ltr0[c]), (const uint32_t* const*)pp_evals.dev(), clog[c], drel.as<DevRelations>(),
                     it_evals.dev(lit0[c]), fk.stream(small_jobs.empty() && spos == 0 ? Fork::MAIN : 1 + spos % 2));
        spos++;
      }
      fk.join();
    }
  }
  // ---- the claimed sums: every rank's own sums + {lookup flag, FRI plan} -> all ranks.  tree_stream: nothing waits here — the
  // words travel on the stream (device all-gather with a stream-ordered comm) into pinned memory behind an event, and the host
  // picks them up in `sums_arrive` AFTER tree 2's transforms have been enqueued (they do not depend on the sums; the device step
  // behind tree 2 does: it starts from the channel state with the sums mixed in) ----
  // (round 6) "logup_defer", as in the single-GPU prover's interaction(): the LogUp tail — claimed sums, the running-sum columns'
  // prefix scans: ~0.15 ms of short memory-bound kernels — and the sums' gather run on a SIDE stream while tree 2's transforms of
  // every other column start on the main one; the running-sum columns go last in their size group (Prover::DeferredCols).
  // The tail's stream `sf` is the main stream or — defer_tail — side stream 1; the collective follows it there through set_stream,
  // so the deferred form is taken only when the communicator can follow (a stream-ordered one without set_stream stays on `st`).
  void claimed_sums_exchange(const std::vector<LogupTailJob>& jobs) {
    const bool defer_tail = tree_stream && tune(T_LOGUP_DEFER) != 0 && (!cm.ordered() || comm_c.set_stream);
    hipStream_t sf = st;
    if (defer_tail) {
      sf = thread_side_stream(1);
      hipEvent_t e = Prover::pipe_event();
      CM_HIP(hipEventRecord(e, st));
      CM_HIP(hipStreamWaitEvent(sf, e, 0));
      late_cols.late.assign(lit_logs.size(), 0);
      for (int c : my_comps)
        for (int q = 0; q < 4; q++) late_cols.late[lit_of[it0[c] + air::component_info(c).n_interaction - 4 + q]] = 1;
    }
    if (!jobs.empty()) {
      d_sums.alloc(jobs.size() * 16);
      logup_finalize_all(jobs, d_sums.u32(), sf, defer_tail ? &tail_scratch : nullptr);
    }
    static_assert(PIN_SUMS + air::N_COMPONENTS * 4 <= PIN_COEFF, "pinned slot layout");
    if (tree_stream && cm.ordered()) {   // (a lone rank too: the one-GPU tests and the bench then run the path a multi-GPU node takes)
      // compact layout per rank: its k-th sum belongs to the k-th component whose cumulative-sum columns it owns; then flag, plan
      cm.need(SW * N);
      if (!jobs.empty()) CM_HIP(hipMemcpyAsync(comm_c.send_buf, d_sums.p, jobs.size() * 16, hipMemcpyDeviceToDevice, sf));
      CM_HIP(hipMemcpyAsync(comm_c.send_buf + SW - 2, flag.p, 4, hipMemcpyDeviceToDevice, sf));
      const uint32_t stop_w = shard_fri_stop_log();
      stage_upload(comm_c.send_buf + SW - 1, &stop_w, 4, sf);
      // (the collective follows the tail onto its stream; nothing else touches the staging buffers until the host has the sums)
      if (sf != st && comm_c.set_stream) comm_c.set_stream(comm_c.ctx, (cm_stream_t)(uintptr_t)sf);
      cm.all_gather(SW);
      if (sf != st && comm_c.set_stream) comm_c.set_stream(comm_c.ctx, (cm_stream_t)(uintptr_t)st);
      // (dedicated pinned words: every other fixed slot ends at PIN_LAST_LAYER_END, and the landing buffer is elsewhere)
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_SHARD_SUMS, comm_c.recv_buf, SW * N * 4, hipMemcpyDeviceToHost, sf));
      sums_land = pinned_words() + PIN_SHARD_SUMS;
      sums_gathered = true;
    } else if (!jobs.empty()) {
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_SUMS, d_sums.p, jobs.size() * 16, hipMemcpyDeviceToHost, sf));
      sums_land = pinned_words() + PIN_SUMS;
    }
    static thread_local hipEvent_t ev = nullptr;
    CM_HIP(hipEventRecord(ev_sums = thread_event(ev), sf));
    if (defer_tail) late_cols.ready = ev;
  }
  void sums_arrive() {
    CM_HIP(hipEventSynchronize(ev_sums));
    d_sums.release();
    tail_scratch.clear();
    if (tree_stream) {
      // host replay of the device-side step behind tree 1 (its results were copied back in front of the sums)
      const uint32_t* s1 = pinned_words() + PIN_STEP1;
      complete_sliced(cm, sl1, pin_sub1);
      CM_CHECK(memcmp(sl1.root.data(), s1, 32) == 0, "sharded trace commitment: the device's tree top differs from the host's");
      ch.mix_root(sl1.root);
      pf.interaction_pow = (uint64_t)s1[8] | ((uint64_t)s1[9] << 32);
      {
        Channel probe = ch;   // the nonce must satisfy the proof-of-work predicate on the HOST channel
        probe.mix_u64(pf.interaction_pow);
        CM_CHECK(s1[11] == 0 && probe.trailing_zeros() >= INTERACTION_POW_BITS, "interaction proof of work: device step diverged from the host channel");
      }
      ch.mix_u64(pf.interaction_pow);
      DevRelations drel_h;
      draw_relations(ch, hrel, drel_h);
      CM_CHECK(ch.n_sent == s1[10] && memcmp(drel_h.z[0], s1 + 12, 16) == 0, "relations: device transcript diverged from the host channel");
    }
    std::vector<uint32_t> all;
    if (sums_gathered) {
      all.assign(SW * N, 0);
      for (uint32_t r = 0; r < N; r++) {
        size_t k = 0;
        for (int c = 0; c < air::N_COMPONENTS; c++)
          if (plan.cum_owner(c) == (int)r) { memcpy(&all[r * SW + 4 * c], &sums_land[r * SW + 4 * k], 16); k++; }
        all[r * SW + SW - 2] = sums_land[r * SW + SW - 2];
        all[r * SW + SW - 1] = sums_land[r * SW + SW - 1];
      }
    } else {
      std::vector<uint32_t> sums_mine(SW, 0);
      for (size_t k = 0; k < my_comps.size(); k++) memcpy(&sums_mine[4 * my_comps[k]], &sums_land[4 * k], 16);
      sums_mine[SW - 2] = pinned_words()[PIN_FLAG];
      sums_mine[SW - 1] = shard_fri_stop_log();
      all = cm.gather_host(sums_mine);
    }
    if (tree_stream) check_flags(all, SW, SW - 2);
    for (int c = 0; c < air::N_COMPONENTS; c++) pf.claimed_sums.push_back(QM31::from_u32(&all[(size_t)plan.cum_owner(c) * SW + 4 * c]));
    for (auto& cs : pf.claimed_sums) ch.mix_felts(&cs, 1);
  }
  void check_halo(bool synchronise = true) {   // (false: the caller has waited for an event behind the error word's copy)
    if (!halo_pending) return;
    if (synchronise) CM_HIP(hipStreamSynchronize(st));
    halo_pending = false;
    CM_CHECK(*pin_halo_err == 0, "sharded constraints: a previous-row neighbour lies outside the two ranges the halo exchange covers");
  }
  // The constraints of a split component are evaluated by row range (below), but its cumulative-sum columns are also read at
  // the PREVIOUS row of the trace domain, which lies in some other rank's range: every rank gets those four LDE columns whole.
  // (round 6) "shard_halo" = 1: a HALO instead — on bit-reversed storage the previous row of every EVEN local position of a range
  // lies in the range whose bit-reversed rank number is one lower (first half of the domain: natural index i - 1) and of every
  // ODD position in the range one higher (second half: i + 1); so every rank sends the even half of its slices to one neighbour and
  // the odd half to the other (one all_to_all_v with two non-empty destinations: 1 / N of the all-gather's bytes per rank) and
  // builds `cum_prev[q]` = the column at the previous row of its q-th row (k_halo_build).  0 = the round-4 all-gather.
  void cum_columns_exchange() {
    const bool halo = tune(T_SHARD_HALO) != 0 && N >= 2;
    if (halo) {
      auto brev = [&](uint32_t x) { return bit_reverse(x, logN); };
      const uint32_t rho = brev(R);
      const uint32_t src_even = brev((rho + N - 1) % N), src_odd = brev((rho + 1) % N);   // whose halves this rank reads
      const uint32_t dst_even = brev((rho + 1) % N), dst_odd = brev((rho + N - 1) % N);   // who reads this rank's even / odd halves
      uint64_t half_words = 0;   // one half of every cumulative-sum slice of every split component
      for (auto& sc : splits) half_words += (uint64_t)4 << sc->slog;
      std::vector<uint64_t> send_words(N, 0), recv_words(N, 0);
      send_words[dst_even] += half_words; send_words[dst_odd] += half_words;
      recv_words[src_even] += half_words; recv_words[src_odd] += half_words;
      cm.need(2 * half_words);
      // send_buf is destination-major in rank order; with N = 2 both halves go to the one other rank: even first, then odd
      std::vector<uint64_t> send_off(N, 0), recv_off(N, 0);
      { uint64_t o = 0; for (uint32_t d = 0; d < N; d++) { send_off[d] = o; o += send_words[d]; } }
      { uint64_t o = 0; for (uint32_t d = 0; d < N; d++) { recv_off[d] = o; o += recv_words[d]; } }
      uint64_t oe = send_off[dst_even], oo = send_off[dst_odd] + (dst_odd == dst_even ? half_words : 0);
      for (auto& sc : splits) {
        const uint32_t hl = 1u << sc->slog;   // half of a slice of 2^(slog + 1) rows
        const size_t j0 = it0[sc->c] + air::component_info(sc->c).n_interaction - 4;
        for (int q = 0; q < 4; q++) {
          pack_parity(sl2.slice[j0 + q], comm_c.send_buf + oe, hl, 0u, st); oe += hl;
          pack_parity(sl2.slice[j0 + q], comm_c.send_buf + oo, hl, 1u, st); oo += hl;
        }
      }
      cm.all_to_all_v(send_words, recv_words);
      DevBuf d_err(4);
      CM_HIP(hipMemsetAsync(d_err.p, 0, 4, st));
      uint64_t re = recv_off[src_even], ro = recv_off[src_odd] + (src_odd == src_even ? half_words : 0);
      for (auto& sc : splits) {
        const uint32_t n = clog[sc->c] + 1, len = 1u << (sc->slog + 1), hl = 1u << sc->slog;
        sc->cum_prev.alloc(std::vector<uint32_t>(4, sc->slog + 1), st);
        for (int q = 0; q < 4; q++) {
          halo_build(comm_c.recv_buf + re, comm_c.recv_buf + ro, src_even, src_odd, R * len, len, n, clog[sc->c], logN, sc->cum_prev.ptrs[q], d_err.u32(), st);
          re += hl; ro += hl;
        }
      }
      CM_HIP(hipMemcpyAsync(pin_halo_err, d_err.p, 4, hipMemcpyDeviceToHost, st));
      halo_pending = true;
      if (!tree_stream) check_halo();   // (tree_stream: at the next synchronisation point — the kernels that read recv_buf are on the stream)
    } else {
      uint64_t words = 0;
      for (auto& sc : splits) words += (uint64_t)4 << (sc->slog + 1);
      cm.need(words * N);
      std::vector<CopySeg> segs;
      uint64_t off = 0;
      for (auto& sc : splits) {
        const uint64_t sl = (uint64_t)1 << (sc->slog + 1);
        const size_t j0 = it0[sc->c] + air::component_info(sc->c).n_interaction - 4;
        for (int q = 0; q < 4; q++) { segs.push_back(CopySeg{sl2.slice[j0 + q], comm_c.send_buf + off, sl}); off += sl; }
      }
      copy_segments(segs, st);
      cm.all_gather(words);
      segs.clear();
      for (auto& sc : splits) sc->cum_lde.alloc(std::vector<uint32_t>(4, clog[sc->c] + 1), st);
      for (uint32_t src = 0; src < N; src++) {
        off = (uint64_t)src * words;
        for (auto& sc : splits) {
          const uint64_t sl = (uint64_t)1 << (sc->slog + 1);
          for (int q = 0; q < 4; q++) { segs.push_back(CopySeg{comm_c.recv_buf + off, sc->cum_lde.ptrs[q] + (uint64_t)src * sl, sl}); off += sl; }
        }
      }
      copy_segments(segs, st);
    }
  }
  // tree 2: LogUp columns, claimed sums (tree_stream: waited for behind tree 2's transforms), the split components' previous rows
  void interaction() {
    it_evals.alloc(lit_logs, st);
    {
      std::vector<LogupTailJob> jobs;
      DevBuf d_small;   // the small components' job table: goes back to the pool behind the sums' exchange, as ever
      logup_launches(jobs, d_small);
      claimed_sums_exchange(jobs);
    }
    if (!tree_stream) sums_arrive();
    P.tick("interaction_gen");
    const size_t total_constraints = powers.size();
    d_powers.alloc(16 * total_constraints);
    {
      own2.coeffs = std::move(it_evals);   // interpolated in place, every size group right in front of its extension
      commit_own(own2, nullptr, true, /*evals_in_place=*/true, it_logs, it_owner, sl2, tree_stream ? std::function<void()>([this] { sums_arrive(); }) : nullptr,
                 late_cols.ready ? &late_cols : nullptr);
      if (tree_stream) {
        // root 2 -> random coefficient -> its powers, behind the all-gather (prover.hip composition): the constraint kernels start
        // without the host having seen the root
        shard_top(comm_c.recv_buf, N, ts + TS_ROOT2, ts + TS_SUB2, st);
        uint32_t cw[9];
        channel_words(ch, cw);
        chan_init_mix_root_draw(cw, ts + TS_CHAN, ts + TS_ROOT2, ts + TS_COEFF, ts + TS_ROOT2_LOG, st);
        coeff_powers(ts + TS_COEFF, d_powers.u32(), (uint32_t)total_constraints, st);
        static_assert(PIN_COEFF + 4 == PIN_ROOT2 && TS_COEFF + 4 == TS_ROOT2_LOG, "{coefficient, root 2} come back in one copy");
        CM_HIP(hipMemcpyAsync(pin_sub2, ts + TS_SUB2, 8 * N * 4, hipMemcpyDeviceToHost, st));
        CM_HIP(hipMemcpyAsync(pinned_words() + PIN_COEFF, ts + TS_COEFF, 48, hipMemcpyDeviceToHost, st));
      }
    }
    tr_evals.buf.release();
    for (auto& sc : splits) { sc->tr_slice.buf.release(); sc->it_slice.buf.release(); }
    if (!splits.empty()) cum_columns_exchange();
    if (!tree_stream) ch.mix_root(sl2.root);
    P.tick("interaction_commit");
    for (auto l : P.trees[0].coeffs.logs) pf.cells += 1ull << l;
    for (auto l : tr_logs) pf.cells += 1ull << l;
    for (auto l : it_logs) pf.cells += 1ull << l;
  }
  // constraints of the own components -> acc_top: the composition polynomial's coefficients, partial sums reduced across the ranks
  void constraint_quotients(ColumnSet& acc_top) {
    std::vector<DevBuf> split_tabs;   // column tables of the split components (alive until the launches are enqueued and drained)
    // B > 1: the own polynomials of trees 0..2 on their (log + 1) evaluation domains
    ColumnSet cdom[3];
    if (B > 1) {
      const ColumnSet* const src[3] = {&P.trees[0].coeffs, &own1.coeffs, &own2.coeffs};
      eval_domain_copies(cdom, src, *P.tw, st);
    }
    // the accumulators of every evaluation log with own components (constraint_plan.hpp); split components: every rank, its rows
    ConstraintAccumulators acc;
    acc.plan(clog, comp_log, [this](int c) { return mine(c) || split(c); });
    acc.alloc(st, /*upload_ptrs=*/true, /*top_contiguous: exchanged as one block*/ true);
    const std::map<uint32_t, std::vector<int>>& cgroups = acc.cgroups;
    // small components (idle ones are 16 padding rows: pure launch latency): private accumulator slots, ONE batched launch,
    // slots summed afterwards — as in the single-GPU prover
    std::vector<ConstraintArgs> small_args;
    std::vector<int> small_cids;
    struct SlotGroup { uint32_t el, n; size_t off_words; };
    std::vector<SlotGroup> sgroups;
    std::map<int, size_t> slot_off;     // component -> word offset of its 4-column slot
    size_t slot_words = 0;
    uint32_t small_max_log = 0;
    for (auto& kv : cgroups) {
      SlotGroup g{kv.first, 0, slot_words};
      for (int c : kv.second)
        if (clog[c] <= SMALL_COMPONENT_MAX_LOG) { slot_off[c] = slot_words; slot_words += (size_t)4 << kv.first; g.n++; }
      if (g.n) sgroups.push_back(g);
    }
    DevBuf slots(((slot_words * 4 + 15) & ~(size_t)15) + 16);
    std::vector<uint32_t*> slot_tab;
    acc.zero(slots.p, slot_words, st);
    std::map<int, size_t> slot_tab_at;
    for (auto& kv : slot_off) {
      slot_tab_at[kv.first] = slot_tab.size();
      for (int k = 0; k < 4; k++) slot_tab.push_back(slots.u32() + kv.second + ((size_t)k << (clog[kv.first] + 1)));
    }
    DevBuf d_slot_tab = upload(slot_tab, st);
    std::vector<std::pair<int, ConstraintArgs>> big_jobs;   // (component, arguments) in launch order: descending size
    for (auto it = cgroups.rbegin(); it != cgroups.rend(); ++it)
      for (int c : it->second) {
        const air::ComponentInfo& info = air::component_info(c);
        ConstraintArgs a;
        if (split(c)) {
          // this rank's rows of the evaluation domain: the column tables point row0 words in front of the slices the LDE exchange
          // left here (the kernel indexes by the global row); the cumulative-sum columns are whole
          const uint32_t esl = clog[c] + 1 - logN;
          a.row0 = R << esl;
          a.n_rows = 1u << esl;
          std::vector<const uint32_t*> tab;
          for (int k = 0; k < info.n_trace; k++) tab.push_back((const uint32_t*)((uintptr_t)sl1.slice[tr0[c] + k] - (uintptr_t)4 * a.row0));
          const SplitComp* sc = nullptr;
          for (auto& x : splits) if (x->c == c) sc = x.get();
          const bool with_halo = sc->cum_prev.ptrs.size() == 4;   // (shard_halo: the cumulative-sum columns stay slices too)
          for (int k = 0; k < info.n_interaction; k++)
            tab.push_back(k + 4 < info.n_interaction || with_halo ? (const uint32_t*)((uintptr_t)sl2.slice[it0[c] + k] - (uintptr_t)4 * a.row0)
                                                                   : (const uint32_t*)sc->cum_lde.ptrs[k - (info.n_interaction - 4)]);
          if (with_halo) for (int k = 0; k < 4; k++) tab.push_back((const uint32_t*)((uintptr_t)sc->cum_prev.ptrs[k] - (uintptr_t)4 * a.row0));
          split_tabs.push_back(upload(tab, st));
          a.tr = split_tabs.back().as<const uint32_t*>();
          a.it = a.tr + info.n_trace;
          if (with_halo) a.it_prev = a.it + info.n_interaction;
        } else {
          a.tr = (const uint32_t* const*)(B > 1 ? cdom[1].dev(ltr0[c]) : own1.lde.dev(ltr0[c]));
          a.it = (const uint32_t* const*)(B > 1 ? cdom[2].dev(lit0[c]) : own2.lde.dev(lit0[c]));
        }
        a.pp = (const uint32_t* const*)(B > 1 ? cdom[0].dev() : P.trees[0].lde.dev());
        const bool small = slot_off.count(c) != 0;
        a.acc = small ? d_slot_tab.as<uint32_t*>() + slot_tab_at[c] : acc.of(it->first);
        fill_constraint_args(a, c, clog[c], pf.claimed_sums[c], drel.as<DevRelations>(), d_powers.u32() + 4 * coff[c]);
        if (small) { small_args.push_back(a); small_cids.push_back(c); small_max_log = std::max(small_max_log, clog[c]); }
        else big_jobs.push_back({c, a});
      }
    DevBuf d_small_args = upload(small_args, st), d_small_cids = upload(small_cids, st);
    {
      // (round 6) one fork region like the single-GPU prover's (prover.hip composition): the batched small components first on a side
      // stream (latency-bound, hidden under the large kernels), a WIDE component of few rows (poseidon2: one long program per row on
      // four blocks, ~0.3 ms of pure latency) next, then every size group on a stream of its own (the components of a group share its
      // accumulator and stay in order); the largest group on the main stream.  A group whose components all ran on its stream has its
      // accumulator interpolated right there (DomainEvaluationAccumulator::finalize starts inside the region).  Everything used to run
      // on the main stream, one kernel after the other (constraints 1.30 against 0.88 ms on one rank).
      Fork fk(st);
      if (!small_args.empty())
        launch_constraints_small(d_small_args.as<ConstraintArgs>(), d_small_cids.as<int>(), (uint32_t)small_args.size(), small_max_log, fk.stream(7));
      std::map<uint32_t, int, std::greater<uint32_t>> group_stream;   // evaluation log (descending) -> stream index
      for (auto& j : big_jobs) {
        const uint32_t el = clog[j.first] + 1;
        if (!group_stream.count(el)) { const int gi = (int)group_stream.size(); group_stream[el] = gi == 0 ? Fork::MAIN : gi % 4; }
      }
      auto is_wide = [&](int c) { return is_wide_component(c, clog); };
      for (auto& j : big_jobs) if (is_wide(j.first)) launch_constraints(j.first, j.second, fk.stream(group_stream.at(clog[j.first] + 1)));
      for (auto& gs_ : group_stream) {
        const uint32_t el = gs_.first;
        for (auto& j : big_jobs) if (clog[j.first] + 1 == el && !is_wide(j.first)) launch_constraints(j.first, j.second, fk.stream(gs_.second));
        bool has_small = false;
        for (auto& g : sgroups) has_small = has_small || g.el == el;
        if (!has_small) {
          interpolate(acc.of(el), 4, el, *P.tw, fk.stream(gs_.second));
          acc.interpolated.insert(el);
        }
      }
      fk.join();
    }
    if (!small_args.empty()) {
      for (auto& g : sgroups) sum_slots(acc.of(g.el), slots.u32() + g.off_words, g.n, g.el, st);
    }
    P.tick("constraints");
    // interpolate every partial accumulator at its own size and add the zero-padded coefficient vectors (linear: the
    // partial sums of all ranks add up to the coefficients the single-GPU prover computes); ONE launch adds all of them
    finalize_accumulators(acc, *P.tw, st);
    // reduce across ranks: slices of the (4 x 2^comp_log)-word buffer go to their owner, are summed mod P, and come back
    if (N > 1) {   // (a lone rank's coefficients are the sum: two 64 MB copies and two collectives less)
      const uint64_t W = (uint64_t)4 << comp_log, sl = W / N;
      cm.need(W);
      CM_HIP(hipMemcpyAsync(comm_c.send_buf, acc.top.buf.p, W * 4, hipMemcpyDeviceToDevice, st));
      cm.all_to_all_v(std::vector<uint64_t>(N, sl), std::vector<uint64_t>(N, sl));
      sum_copies(comm_c.recv_buf, N, sl, sl, comm_c.send_buf, true, st);
      cm.all_gather(sl);
      CM_HIP(hipMemcpyAsync(acc.top.buf.p, comm_c.recv_buf, W * 4, hipMemcpyDeviceToDevice, st));
    }
    acc_top = std::move(acc.top);
  }
  // composition polynomial + tree 3 (prover.rs:114-120)
  void composition() {
    if (!tree_stream) draw_constraint_powers(ch, powers, d_powers, st);
    ColumnSet acc_top;
    constraint_quotients(acc_top);
    {
      CommittedTree& t = P.trees[3];
      t.coeffs = std::move(acc_top);
      P.commit_enqueue(t, nullptr, true, st, /*with_merkle=*/false);   // LDE of the 4 coordinate columns on every rank (0.15 ms) ...
      slice_replicated(cm, t.lde, sl3, nullptr, /*enqueue_only=*/tree_stream);   // ... Merkle hashing by row range
      if (tree_stream) {
        // root 3 -> the felt of the OODS point, on the device copy of the channel the coefficient step left (prover.hip oods_sampling)
        shard_top(comm_c.recv_buf, N, ts + TS_ROOT3, ts + TS_SUB3, st);
        chan_mix_root_draw(ts + TS_CHAN, ts + TS_ROOT3, ts + TS_STEP3, ts + TS_STEP3 + 4, st);
        CM_HIP(hipMemcpyAsync(pin_sub3, ts + TS_SUB3, 8 * N * 4, hipMemcpyDeviceToHost, st));
        CM_HIP(hipMemcpyAsync(pinned_words() + PIN_STEP3, ts + TS_STEP3, 48, hipMemcpyDeviceToHost, st));   // {felt[4], root 3 [8]}
        static thread_local hipEvent_t ev = nullptr;   // root 3 comes back HERE, in front of the evaluation kernels enqueued next
        CM_HIP(hipEventRecord(ev_root3 = thread_event(ev), st));
      } else {
        t.root = sl3.root;
        ch.mix_root(sl3.root);
      }
    }
    P.tick("composition_commit");
  }
  // OODS sampling: own columns (+ trees 0 and 3 on every rank), values all-gathered; the DEEP-quotient plan is made meanwhile
  void oods_sampling() {
    if (!tree_stream) oods = draw_oods_point(ch);
    // global sample slots: (tree, column, prev?) -> slot; owner of every slot
    struct Slot { int t; uint32_t c; bool prev; int owner; const uint32_t* coeffs; uint32_t log; };
    std::vector<Slot> slots;
    std::vector<std::vector<uint32_t>> sidx_cur(4), sidx_prev(4);
    n_cols_t[0] = P.trees[0].coeffs.size(); n_cols_t[1] = tr_logs.size(); n_cols_t[2] = it_logs.size(); n_cols_t[3] = 4;
    for (int t = 0; t < 4; t++) { sidx_cur[t].assign(n_cols_t[t], 0); sidx_prev[t].assign(n_cols_t[t], 0); }
    // where this rank holds the coefficients of every column it samples (trees 0 / 3: every rank; trees 1 / 2: the owner)
    std::vector<std::vector<const uint32_t*>> cptr(4);
    for (int t = 0; t < 4; t++) {
      cptr[t].resize(n_cols_t[t]);
      if (t == 0 || t == 3) { for (size_t c = 0; c < n_cols_t[t]; c++) cptr[t][c] = P.trees[t].coeffs.ptrs[c]; continue; }
      const std::vector<int>& ow = t == 1 ? tr_owner : it_owner;
      size_t li = 0;
      for (size_t c = 0; c < n_cols_t[t]; c++) cptr[t][c] = (uint32_t)ow[c] == R ? (t == 1 ? own1 : own2).coeffs.ptrs[li++] : nullptr;
    }
    for (int t = 0; t < 4; t++)
      for (uint32_t c = 0; c < n_cols_t[t]; c++) {
        sidx_cur[t][c] = (uint32_t)slots.size();
        slots.push_back(Slot{t, c, false, col_owner_of(t, c), cptr[t][c], col_log(t, c)});
      }
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      int ni = air::component_info(c).n_interaction;
      for (int k = ni - 4; k < ni; k++) {
        const uint32_t gc = (uint32_t)(it0[c] + k);
        sidx_prev[2][gc] = (uint32_t)slots.size();
        slots.push_back(Slot{2, gc, true, it_owner[gc], cptr[2][gc], clog[c]});
      }
    }
    const size_t n_slots = slots.size();
    d_oods_out.alloc(n_slots * 16);
    std::map<uint32_t, CPoint<QM31>> prev_points;
    std::vector<uint32_t> samples(4 * n_slots, 0);
    // (d_oods_out: every slot is written by the upload of the gathered samples below)
    // jobs = (log, prev?) groups of the slots this rank evaluates (trees 0 / 3: every rank, so that nobody waits for them)
    std::map<std::pair<uint32_t, bool>, std::vector<uint32_t>> groups;
    for (uint32_t s = 0; s < n_slots; s++)
      if (slots[s].coeffs) groups[{slots[s].log, slots[s].prev}].push_back(s);
    std::vector<const uint32_t*> table;
    struct J { uint32_t log; bool prev; size_t off, n; std::vector<uint32_t> ids; };
    std::vector<J> js;
    for (auto& kv : groups) {
      J j{kv.first.first, kv.first.second, table.size(), kv.second.size(), kv.second};
      for (auto s : kv.second) table.push_back(slots[s].coeffs);
      js.push_back(j);
    }
    DevBuf &d_table = d_oods_table = upload(table, st), &d_tmp = d_oods_tmp;
    size_t n_tmp = table.size();
    d_tmp.alloc(n_tmp * 16 + 16);
    std::vector<EapJob> ej;
    for (auto& j : js) {
      CPoint<QM31> pt = oods;
      EapJob e{j.log, (uint32_t)j.n, d_table.as<const uint32_t*>() + j.off, QM31(), QM31(), d_tmp.u32() + 4 * j.off};
      if (j.prev) {
        CPoint<M31> step = point_at_index(subgroup_gen_index(j.log));
        if (tree_stream) { e.has_shift = true; e.shift_x = step.x.v; e.shift_y = (-step.y).v; }
        else pt = cadd(oods, CPoint<QM31>{QM31(step.x), QM31(-step.y)});
      }
      e.px = pt.x; e.py = pt.y;
      ej.push_back(e);
    }
    eval_at_point_multi(ej, st, tree_stream ? ts + TS_STEP3 : nullptr);
    std::vector<uint32_t> tmp(4 * n_tmp);
    const void* tmp_land = n_tmp ? stage_download_async(d_tmp.p, tmp.size() * 4, st) : nullptr;   // pinned: read after the synchronisation below
    if (tree_stream) {
      // host replay of the steps behind trees 2 and 3, in transcript order, as soon as root 3 is back — the evaluation kernels are
      // still running (the one round trip since the claimed sums)
      CM_HIP(hipEventSynchronize(ev_root3));
      check_halo(/*synchronise=*/false);
      complete_sliced(cm, sl2, pin_sub2);
      CM_CHECK(memcmp(sl2.root.data(), pinned_words() + PIN_ROOT2, 32) == 0, "sharded interaction commitment: the device's tree top differs from the host's");
      ch.mix_root(sl2.root);
      const QM31 rho = ch.draw_felt();
      CM_CHECK(rho == QM31::from_u32(pinned_words() + PIN_COEFF), "composition: device transcript diverged from the host channel");
      QM31 pw(M31(1));
      for (size_t g = powers.size(); g-- > 0;) { powers[g] = pw; pw = pw * rho; }   // host copy: the OODS check needs it
      complete_sliced(cm, sl3, pin_sub3);
      CM_CHECK(memcmp(sl3.root.data(), pinned_words() + PIN_STEP3 + 4, 32) == 0, "sharded composition commitment: the device's tree top differs from the host's");
      P.trees[3].root = sl3.root;
      ch.mix_root(sl3.root);
      QM31 t;
      oods = draw_oods_point(ch, &t);
      CM_CHECK(t == QM31::from_u32(pinned_words() + PIN_STEP3), "oods: device transcript diverged from the host channel");
    }
    for (int c = 0; c < air::N_COMPONENTS; c++) {
      CPoint<M31> step = point_at_index(subgroup_gen_index(clog[c]));
      prev_points[clog[c]] = cadd(oods, CPoint<QM31>{QM31(step.x), QM31(-step.y)});
    }
    // mask sizes now ([oods] or [previous row, oods]), values below: the quotient tables are built while the evaluation kernels run
    pf.sampled_values.resize(4);
    for (int t = 0; t < 4; t++) {
      pf.sampled_values[t].resize(n_cols_t[t]);
      for (uint32_t c = 0; c < n_cols_t[t]; c++)
        for (int k = (t == 2 && sidx_prev[2][c] != 0 ? 2 : 1); k > 0; k--) pf.sampled_values[t][c].push_back(QM31());
    }
    plan_deep_quotients(sidx_cur, sidx_prev, prev_points);
    // ---- the sampled values: wait, gather, mix ----
    {
      CM_HIP(hipStreamSynchronize(st));
      if (n_tmp) memcpy(tmp.data(), tmp_land, tmp.size() * 4);
      std::vector<uint32_t> mine_s(4 * n_slots, 0);
      for (auto& j : js)
        for (size_t i = 0; i < j.n; i++) memcpy(&mine_s[4 * j.ids[i]], &tmp[4 * (j.off + i)], 16);
      std::vector<uint32_t> all = cm.gather_host(mine_s);
      for (size_t s = 0; s < n_slots; s++) memcpy(&samples[4 * s], &all[(size_t)slots[s].owner * 4 * n_slots + 4 * s], 16);
      stage_upload(d_oods_out.p, samples.data(), samples.size() * 4, st);
    }
    for (int t = 0; t < 4; t++)
      for (uint32_t c = 0; c < n_cols_t[t]; c++) {
        const bool has_prev = t == 2 && sidx_prev[2][c] != 0;
        if (has_prev) pf.sampled_values[t][c][0] = QM31::from_u32(&samples[4 * sidx_prev[2][c]]);
        pf.sampled_values[t][c][has_prev ? 1 : 0] = QM31::from_u32(&samples[4 * sidx_cur[t][c]]);
      }
    {
      std::vector<QM31> flat;
      for (auto& t : pf.sampled_values) for (auto& c : t) for (auto& sm : c) flat.push_back(sm);
      ch.mix_felts(flat.data(), flat.size());
    }
    P.tick("oods_sampling");
  }
  // DEEP quotients of the own ROWS, host half (quotient_plan.hpp; no sampled value needed yet): plan, upload, launch arguments
  void plan_deep_quotients(const std::vector<std::vector<uint32_t>>& sidx_cur, const std::vector<std::vector<uint32_t>>& sidx_prev,
                           const std::map<uint32_t, CPoint<QM31>>& prev_points) {
    std::vector<QuotientCol> qcols;
    for (int t = 0; t < 4; t++)
      for (uint32_t c = 0; c < n_cols_t[t]; c++) {
        const uint32_t lde_log = col_log(t, c) + B;
        const uint64_t sl = (uint64_t)1 << (lde_log - logN);
        qcols.push_back({t, c, lde_log, /* this rank's row slice */ t == 0 || t == 3 ? P.trees[t].lde.ptrs[c] + (uint64_t)R * sl : t == 1 ? sl1.slice[c] : sl2.slice[c]});
      }
    QuotientPlan qp; const QuotientWindow win{(int)logN, R};   // this rank's rows
    qp.build(qcols, pf.sampled_values, sidx_cur, sidx_prev, oods, prev_points, B, win, st);
    d_qblob.alloc(qp.blob.size());
    qp.bind(d_qblob.as<uint8_t>());
    stage_upload(d_qblob.p, qp.blob.data(), qp.blob.size(), st);   // (behind the evaluation kernels, in front of the wait)
    o_qjobs = qp.o_jobs; n_qjobs = qp.n_jobs; gs = std::move(qp.groups);
    qargs = quotient_args(gs, d_qblob.as<uint8_t>(), *P.tw, win);
    // "quot_leaf": the first-layer FRI subtree's leaf layer is written by the LARGEST group's quotient kernel (prover.hip deep_quotients)
    if (shard_fri_stop_log() < 99 && quotient_leaf_wanted(qargs)) {
      fri_first.local.leaf_prealloc.alloc((size_t)32 * qargs[0].first.n_rows);
      qargs[0].first.leaf_hashes = fri_first.local.leaf_prealloc.u32();
      fri_first.leaf_done = true;
    }
  }
  // compute_fri_quotients: one launch per size group
  void deep_quotients() {
    const QM31 qcoeff = ch.draw_felt();
    quotient_coeffs((const QuotientCoefJob*)(d_qblob.as<uint8_t>() + o_qjobs), (uint32_t)n_qjobs, d_oods_out.u32(), qcoeff, st);
    {
      // one kernel per size group, independent outputs: the small groups (latency-bound) together on one side stream first, the
      // large ones by descending size on streams of their own (the single-GPU prover's region)
      Fork fkq(st);
      int qk = 0;
      for (auto& qa : qargs) if (qa.first.log_size < 14) launch_quotients(qa.first, qa.second, fkq.stream(Fork::N - 1));
      for (auto& qa : qargs)
        if (qa.first.log_size >= 14) { launch_quotients(qa.first, qa.second, fkq.stream(qk == 0 ? Fork::main_or(0) : qk % (Fork::N - 1))); qk++; }
      fkq.join();
    }
    for (auto& g : gs) q_logs.push_back(g.log);
    d_qblob.release(); qargs.clear();   // (where d_blob's block ended: pool blocks are reused in stream order, no host synchronisation)
    P.tick("quotients");
  }
  // ---- FRI commit.  Folds are pair-local (rows 2i, 2i + 1 of a layer give row i of the next), so a rank that holds rows
  // [r, r+1) * 2^l / N of a layer produces the same range of the next one with no exchange; a layer's tree is the rank's subtree +
  // a 32-byte all-gather + the top log2 N levels (SlicedTree, like the four commitment trees).  The first-layer tree (over the
  // quotient slices) and every inner layer above 2^stop rows are committed that way, with the transcript on the host channel;
  // then the current layer and the small quotient groups are all-gathered and FriPhase::commit finishes on every rank (device-side
  // transcript, k_fri_tail) — the replicated part is the latency-bound tail only. ----
  void fri_and_pow() {
    last_log = cfg.log_last_layer_degree_bound + cfg.log_blowup_factor;
    layer_log = q_logs[0] - 1;
    shard_fri = shard_fri_stop_log() < 99;
    // (round 6) "shard_fri_stream": the sharded layers stay ON THE STREAM — after a tree's 32-byte all-gather ONE kernel hashes the
    // top log2 N levels over the N sub-roots, mixes the root into a device copy of the channel and draws the folding challenge
    // (k_shard_top_step); the fold kernels read the challenge from device memory.  The host replays every step (top levels for the
    // decommitment, mix_root, draw_felt) ONCE behind the last sharded layer and refuses the proof on a mismatch, instead of
    // stopping the stream for a root and a challenge after every tree (7 round trips at the metric config).  With a host-blocking
    // cm_comm the collective itself still waits; with the stream-ordered RCCL communicator nothing does.  0 = the host-driven form.
    fri_stream = shard_fri && tune(T_SHARD_FRI_STREAM) != 0 && !framing().hash_node_rfc;
    if (shard_fri) fri_sharded_layers();
    fri_hand_over();
    {
      FriResume rs;
      rs.layer = cur_valid ? &full_layer : nullptr;
      rs.layer_log = layer_log;
      rs.qi = qi_next;
      rs.n_inner_before = (uint32_t)sfl.size();
      rs.alpha_c = alpha_c;
      rs.d_chan = rs_d_chan;
      rs.d_alpha_c = rs_d_alpha_c;
      fri.commit(P, cfg, quotients, q_logs, pf, [&] {
        fri_replay();   // (fri_stream) the sharded layers' steps, in front of FriPhase's own replay
        check_composition_at_oods(pf, tr0, it0, clog, hrel, powers, coff, oods);
      }, shard_fri ? &rs : nullptr);
    }
    hm.mark("fri_commit returned");
    P.tick("fri_commit");
    pf.proof_of_work = grind_gpu(ch.digest.data(), cfg.pow_bits, st);
    ch.mix_u64(pf.proof_of_work);
    P.tick("pow");
  }
  // the first-layer tree and every layer above 2^stop rows, by row range
  void fri_sharded_layers() {
    for (auto& g : gs)
      for (int c = 0; c < 4; c++) { fri_first.lde_logs.push_back(g.log); fri_first.slice.push_back(g.out.ptrs[c]); }
    const uint32_t stop = std::max(shard_fri_stop_log(), logN + 5);   // a slice keeps at least 2^5 rows
    const uint32_t n_slots = 1 + (layer_log > last_log ? layer_log - last_log : 0);   // first-layer tree + every possible inner layer
    const size_t slot_words = 4 + 8 + 8 * (size_t)N;                                     // {challenge, root, sub-roots} per tree
    uint32_t *d_chan = nullptr, *d_slots = nullptr;
    std::vector<SlicedTree*> order;   // the trees in transcript order
    auto d_alpha = [&](size_t k) { return d_slots + k * slot_words; };
    auto tree_step = [&](SlicedTree& t) {   // tree -> root -> challenge: on the stream, or through the host
      if (fri_stream) {
        enqueue_sliced(cm, t);
        const size_t k = order.size();
        shard_top_step(comm_c.recv_buf, N, d_chan, d_alpha(k), d_alpha(k) + 4, d_alpha(k) + 12, st);
        order.push_back(&t);
        return QM31();
      }
      finish_sliced(cm, t);
      ch.mix_root(t.root);
      return ch.draw_felt();
    };
    if (fri_stream) {
      d_fs.alloc((16 + n_slots * slot_words) * 4);
      d_chan = d_fs.u32();
      d_slots = d_chan + 16;
      uint32_t cw[16] = {0};
      channel_words(ch, cw);
      stage_upload(d_chan, cw, sizeof(cw), st);
    }
    alpha_c = tree_step(fri_first);
    // A layer object exists BEFORE its values: the fold that produces them — fold_circle of the quotient group of that size into a
    // blank first layer, fold_line of the previous layer, or both — hashes the leaf layer of the layer's subtree in the same pass when
    // it can (k_fold_leaf on the row range: the single-GPU prover's fused kernel, "fri_fold_leaf"; device challenges only).
    auto new_layer = [&](uint32_t log) {
      std::unique_ptr<ShardedFriLayer> L(new ShardedFriLayer());
      L->log = log;
      L->slice.alloc(std::vector<uint32_t>(4, log - logN), st, false);
      L->tree.lde_logs.assign(4, log);
      for (int c = 0; c < 4; c++) L->tree.slice.push_back(L->slice.ptrs[c]);
      return L;
    };
    auto produce = [&](ShardedFriLayer& X, const ShardedFriLayer* prev, size_t prev_slot, const QM31& prev_alpha) {
      const uint32_t n_loc = 1u << (X.log - logN), row0 = R * n_loc;
      size_t n_groups = 0;
      while (qi_next + n_groups < gs.size() && gs[qi_next + n_groups].log - 1 == X.log) n_groups++;
      CM_CHECK(prev || n_groups, "fri: the first layer received no quotient column");
      const uint32_t* lsrc[4] = {nullptr, nullptr, nullptr, nullptr};
      if (prev) for (int c = 0; c < 4; c++) lsrc[c] = prev->slice.ptrs[c];
      if (fri_stream && n_groups <= 1) {
        sliced_prepare(cm, X.tree, st);
        uint32_t* leaves = sliced_leaf_target(X.tree);
        const uint32_t* circ[4] = {nullptr, nullptr, nullptr, nullptr};
        if (n_groups) for (int c = 0; c < 4; c++) circ[c] = gs[qi_next].out.ptrs[c];
        const bool fused = leaves && (prev ? fold_line_leaf(X.slice.ptrs.data(), lsrc, n_groups ? circ : nullptr, prev->log, *P.tw, st, d_alpha(prev_slot), d_alpha(0), leaves, row0, n_loc)
                                           : fold_circle_leaf(X.slice.ptrs.data(), circ, gs[qi_next].log, *P.tw, st, d_alpha(0), leaves, row0, n_loc));
        if (fused) { X.tree.leaf_done = true; qi_next += n_groups; return; }
      }
      bool blank = true;
      if (prev) { fold_line_rows(X.slice.ptrs.data(), lsrc, prev->log, *P.tw, prev_alpha, row0, n_loc, st, fri_stream ? d_alpha(prev_slot) : nullptr); blank = false; }
      for (size_t k = 0; k < n_groups; k++, qi_next++) {
        const uint32_t* src[4] = {gs[qi_next].out.ptrs[0], gs[qi_next].out.ptrs[1], gs[qi_next].out.ptrs[2], gs[qi_next].out.ptrs[3]};
        fold_circle_into_line_rows(X.slice.ptrs.data(), src, gs[qi_next].log, *P.tw, alpha_c, !blank, row0, n_loc, st, fri_stream ? d_alpha(0) : nullptr);
        blank = false;
      }
    };
    std::unique_ptr<ShardedFriLayer> L;   // the layer whose values are complete and whose tree comes next
    if (layer_log > last_log && layer_log > stop) {
      L = new_layer(layer_log);
      produce(*L, nullptr, 0, QM31());
    }
    while (L) {
      const size_t slot = order.size();
      const QM31 alpha = tree_step(L->tree);
      const uint32_t next_log = layer_log - 1;
      if (next_log > last_log && next_log > stop) {
        std::unique_ptr<ShardedFriLayer> X = new_layer(next_log);
        produce(*X, L.get(), slot, alpha);
        sfl.push_back(std::move(L));
        L = std::move(X);
      } else {
        // the hand-over layer: this rank's rows of it (the quotient group of that size is folded in by FriPhase::commit)
        const uint32_t n_loc = 1u << (next_log - logN);
        cur = ColumnSet();
        cur.alloc(std::vector<uint32_t>(4, next_log - logN), st, false);
        const uint32_t* lsrc[4] = {L->slice.ptrs[0], L->slice.ptrs[1], L->slice.ptrs[2], L->slice.ptrs[3]};
        fold_line_rows(cur.ptrs.data(), lsrc, layer_log, *P.tw, alpha, R * n_loc, n_loc, st, fri_stream ? d_alpha(slot) : nullptr);
        cur_valid = true;
        sfl.push_back(std::move(L));
      }
      layer_log = next_log;
    }
    if (fri_stream) {
      // the host's half, once: sub-roots -> top levels + root of every tree (the decommitment needs the nodes), transcript replay —
      // NOT here: the words travel to pinned memory behind an event, the replicated layers are enqueued first (FriPhase takes the
      // device channel and the circle-fold challenge from device memory: FriResume::d_chan / d_alpha_c) and the host replays while
      // they run (fri_replay below).  It used to stop the stream: ~70 us of idle GPU in the round-6 timeline.
      CM_CHECK(order.size() * slot_words <= PIN_WORDS - PIN_SHARD_FRI, "sharded fri: more layers than the pinned slot holds");
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_SHARD_FRI, d_slots, order.size() * slot_words * 4, hipMemcpyDeviceToHost, st));
      fri_back_land = pinned_words() + PIN_SHARD_FRI;
      static thread_local hipEvent_t ev = nullptr;
      CM_HIP(hipEventRecord(ev_fri_back = thread_event(ev), st));
      fri_order = order; fri_slot_words = slot_words;
      rs_d_chan = d_chan; rs_d_alpha_c = d_alpha(0);
    } else pf.fri_first.commitment = fri_first.root;
  }
  void fri_replay() {
    if (!ev_fri_back) return;   // (the host-driven form replayed every step where it happened)
    CM_HIP(hipEventSynchronize(ev_fri_back));
    for (size_t k = 0; k < fri_order.size(); k++) {
      const uint32_t* w = &fri_back_land[k * fri_slot_words];
      complete_sliced(cm, *fri_order[k], w + 12);
      CM_CHECK(memcmp(fri_order[k]->root.data(), w + 4, 32) == 0, "sharded fri: the device's tree top differs from the host's");
      ch.mix_root(fri_order[k]->root);
      const QM31 a = ch.draw_felt();
      CM_CHECK(a == QM31::from_u32(w), "sharded fri: the device transcript diverged from the host channel");
    }
    pf.fri_first.commitment = fri_first.root;
  }
  // hand-over: the current layer's slices and the quotient groups not folded yet -> full columns on every rank
  void fri_hand_over() {
    if (N == 1) {
      // a lone rank's slices ARE the columns: the layer moves, the quotient groups not folded yet are aliased (their storage stays
      // with `gs`, which the decommitment of the first-layer tree reads and which outlives `quotients`' users)
      const size_t g0 = shard_fri ? qi_next : 0;
      if (cur_valid) full_layer = std::move(cur);
      for (size_t gi = 0; gi < gs.size(); gi++) {
        quotients.emplace_back();
        if (gi >= g0) { quotients.back().logs.assign(4, gs[gi].log); quotients.back().ptrs = gs[gi].out.ptrs; }
      }
    } else {
      const size_t g0 = shard_fri ? qi_next : 0;
      uint64_t per_rank = 0;
      if (cur_valid) per_rank += (uint64_t)4 << (layer_log - logN);
      for (size_t gi = g0; gi < gs.size(); gi++) per_rank += (uint64_t)4 << (gs[gi].log - logN);
      cm.need(per_rank * N);
      {
        std::vector<CopySeg> segs;
        uint64_t off = 0;
        if (cur_valid) for (int c = 0; c < 4; c++) { const uint64_t sl = (uint64_t)1 << (layer_log - logN); segs.push_back(CopySeg{cur.ptrs[c], comm_c.send_buf + off, sl}); off += sl; }
        for (size_t gi = g0; gi < gs.size(); gi++)
          for (int c = 0; c < 4; c++) { const uint64_t sl = (uint64_t)1 << (gs[gi].log - logN); segs.push_back(CopySeg{gs[gi].out.ptrs[c], comm_c.send_buf + off, sl}); off += sl; }
        copy_segments(segs, st);
      }
      cm.all_gather(per_rank);
      {
        std::vector<CopySeg> segs;
        if (cur_valid) full_layer.alloc(std::vector<uint32_t>(4, layer_log), st, false);
        for (size_t gi = 0; gi < gs.size(); gi++) {
          quotients.emplace_back();
          if (gi >= g0) quotients.back().alloc(std::vector<uint32_t>(4, gs[gi].log), st, false);
        }
        for (uint32_t sr = 0; sr < N; sr++) {
          uint64_t off = (uint64_t)sr * per_rank;
          if (cur_valid) for (int c = 0; c < 4; c++) { const uint64_t sl = (uint64_t)1 << (layer_log - logN); segs.push_back(CopySeg{comm_c.recv_buf + off, full_layer.ptrs[c] + (uint64_t)sr * sl, sl}); off += sl; }
          for (size_t gi = g0; gi < gs.size(); gi++)
            for (int c = 0; c < 4; c++) {
              const uint64_t sl = (uint64_t)1 << (gs[gi].log - logN);
              segs.push_back(CopySeg{comm_c.recv_buf + off, quotients[gi].ptrs[c] + (uint64_t)sr * sl, sl});
              off += sl;
            }
        }
        copy_segments(segs, st);
      }
    }
  }
  // queries + decommitment
  void decommit() {
    hm.mark("pow done");
    Queries queries = Queries::draw(ch, cfg.n_queries, q_logs[0]);
    std::map<uint32_t, std::vector<uint32_t>> qpos;
    for (auto l : q_logs) qpos[l] = queries.fold(queries.log_domain_size - l).positions;
    {
      // two gathers: (A) the replicated FRI layers + the four commitment trees — enqueued as soon as it is planned, so that it runs while
      // the host plans (B) the row-sharded FRI layers; one wait for both
      GatherBatch gb, gbB;
      fri.plan_decommit(queries, qpos, quotients, q_logs, gb);
      hm.mark("decommit: queries + replicated plan");   // the replicated layers (and the first-layer tree when FRI is not sharded)
      const SlicedTree* slt[4] = {&sl0, &sl1, &sl2, &sl3};
      pf.decommitments.resize(4);
      pf.queried_values.resize(4);
      // sections in one fixed order on every rank: the four commitment trees, then the row-sharded FRI layers
      std::vector<std::unique_ptr<ShardSection>> secs;
      auto new_sec = [&]() -> ShardSection& { secs.emplace_back(new ShardSection()); return *secs.back(); };
      for (int t = 0; t < 4; t++) {
        ShardSection& sc = new_sec();
        sc.d = &pf.decommitments[t]; sc.qv = &pf.queried_values[t]; sc.gb = &gb;
        plan_sharded_decommit(*slt[t], cm, qpos, gb, sc.fetch, sc.sd);
      }
      hm.mark("decommit: four trees planned");
      // pinned landing words of both gathers: A's size is known, B's is bounded (per sharded tree and query: two hashes and a
      // handful of values per layer); a B beyond the bound — never seen — waits for A and takes the landing buffer for itself
      const size_t wordsA = gb.total_words();
      const size_t boundB = (sfl.size() + 1 + gs.size()) * (size_t)cfg.n_queries * 24 * 32;
      uint32_t* const land = (uint32_t*)stage_landing((wordsA + boundB) * 4, st);
      gb.enqueue(st, land);
      pf.fri_inner.reserve(sfl.size() + fri.inner.size());   // sections keep pointers into the first entries: no reallocation later
      pf.fri_inner.resize(sfl.size());
      if (shard_fri) {
        std::map<uint32_t, std::vector<uint32_t>> first_dpos;
        for (auto& g : gs) {
          ShardSection& sc = new_sec();
          sc.wit = &pf.fri_first.fri_witness; sc.gb = &gbB;
          std::vector<uint32_t> pos;
          plan_fri_positions_sharded(cm, g.log, g.out.ptrs.data(), qpos.at(g.log), pos, gbB, sc.fetch, sc.sd);
          first_dpos[g.log] = std::move(pos);
        }
        {
          ShardSection& sc = new_sec();
          sc.d = &pf.fri_first.decommitment; sc.gb = &gbB;
          plan_sharded_decommit(fri_first, cm, first_dpos, gbB, sc.fetch, sc.sd);
        }
        Queries lq = queries.fold(1);
        for (size_t i = 0; i < sfl.size(); i++) {
          ShardedFriLayer& L = *sfl[i];
          std::map<uint32_t, std::vector<uint32_t>> dpos;
          {
            ShardSection& sc = new_sec();
            sc.wit = &pf.fri_inner[i].fri_witness; sc.gb = &gbB;
            plan_fri_positions_sharded(cm, L.log, L.slice.ptrs.data(), lq.positions, dpos[L.log], gbB, sc.fetch, sc.sd);
          }
          ShardSection& sc = new_sec();
          sc.d = &pf.fri_inner[i].decommitment; sc.gb = &gbB;
          plan_sharded_decommit(L.tree, cm, dpos, gbB, sc.fetch, sc.sd);
          pf.fri_inner[i].commitment = L.tree.root;
          lq = lq.fold(1);
        }
      }
      hm.mark("decommit: sharded FRI planned");
      std::vector<uint32_t> keepA;
      if (gbB.total_words() <= boundB) {
        gbB.enqueue(st, land + wordsA);
        CM_HIP(hipStreamSynchronize(st));
      } else {
        CM_HIP(hipStreamSynchronize(st));
        keepA.assign(land, land + wordsA);
        gb.words = keepA.data() + (gb.words - land); gb.hashes = keepA.data() + (gb.hashes - land); gb.run_out = keepA.data() + (gb.run_out - land);
        gbB.run(st);
      }
      hm.mark("decommit: gather ran");
      const FriLayerProofData* const inner_base = pf.fri_inner.data();
      fri.finish_decommit(gb, pf);   // appends the replicated inner layers behind the sharded ones
      CM_CHECK(pf.fri_inner.data() == inner_base, "sharded decommitment: fri_inner was reallocated under the section pointers");
      // my items of every section, in script order -> all ranks (a lone rank has nobody to tell: it assembles straight from the gather)
      auto fetched = [&](const ShardSection& sc, const std::pair<int, size_t>& f) -> const uint32_t* {
        return f.first == 0 ? &sc.gb->hashes[8 * f.second] : f.first == 1 ? &sc.gb->run_out[f.second] : &sc.gb->words[f.second];
      };
      std::vector<uint32_t> all;
      uint64_t maxw = 0;
      if (N > 1) {
        for (uint32_t k = 0; k < N; k++) {
          uint64_t w = 0;
          for (auto& sc : secs) w += sc->sd.words_of[k];
          maxw = std::max(maxw, w);
        }
        std::vector<uint32_t> mine_items;
        mine_items.reserve(maxw);
        for (auto& sc : secs) {
          size_t fi = 0;
          for (auto& item : sc->sd.script) {
            if (item.kind == 2 || item.owner != R) continue;
            const uint32_t* w = fetched(*sc, sc->fetch[fi++]);
            mine_items.insert(mine_items.end(), w, w + item.count);
          }
        }
        mine_items.resize(maxw, 0);
        all = cm.gather_host(mine_items);
      }
      hm.mark("decommit: items gathered");
      std::vector<size_t> cursor(N);
      for (uint32_t k = 0; k < N; k++) cursor[k] = (size_t)k * maxw;
      for (auto& sc : secs) {
        size_t fi = 0;
        {   // one pass over the 8-byte items sizes the section's vectors (a proof carries ~1 MB of witnesses: no regrowth while copying)
          size_t nh = 0, nw = 0, nq = 0, nf = 0;
          for (auto& item : sc->sd.script) {
            if (item.kind == 0 || item.kind == 2) nh++;
            else if (item.kind == 3) nf++;
            else if (item.is_query) nq += item.count;
            else nw += item.count;
          }
          if (sc->d) { sc->d->hash_witness.reserve(sc->d->hash_witness.size() + nh); sc->d->column_witness.reserve(sc->d->column_witness.size() + nw); }
          if (sc->qv) sc->qv->reserve(sc->qv->size() + nq);
          if (sc->wit) sc->wit->reserve(sc->wit->size() + nf);
        }
        for (auto& item : sc->sd.script) {
          if (item.kind == 2) { sc->d->hash_witness.push_back(sc->sd.host_hashes[item.count]); continue; }
          const uint32_t* w = item.owner == R ? fetched(*sc, sc->fetch[fi++]) : &all[cursor[item.owner]];   // own items: from the gather itself
          cursor[item.owner] += item.count;
          if (item.kind == 0) { Hash32 h; memcpy(h.data(), w, 32); sc->d->hash_witness.push_back(h); }
          else if (item.kind == 3) sc->wit->push_back(QM31::from_u32(w));
          else if (item.is_query) { if (sc->qv) sc->qv->insert(sc->qv->end(), w, w + item.count); }
          else sc->d->column_witness.insert(sc->d->column_witness.end(), w, w + item.count);
        }
      }
      pf.commitments = {sl0.root, sl1.root, sl2.root, sl3.root};
    }
    hm.mark("decommit: assembled");
    P.tick("decommit");
  }
};

ProofData* prove_sharded(const DeviceInput& din, const cm_pcs_config& cfg, const cm_comm& comm_c) {
  if (const uint64_t budget = mem_budget())   // a lone proof has nothing to wait for: it fits or it is refused before any GPU work
    check_item_fits(item_bytes(din.meta, device_input_bytes(din), cfg, std::max(comm_c.world, 1u)), budget, "cm_prove_sharded");
  struct InFlight { InFlight() { mem_proof_enter(); } ~InFlight() { mem_proof_leave(); } } mem_in_flight;
  return ShardedProver(din, cfg, comm_c).run();
}
