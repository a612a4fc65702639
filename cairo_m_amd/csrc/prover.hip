// Whole-segment HIP prover: `prove_cairo_m::<Blake2sMerkleChannel>`
// (/root/reference/crates/prover/src/prover.rs:23-147; transcript order is normative) driving the gfx950
// kernels.  Host code here only sequences launches, runs the Fiat-Shamir channel, and assembles the proof;
// every pass over trace data (trace gen, LogUp, IFFT/LDE, Merkle, constraints, OODS sampling, DEEP
// quotients, FRI folds, PoW search, decommit gathers) is a kernel.  No CPU fallback exists.
#include "../../include/cairom_hip.h"
#include "prover_common.hpp"
#include "quotient_plan.hpp"
#include "constraint_plan.hpp"
#include "proof_context.hpp"
#include "air_kernels.hpp"
#include "gpu_air.hpp"
#include "point_eval.hpp"
#include "host_adapter.hpp"
#include "shard_kernels.hpp"
#include "segment_input.hpp"
#include "tail_plan.hpp"
#include "prover_api.hpp"
#include <atomic>
#include <chrono>
#include <deque>
#include <condition_variable>
#include <thread>
#include <memory>
#include <mutex>
#include <map>
#include <set>
#include <algorithm>
#include <functional>

namespace cm {

// (log_size_for, DeviceInput: segment_input.hpp)

// PublicData::new (public_data.rs:244-272) in two halves: the registers, clock and roots from the input's scalars, and the entries
// of the three public ranges — from the host rows (make_public_data) or gathered on the device by a run's adapter
// (public_data_from_entries)
static PublicData public_data_scalars(const cm_prover_input& in) {
  PublicData d;
  d.initial_pc = in.initial_pc; d.initial_fp = in.initial_fp; d.final_pc = in.final_pc; d.final_fp = in.final_fp;
  uint64_t steps = 0;
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) steps += in.n_bundles[i];
  d.clock = M31::reduce(steps).v;
  d.initial_root = in.initial_root; d.final_root = in.final_root;
  for (uint32_t w : {d.initial_pc, d.initial_fp, d.final_pc, d.final_fp, d.initial_root, d.final_root})
    CM_CHECK(w < P, "ProverInput: a public register / root word is not a canonical M31");
  return d;
}
static void check_public_entry(const PublicEntry& e) {
  CM_CHECK(e.addr < P && e.clock < P && e.value[0] < P && e.value[1] < P && e.value[2] < P && e.value[3] < P,
           "ProverInput: a public memory entry is not made of canonical M31 words");
}
// entries = program, input, output laid end to end, one per address of each range (present = 0 where the boundary memory has no cell)
static PublicData public_data_from_entries(const cm_prover_input& in, const PublicEntry* entries) {
  PublicData d = public_data_scalars(in);
  const PublicEntry* e = entries;
  auto take = [&](std::vector<PublicEntry>& v, const uint32_t range[2]) {
    const uint32_t n = range[1] > range[0] ? range[1] - range[0] : 0u;
    v.assign(e, e + n);
    for (const PublicEntry& x : v) if (x.present) check_public_entry(x);
    e += n;
  };
  take(d.program, in.program_range); take(d.input, in.input_range); take(d.output, in.output_range);
  return d;
}
static PublicData make_public_data(const cm_prover_input& in) {
  PublicData d = public_data_scalars(in);
  std::map<uint32_t, const cm_memory_cell*> init, fin;
  for (uint64_t i = 0; i < in.n_initial_memory; i++) init[in.initial_memory[i].address] = &in.initial_memory[i];
  for (uint64_t i = 0; i < in.n_final_memory; i++) fin[in.final_memory[i].address] = &in.final_memory[i];
  auto extract = [](const std::map<uint32_t, const cm_memory_cell*>& m, const uint32_t range[2]) {
    std::vector<PublicEntry> v;
    for (uint32_t a = range[0]; a < range[1]; a++) {
      PublicEntry e{};
      auto it = m.find(a);
      if (it != m.end()) {
        e.present = 1; e.addr = a; for (int k = 0; k < 4; k++) e.value[k] = it->second->value[k]; e.clock = it->second->clock;
        check_public_entry(e);
      }
      v.push_back(e);
    }
    return v;
  };
  d.program = extract(init, in.program_range);
  d.input = extract(init, in.input_range);
  d.output = extract(fin, in.output_range);
  return d;
}

// `st` = null: blocking copies on the NULL stream + a device-wide synchronisation (the one-shot form).  Otherwise every copy is
// enqueued on `st` and only `st` is waited for — the streaming ingest (cm_prove_many_host) uploads segment k + 1 on the calling
// thread's stream while the workers' proofs of segments <= k keep the GPU busy; a device-wide wait would stall the uploader
// behind every proof in flight.
DeviceInput* upload_input(const cm_prover_input& in, hipStream_t st) {
  bind_thread_to_library_device();
  std::unique_ptr<DeviceInput> dh(new DeviceInput());
  DeviceInput* d = dh.get();
  d->meta = in;
  auto up = [st](DevBuf& b, const void* p, size_t bytes) {
    b.alloc(bytes);
    if (!bytes) return;
    if (st) CM_HIP(hipMemcpyAsync(b.p, p, bytes, hipMemcpyHostToDevice, st));
    else CM_HIP(hipMemcpy(b.p, p, bytes, hipMemcpyHostToDevice));
  };
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) up(d->bundles[i], in.bundles[i], in.n_bundles[i] * sizeof(cm_bundle));
  up(d->data_accesses, in.data_accesses, in.n_data_accesses * sizeof(cm_data_access));
  up(d->init_mem, in.initial_memory, in.n_initial_memory * sizeof(cm_memory_cell));
  up(d->fin_mem, in.final_memory, in.n_final_memory * sizeof(cm_memory_cell));
  up(d->clock_updates, in.clock_updates, in.n_clock_updates * sizeof(cm_clock_update));
  up(d->init_tree, in.initial_tree, in.n_initial_tree * sizeof(cm_merkle_node));
  up(d->fin_tree, in.final_tree, in.n_final_tree * sizeof(cm_merkle_node));
  d->public_data = make_public_data(in);
  if (st) CM_HIP(hipStreamSynchronize(st));
  else CM_HIP(hipDeviceSynchronize());   // the copies ran on the NULL stream; the prover's streams are non-blocking
  return dh.release();
}

// device adapter (adapter_device.hip): bulk arrays already live in HBM, the small boundary-memory / Merkle-tree
// arrays come from the host (pointers in `meta`, valid during the call)
DeviceInput* make_device_input(const cm_prover_input& meta, DevBuf (&bundles)[CM_N_OPCODE_COMPONENTS], DevBuf& data_accesses,
                               DevBuf& clock_updates, DevBuf* init_tree_dev, DevBuf* fin_tree_dev) {
  DeviceInput* d = new DeviceInput();
  d->meta = meta;
  auto up = [](DevBuf& b, const void* p, size_t bytes) {
    b.alloc(bytes);
    if (bytes) CM_HIP(hipMemcpy(b.p, p, bytes, hipMemcpyHostToDevice));
  };
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) d->bundles[i] = std::move(bundles[i]);
  d->data_accesses = std::move(data_accesses);
  d->clock_updates = std::move(clock_updates);
  up(d->init_mem, meta.initial_memory, meta.n_initial_memory * sizeof(cm_memory_cell));
  up(d->fin_mem, meta.final_memory, meta.n_final_memory * sizeof(cm_memory_cell));
  if (init_tree_dev) d->init_tree = std::move(*init_tree_dev);   // trees hashed on the GPU by the device adapter
  else up(d->init_tree, meta.initial_tree, meta.n_initial_tree * sizeof(cm_merkle_node));
  if (fin_tree_dev) d->fin_tree = std::move(*fin_tree_dev);
  else up(d->fin_tree, meta.final_tree, meta.n_final_tree * sizeof(cm_merkle_node));
  d->public_data = make_public_data(meta);
  // the host pointers of `meta` die with the caller's temporaries
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) d->meta.bundles[i] = nullptr;
  d->meta.data_accesses = nullptr; d->meta.initial_memory = nullptr; d->meta.final_memory = nullptr;
  d->meta.clock_updates = nullptr; d->meta.initial_tree = nullptr; d->meta.final_tree = nullptr;
  CM_HIP(hipDeviceSynchronize());   // NULL-stream copies above; the prover's streams are non-blocking
  return d;
}
// a run's adapter (adapter_run.inc): every array already lives in the calling thread's pool and its stream has been waited for;
// no copy, no wait here
DeviceInput* make_device_input_resident(const cm_prover_input& meta, DevBuf (&bundles)[CM_N_OPCODE_COMPONENTS], DevBuf& data_accesses, DevBuf& clock_updates,
                                        DevBuf& init_mem, DevBuf& fin_mem, DevBuf& init_tree, DevBuf& fin_tree, const PublicEntry* entries) {
  std::unique_ptr<DeviceInput> d(new DeviceInput());
  d->meta = meta;   // (every pointer of it is null)
  d->public_data = public_data_from_entries(meta, entries);
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) d->bundles[i] = std::move(bundles[i]);
  d->data_accesses = std::move(data_accesses);
  d->clock_updates = std::move(clock_updates);
  d->init_mem = std::move(init_mem); d->fin_mem = std::move(fin_mem);
  d->init_tree = std::move(init_tree); d->fin_tree = std::move(fin_tree);
  return d.release();
}
// (adapt_segment_device, the run object and the openers: prover_api.hpp)
// copy a device-resident input back to the host (tests)
void download_input(const DeviceInput& d, host::ProverInputOwned& o) {
  CM_HIP(hipDeviceSynchronize());
  const cm_prover_input& m = d.meta;
  o.initial_pc = m.initial_pc; o.initial_fp = m.initial_fp; o.final_pc = m.final_pc; o.final_fp = m.final_fp;
  o.initial_root = m.initial_root; o.final_root = m.final_root;
  for (int i = 0; i < 2; i++) { o.program_range[i] = m.program_range[i]; o.input_range[i] = m.input_range[i]; o.output_range[i] = m.output_range[i]; }
  auto down = [](auto& vec, const DevBuf& b, uint64_t n) {
    vec.resize(n);
    if (n) CM_HIP(hipMemcpy(vec.data(), b.p, n * sizeof(vec[0]), hipMemcpyDeviceToHost));
  };
  o.n_steps = 0;
  for (int i = 0; i < CM_N_OPCODE_COMPONENTS; i++) { down(o.bundles[i], d.bundles[i], m.n_bundles[i]); o.n_steps += m.n_bundles[i]; }
  down(o.data_accesses, d.data_accesses, m.n_data_accesses);
  down(o.initial_memory, d.init_mem, m.n_initial_memory);
  down(o.final_memory, d.fin_mem, m.n_final_memory);
  down(o.clock_updates, d.clock_updates, m.n_clock_updates);
  down(o.initial_tree, d.init_tree, m.n_initial_tree);
  down(o.final_tree, d.fin_tree, m.n_final_tree);
}

// Optional cache of tree 0.  The preprocessed columns are constants (preprocessed/mod.rs:75-82), so their
// coefficients, LDE and Merkle tree are the same for every proof of one PCS config.  OFF by default — a proof then
// recomputes them like the reference does (prover.rs:70-73) and bench.py times that; cm_set_preprocessed_cache(1) or
// CM_PREPROCESSED_CACHE=1 keeps the committed tree per host thread (it lives in that thread's device pool).
std::atomic<int> g_pp_cache{-1};
static bool pp_cache_enabled() {
  int v = g_pp_cache.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("CM_PREPROCESSED_CACHE");
    v = (e && *e && *e != '0') ? 1 : 0;
    g_pp_cache.store(v, std::memory_order_relaxed);
  }
  return v == 1;
}
struct PreprocessedCache {
  bool valid = false;
  uint32_t log_blowup = 0;
  ColumnSet evals;     // the tables on their trace domains: the LogUp pass of rc8/16/20 and bitwise reads them
  CommittedTree tree;
};
static thread_local PreprocessedCache tl_pp_cache;


// CM_NO_SMALL_BATCH=1: one launch per small component again (A/B of the batched small-component kernels)
static bool no_small_batch() { static const bool v = getenv("CM_NO_SMALL_BATCH") != nullptr; return v; }

// Twiddle tables.  The reference recomputes them in every prove_cairo_m (`SimdBackend::precompute_twiddles`, prover.rs:56-60),
// so by default every proof builds its own tables (in pool memory, on a side stream next to trace generation); they
// depend only on the domain size, and cm_set_twiddle_cache(1) / CM_TWIDDLE_CACHE=1 keeps one table per size for the
// process instead (OFF in every quoted number, like the preprocessed-tree cache).
std::atomic<int> g_tw_cache{-1};
static bool tw_cache_enabled() {
  int v = g_tw_cache.load(std::memory_order_relaxed);
  if (v < 0) {
    const char* e = getenv("CM_TWIDDLE_CACHE");
    v = (e && *e && *e != '0') ? 1 : 0;
    g_tw_cache.store(v, std::memory_order_relaxed);
  }
  return v == 1;
}
static Twiddles* cached_twiddles(uint32_t R, hipStream_t st) {
  static std::mutex mu;
  static std::map<uint32_t, Twiddles*> cache;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(R);
  if (it != cache.end()) return it->second;
  Twiddles* t = twiddles_create(R, st);
  CM_HIP(hipStreamSynchronize(st));  // other host threads use the tables from their own streams
  cache[R] = t;
  return t;
}
// (MemSwitches, estimate_memory: mem_estimate.hpp)
MemSwitches mem_switches() { return MemSwitches{pp_cache_enabled(), tw_cache_enabled(), tune(T_DEFER_TEARDOWN) != 0}; }
// ---- memory budget (cm_set_memory_budget) ----------------------------------------------------------------------------------
// What one item needs: its resident input and the estimate's bound on what its proof adds to the proving thread's pool.
struct ItemBytes { uint64_t input = 0, working = 0; };
static ItemBytes item_bytes(const cm_prover_input& meta, uint64_t input_bytes, const cm_pcs_config& cfg, uint32_t world) {
  uint32_t clog[air::N_COMPONENTS];
  component_logs(meta, clog);
  cm_mem_estimate e;
  memset(&e, 0, sizeof(e));
  cm_pcs_config c = cfg;
  c.log_blowup_factor = std::min(std::max(c.log_blowup_factor, 1u), 4u);   // (an invalid config is refused by the prover itself)
  for (auto& l : clog) l = std::min(l, 27u);
  estimate_memory(clog, c, world, mem_switches(), e);
  return ItemBytes{input_bytes, e.working_bytes};
}
// the third rule of the budget: an item that cannot fit alone fails before any GPU work for it
static void check_item_fits(const ItemBytes& b, uint64_t budget, const char* who) {
  if (budget && b.input + b.working > budget)
    throw CmError(2, std::string(who) + ": the item needs input_bytes " + std::to_string(b.input) + " + working_bytes " + std::to_string(b.working) +
                         " = " + std::to_string(b.input + b.working) + " bytes, the memory budget is " + std::to_string(budget));
}
// Admission by bytes for the pipelines (process-wide, like the budget): `inputs` = device inputs resident for them, `working` =
// the estimates of the proofs running.  Nothing waits when no budget is set; when nothing is running the next item is always
// admitted, so an item that fits alone can never wait for ever.
struct Admission {
  std::mutex mu;
  std::condition_variable cv;
  uint64_t inputs = 0, working = 0;
  uint32_t running = 0;
  void add_inputs(uint64_t b) { std::lock_guard<std::mutex> lk(mu); inputs += b; }
  void sub_inputs(uint64_t b) { { std::lock_guard<std::mutex> lk(mu); inputs -= std::min(inputs, b); } cv.notify_all(); }
  // a producer, before it makes a device input of `b` bytes (counted as resident from here on).  Never blocks: a producer that
  // waits for room must keep releasing the inputs that come back to it — their release may be the room
  bool try_admit_input(uint64_t b) {
    std::lock_guard<std::mutex> lk(mu);
    const uint64_t bud = mem_budget();
    if (bud && inputs + working + b > bud && !(running == 0 && inputs == 0)) return false;
    inputs += b;
    return true;
  }
  // a worker, before it starts a proof whose estimate is `w`
  void admit_proof(uint64_t w) {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { const uint64_t bud = mem_budget(); return !bud || inputs + working + w <= bud || running == 0; });
    working += w; running++;
  }
  void finish_proof(uint64_t w) {
    { std::lock_guard<std::mutex> lk(mu); working -= std::min(working, w); running--; }
    cv.notify_all();
  }
};
static Admission& admission() { static Admission* a = new Admission(); return *a; }
// One proof of a pipeline worker under the admission rules.  With a budget the worker gives back what its previous proof parked
// before it waits (parked blocks are live bytes nobody admitted), and trims its pool when the process holds more than the budget.
static ProofData* prove_admitted(const DeviceInput& din, const cm_pcs_config& cfg, const char* who) {
  const uint64_t budget = mem_budget();
  if (!budget) return prove(din, cfg);
  const ItemBytes b = item_bytes(din.meta, device_input_bytes(din), cfg, 1);
  check_item_fits(b, budget, who);
  release_thread_parked();
  {
    cm_mem_stats s;
    s.struct_size = sizeof(s);
    if (cm_mem_stats_get(&s) == 0 && s.reserved_bytes > budget) pool_trim();
  }
  Admission& a = admission();
  a.admit_proof(b.working);
  struct Done { Admission& a; uint64_t w; ~Done() { release_thread_parked(); a.finish_proof(w); } } done{a, b.working};
  return prove(din, cfg);
}
struct ProofTwiddles {   // per-proof tables in pool memory
  Twiddles t;
  DevBuf x, ix, y, iy, scratch;
  void build(uint32_t R, hipStream_t s) {
    t.R = R;
    x.alloc((size_t)4 << (R - 1)); ix.alloc((size_t)4 << (R - 1)); y.alloc((size_t)4 << R); iy.alloc((size_t)4 << R);
    scratch.alloc(twiddles_scratch_words(R) * 4);
    t.xtw = x.u32(); t.ixtw = ix.u32(); t.ytw = y.u32(); t.iytw = iy.u32(); t.scratch = scratch.u32();
    twiddles_build(t, s);
  }
};

// (coset_vanishing_canonic, zero_ranges: constraint_plan.hpp)
// (component_logs: segment_input.hpp)
// ---- transcript steps shared by the single-GPU and the sharded prover ------------------------------------------------------
// PcsConfig::mix_into + PublicData::mix_into (prover.rs:33-36, 62-66)
static void mix_config_and_public_data(Channel& ch, const cm_pcs_config& cfg, const PublicData& d) {
  // PcsConfig::mix_into + FriConfig::mix_into (prover.rs:36); the order inside FriConfig is a framing switch (framing.hpp `pcs_mix`)
  ch.mix_u64(cfg.pow_bits);
  ch.mix_u64(cfg.log_blowup_factor);
  if (framing().pcs_mix_blq) { ch.mix_u64(cfg.log_last_layer_degree_bound); ch.mix_u64(cfg.n_queries); }
  else { ch.mix_u64(cfg.n_queries); ch.mix_u64(cfg.log_last_layer_degree_bound); }
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
// (draw_relations: segment_input.hpp)
// random coefficient of the composition polynomial: powers[g] = rho^(total - 1 - g), uploaded as words
static void draw_constraint_powers(Channel& ch, std::vector<QM31>& powers, DevBuf& d_powers, hipStream_t st) {
  QM31 random_coeff = ch.draw_felt();
  QM31 cur(M31(1));
  const size_t total = powers.size();
  for (size_t g = total; g-- > 0;) { powers[g] = cur; cur = cur * random_coeff; }
  std::vector<uint32_t> powers_w(4 * total);
  for (size_t g = 0; g < total; g++) powers[g].to_u32(&powers_w[4 * g]);
  stage_upload(d_powers.p, powers_w.data(), powers_w.size() * 4, st);
}

// Sanity check of stwo `prove`: the composition polynomial's OODS value equals the constraints evaluated on the sampled mask
// values (host-only work; both provers run it while the GPU is busy with the quotient / FRI kernels).
static void check_composition_at_oods(const ProofData& pf, const std::vector<size_t>& tr0, const std::vector<size_t>& it0, const uint32_t* clog,
                                      const HostRelations& hrel, const std::vector<QM31>& powers, const std::vector<size_t>& coff,
                                      const CPoint<QM31>& oods) {
  QM31 c4[4] = {pf.sampled_values[3][0][0], pf.sampled_values[3][1][0], pf.sampled_values[3][2][0], pf.sampled_values[3][3][0]};
  QM31 comp = combine_ef(c4);
  QM31 ppv[air::N_PREPROC];
  for (int i = 0; i < air::N_PREPROC; i++) ppv[i] = pf.sampled_values[0][i][0];
  QM31 sum;
  for (int c = 0; c < air::N_COMPONENTS; c++) {
    const air::ComponentInfo& info = air::component_info(c);
    std::vector<QM31> tr, it;
    for (int k = 0; k < info.n_trace; k++) tr.push_back(pf.sampled_values[1][tr0[c] + k][0]);
    for (int k = 0; k < info.n_interaction; k++) for (auto& s : pf.sampled_values[2][it0[c] + k]) it.push_back(s);
    QM31 shift = pf.claimed_sums[c] * inv(M31::from_u32(1u << clog[c]));
    QM31 num = point_eval(c, tr.data(), it.data(), ppv, hrel, &powers[coff[c]], info.n_base_constraints, shift);
    sum += num * inv(coset_vanishing_canonic<QM31>(clog[c], oods));
  }
  if (sum != comp) throw CmError(10, "ConstraintsNotSatisfied: composition polynomial does not match the constraints at the OODS point");
}
// the OODS point from one drawn felt t: ((1 - t^2) / (1 + t^2), 2t / (1 + t^2))
static CPoint<QM31> draw_oods_point(Channel& ch, QM31* t_out = nullptr) {
  QM31 t = ch.draw_felt();
  if (t_out) *t_out = t;
  QM31 t2 = t * t;
  QM31 iv = inv(t2 + M31(1));
  CPoint<QM31> p;
  p.x = (QM31(M31(1)) - t2) * iv;
  p.y = (t + t) * iv;
  return p;
}
// side streams a fork region spreads its large launches over (A/B: CM_FORK_WIDTH; the join costs one barrier packet per used stream)
static int fork_width(int dflt) {
  const int w = tune(T_FORK_WIDTH);
  return w > 0 && w < dflt ? w : dflt;
}
// =========================================================================================================
// CM_HOST_TRACE=1: host-side time between marks on stderr (where the GPU sits idle waiting for the host)
// (the split of the sampled values, per mille in the chunk evaluated and hashed first: tuning key "oods_split", 780)
struct HostTrace {
  const char* prefix; int width; bool on;
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  HostTrace(const char* prefix_, int width_, const char* env, const char* env2 = nullptr)   // env2 = CM_HOST_MARKS: no synchronising ticks
      : prefix(prefix_), width(width_), on(getenv(env) != nullptr || (env2 && getenv(env2) != nullptr)) {}
  void mark(const char* what) {
    if (!on) return;
    auto n = std::chrono::steady_clock::now();
    fprintf(stderr, "%s %-*s %8.1f us\n", prefix, width, what, std::chrono::duration<double, std::micro>(n - t).count());
    t = n;
  }
};
// (check_pcs_config, ProofContext, mix_claim, channel_words, DrainOnExit: proof_context.hpp)
// One segment proof on one GPU: the phases of prove_cairo_m (prover.rs:23-147) in transcript order.  Each phase enqueues its
// kernels and returns at the next point where the transcript needs a device result; what crosses a phase boundary is a member.
struct SegmentProver : ProofContext {
  HostTrace ht{"[host]", 40, "CM_HOST_TRACE", "CM_HOST_MARKS"};
  struct DtorMark { HostTrace* ht; const char* what; ~DtorMark() { ht->mark(what); } };   // (CM_HOST_MARKS: where the teardown goes)
  DtorMark dm_p{&ht, "~ everything else (P: trees, events)"};
  Prover P;
  DtorMark dm_after_p{&ht, "~ twiddles .. step buffers"};
  hipStream_t st;
  Channel& ch;
  std::vector<int> by_size;                  // launch order of the opcode components: by_size_all without the builtins
  ProofTwiddles own_tw;
  std::unique_ptr<Fork> tw_fork;
  ColumnSet pp_evals, tr_evals;              // preprocessed / execution-trace evaluations (trace domain)
  DevBuf drel;                               // DevRelations
  DevBuf d_powers;                           // `powers` on the device
  DevBuf d_step1;                            // device-side transcript step after tree 1: {root[8], nonce[2], n_sent, error, z0[4]}
  DevBuf d_step2;                            // device-side transcript step after tree 2: {channel[16], coefficient[4], root[8]}
  DevBuf d_ctab;                             // composition: every small table of the constraints phase, ONE upload
  DtorMark dm_q{&ht, "~ oods buffers, quotients"};
  DevBuf d_oods_table, d_oods_out, d_qblob;  // sampling pointer table, sampled values, DEEP-quotient plan
  size_t o_qjobs = 0, n_qjobs = 0;
  std::vector<uint32_t> q_logs;
  std::vector<ColumnSet> quotients;
  DtorMark dm_fri{&ht, "~ fri"};
  FriPhase fri;
  DtorMark dm_rest{&ht, "~ ojobs, qg, affinity"};
  struct ORef { int t; uint32_t c; bool prev; };
  struct OJob { uint32_t log; bool prev; CPoint<QM31> pt; std::vector<ORef> refs; size_t off = 0, out_off = 0; int chunk = 0; };
  std::vector<OJob> ojobs;                    // sampling jobs, built (and their pointer table uploaded) by oods_prepare()
  size_t n_oods_out = 0;
  bool oods_poll = false;                    // the host watches the landing words of the sampled values instead of waiting for an event
  static void cpu_relax() { __builtin_ia32_pause(); }
  size_t n_oods_out0 = 0, n_flat0 = 0;       // sampled values / flat samples of chunk 0 (the part hashed while chunk 1 is evaluated)
  std::vector<QuotientGroup> qg;             // DEEP-quotient size groups (quotient_plan.hpp)
  AffinityScope cpu_scope;   // the calling thread sits next to the GPU for this proof only (pool.hip)
  SegmentProver(const DeviceInput& din_, const cm_pcs_config& cfg_)
      : ProofContext(din_, cfg_), st(nullptr), ch(P.ch) {
    start(P);
    st = P.st;
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

    kprof_close_run();   // a run of timed launches still open on this thread
    ht.mark("finish: entered");
    finish_common(P);
    ht.mark("finish: phase events read, fork/join checked");
    pf.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - P.t0).count();
    if (pp_cache_enabled()) {
      tl_pp_cache.tree = std::move(P.trees[0]);
      tl_pp_cache.evals = std::move(pp_evals);
      tl_pp_cache.log_blowup = cfg.log_blowup_factor;
      tl_pp_cache.valid = true;
    } else if (tl_pp_cache.valid) {
      tl_pp_cache = PreprocessedCache();  // switched off: give the buffers back to the pool
    }
    // Teardown that can wait: the FRI phase alone owns ~500 pool blocks (20 layers x (4 columns + a tree of ~20 layers)) and
    // giving them back took 80-100 us with the GPU idle between two proofs.  They are parked here and released by this thread's
    // NEXT proof while it waits for tree 1 (or when the thread ends); the next FRI phase finds them back in the pool.
    if (defer_teardown()) {
      std::unique_ptr<Parked>& g = parked();
      g.reset(new Parked());
      g->fri = std::move(fri);
      g->qg = std::move(qg);
      g->ojobs = std::move(ojobs);
      g->quotients = std::move(quotients);
    }
    ht.mark("finish: done");
    return out.release();
  }
  struct Parked { FriPhase fri; std::vector<QuotientGroup> qg; std::vector<OJob> ojobs; std::vector<ColumnSet> quotients; };
  static std::unique_ptr<Parked>& parked() {
    static thread_local std::unique_ptr<Parked> g;
    static thread_local bool hooked = false;
    if (!hooked) {   // cm_pool_trim / cm_shutdown / the pool's out-of-memory retry / prove_sharded release it too (pool.hip)
      hooked = true;
      set_thread_parked_release([] { parked().reset(); });
    }
    return g;
  }
  static bool defer_teardown() { return tune(T_DEFER_TEARDOWN) != 0; }

  // component sizes, twiddles (side stream), transcript setup (prover.rs:33-66)
  void setup() {
    size_components();
    column_offsets();
    for (int c : by_size_all) if (c < air::N_OPCODE_COMPONENTS) by_size.push_back(c);
    if (tw_cache_enabled()) P.tw = cached_twiddles(comp_log + cfg.log_blowup_factor, st);
    else {
      tw_fork.reset(new Fork(st));
      own_tw.build(comp_log + cfg.log_blowup_factor, tw_fork->stream(Fork::N - 1));   // joined before the first transform
      P.tw = &own_tw.t;
    }

    // ---- transcript setup (prover.rs:33-36, 62-66) ----
    pf.public_data = din.public_data;
    mix_config_and_public_data(ch, cfg, pf.public_data);
    ht.mark("setup");
    P.tick("setup");

  }

  // tree 0 (preprocessed, on a side stream) and tree 1: execution trace of every component + commitment (prover.rs:70-82)
  void trace_commit() {
    // ---- tree 0: preprocessed trace (prover.rs:70-73) ----
    std::unique_ptr<Fork> pp_fork;
    hipStream_t tree0_stream = nullptr;
    DrainOnExit tree0_guard;   // an exception between the fork and the join must not return tree 0's buffers to the pool under its kernels
    bool build_tree0 = false;
    if (pp_cache_enabled() && tl_pp_cache.valid && tl_pp_cache.log_blowup == cfg.log_blowup_factor) {
      P.trees[0] = std::move(tl_pp_cache.tree);  // both handed back at the end of the proof
      pp_evals = std::move(tl_pp_cache.evals);
      tl_pp_cache.valid = false;
      ch.mix_root(P.trees[0].root);
    } else {
      std::vector<uint32_t> logs(air::PREPROC_LOG, air::PREPROC_LOG + air::N_PREPROC);
      pp_evals.alloc(logs, st);
      // The constant columns are generated on the side stream that builds the twiddles and later commits tree 0 (the same HIP
      // stream: ordered behind one, in front of the other): nothing before the LogUp phase reads them on the main stream, which
      // starts trace generation ~150 us earlier this way.  cm_set_tuning("pp_side", 0) / CM_PP_SIDE=0: on the main stream (A/B).
      const bool pp_side = tune(T_PP_SIDE) != 0;
      hipStream_t pps = st;
      if (pp_side) {
        if (!tw_fork) tw_fork.reset(new Fork(st));   // (twiddle cache on: nothing else is on that stream yet)
        pps = tw_fork->stream(Fork::N - 1);
      }
      launch_preproc_all(pp_evals.ptrs.data(), pps);
      build_tree0 = true;   // enqueued on a side stream right after the trace-generation launches (below)
    }
    ht.mark("preprocessed enqueued");
    P.tick("preprocessed");
    ht.mark("preprocessed gpu done");

    // ---- tree 1: execution trace (prover.rs:77-82; Claim::write_trace) ----
    tr_evals.alloc(tr_logs, st);
    DevBuf flag(4);   // range-check / bitwise lookup out of range: read back with the tree-1 root (no round trip of its own)
    uint32_t* flag_host = pinned_words();
    {
      // multiplicity columns = histograms over every lookup of every opcode component (components/mod.rs:139-160)
      CM_HIP(hipMemsetAsync(flag.p, 0, 4, st));
      HistPtrs h;
      h.rc8 = tr_evals.ptrs[tr0[air::C_RC8]]; h.rc16 = tr_evals.ptrs[tr0[air::C_RC16]];
      h.rc20 = tr_evals.ptrs[tr0[air::C_RC20]]; h.bitwise = tr_evals.ptrs[tr0[air::C_BITWISE]];
      h.error_flag = flag.u32();
      if (h.rc16 == h.rc8 + (1u << 8) && h.rc20 == h.rc16 + (1u << 16) && h.bitwise == h.rc20 + (1u << 20)) {
        // the four multiplicity columns are adjacent in the trace arena: one memset
        CM_HIP(hipMemsetAsync(h.rc8, 0, 4 * ((size_t)(1u << 8) + (1u << 16) + (1u << 20) + (1u << 18)), st));
      } else {
        CM_HIP(hipMemsetAsync(h.rc8, 0, 4u << 8, st));
        CM_HIP(hipMemsetAsync(h.rc16, 0, 4u << 16, st));
        CM_HIP(hipMemsetAsync(h.rc20, 0, 4u << 20, st));
        CM_HIP(hipMemsetAsync(h.bitwise, 0, 4u << 18, st));
      }
      // small opcode components (idle ones are 16 padding rows): trace + histogram of all of them in ONE launch
      std::vector<SmallTraceJob> small_trace;
      for (int c = 0; c < air::N_OPCODE_COMPONENTS; c++)
        if (clog[c] <= SMALL_COMPONENT_MAX_LOG && !no_small_batch())
          small_trace.push_back(SmallTraceJob{din.bundles[c].p, (uint32_t)in.n_bundles[c], tr_evals.dev(tr0[c]), clog[c], c});
      DevBuf d_small_trace = upload(small_trace, st);
      // components are independent: fork over side streams (trace then histogram of one component stay ordered)
      KProfRegion kreg("k_trace_gen(region)", st);
      Fork fk(st);
      // large components first: their kernels keep the GPU busy while the host issues the ~40 launches of the idle
      // ones (the host launch rate, not the GPU, bounds this region otherwise); histogram adds commute
      // the batched small components first: ~100 us of pure latency on a handful of CUs, hidden under the large kernels
      // (launched last it ran alone at the end of the region)
      launch_trace_hist_small(d_small_trace.as<SmallTraceJob>(), (uint32_t)small_trace.size(), din.data_accesses.p, h, fk.stream(Fork::N - 2));
      int spos = 0;
      for (int pos = 0; pos < air::N_OPCODE_COMPONENTS; pos++) {
        const int c = by_size[pos];
        if (clog[c] <= SMALL_COMPONENT_MAX_LOG && !no_small_batch()) continue;
        hipStream_t sc = fk.stream(spos == 0 ? Fork::main_or(0) : spos % fork_width(Fork::N - 2));   // by_size: the first one is the largest
        spos++;
        const bool fuse_th = tune(T_TRACE_HIST_FUSE) != 0;   // A/B
        if (fuse_th) launch_opcode_trace_hist(c, din.bundles[c].p, (uint32_t)in.n_bundles[c], din.data_accesses.p, clog[c], tr_evals.dev(tr0[c]), h, sc);
        else {
          launch_opcode_trace(c, din.bundles[c].p, (uint32_t)in.n_bundles[c], din.data_accesses.p, clog[c], tr_evals.dev(tr0[c]), sc);
          launch_hist(c, (const uint32_t* const*)tr_evals.dev(tr0[c]), clog[c], h, sc);
        }
      }
      launch_memory_trace(din.init_mem.p, (uint32_t)in.n_initial_memory, din.fin_mem.p, (uint32_t)in.n_final_memory, in.initial_root,
                          in.final_root, clog[air::C_MEMORY], tr_evals.dev(tr0[air::C_MEMORY]), fk.stream(air::C_MEMORY));
      launch_merkle_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree, in.initial_root,
                          in.final_root, clog[air::C_MERKLE], tr_evals.dev(tr0[air::C_MERKLE]), fk.stream(air::C_MERKLE));
      launch_clock_update_trace(din.clock_updates.p, (uint32_t)in.n_clock_updates, clog[air::C_CLOCK_UPDATE],
                                tr_evals.dev(tr0[air::C_CLOCK_UPDATE]), fk.stream(air::C_CLOCK_UPDATE));
      launch_poseidon2_trace(din.init_tree.p, (uint32_t)in.n_initial_tree, din.fin_tree.p, (uint32_t)in.n_final_tree,
                             clog[air::C_POSEIDON2], tr_evals.dev(tr0[air::C_POSEIDON2]), fk.stream(air::C_POSEIDON2));
      fk.join();
      kreg.close();
      ht.mark("trace_gen: launched + joined");
      flag_host[0] = 0xffffffffu;
      CM_HIP(hipMemcpyAsync(flag_host, flag.p, 4, hipMemcpyDeviceToHost, st));
    }
    if (tw_fork) tw_fork->join();   // the proof's twiddle tables are complete from here on
    if (build_tree0) {
      // tree 0 (a chain of ~30 small launches) is built on a side stream while the transforms and hashes of tree 1 keep
      // the GPU busy; its root comes back together with the root of tree 1.  Forked from the stream position after the
      // trace-generation launches so that its chain does not queue in front of them.
      // The side streams share four hardware queues with the main and the pipeline stream, and a queue runs its packets in order:
      // on side stream 7 the whole tree sat BEHIND the transforms of tree 1 (same queue as the pipeline stream) and its Merkle
      // chain ran alone after tree 1 had finished (0.17 ms of a nearly idle GPU, and the host learnt root 0 only then).  A stream
      // of the highest priority class has hardware queues of its own.  CM_TREE0_PRIO=0: the side stream (A/B), 1: lowest class.
      // A lone proof only: with several proofs in flight (cm_prove_many) the other proofs' kernels fill the queues anyway, and
      // four high-priority chains cutting into them cost 0.5-1 ms per proof (9.6 -> 10.1-10.8 with four in flight).
      const int t0_prio = tune(T_TREE0_PRIO);
      if (t0_prio != 0 && g_proofs_in_flight.load(std::memory_order_relaxed) <= 1) {
        tree0_guard.s = tree0_stream = thread_priority_stream(t0_prio);
        hipEvent_t e = Prover::pipe_event();
        CM_HIP(hipEventRecord(e, st));                       // trace generation launched, twiddles joined
        CM_HIP(hipStreamWaitEvent(tree0_stream, e, 0));
      } else {
        pp_fork.reset(new Fork(st));
        tree0_guard.s = tree0_stream = pp_fork->stream(Fork::N - 1);   // the side stream waits for THIS point of the main stream (trace generation done)
      }
    }
    P.tick("trace_gen");
    // tree 1 first: its large transforms start as soon as the trace exists and keep the GPU busy while the host issues tree 0's
    // chain of small launches (enqueued first, that chain delayed the first tree-1 kernel by the host time of ~30 launches)
    const bool tree1_first = tune(T_TREE1_FIRST) != 0;   // A/B switch
    if (build_tree0 && !tree1_first && !(tune(T_TREE0_GUEST) != 0 && !pp_cache_enabled())) P.commit_enqueue(P.trees[0], &pp_evals, false, tree0_stream);
    P.trees[1].merkle.pace_ev = Prover::pace_event(1);
    // (round 6) "tree0_guest": the seven preprocessed columns ride in tree 1's size-group launches (Prover::GuestTree) and only tree 0's
    // Merkle launches run on its stream.  Not with the preprocessed cache on: a cached tree must own its device tables.
    const bool tree0_guest = build_tree0 && tune(T_TREE0_GUEST) != 0 && !pp_cache_enabled();
    {
      Prover::GuestTree guest{&P.trees[0], &pp_evals, tree0_stream};
      Prover::CommitPrep cp1 = P.commit_prepare(P.trees[1], &tr_evals, false, st, true, false, P.pipe_stream(), nullptr, tree0_guest ? &guest : nullptr);
      ht.mark("trace_commit: tree 1 prepared");
      P.commit_launch(cp1);
      ht.mark("trace_commit: tree 1 launched");
    }
    if (build_tree0 && tree1_first && !tree0_guest) P.commit_enqueue(P.trees[0], &pp_evals, false, tree0_stream);
    ht.mark("trace_commit: tree 0 enqueued");
    // Root 0 first (transcript order, prover.rs:70-82: root 0, claim, root 1): tree 0 has been running on its side stream next
    // to all of the above; its root is copied on THAT stream and waited for here, while the GPU is still busy with tree 1.
    if (build_tree0) {
      static thread_local hipEvent_t ev_root0 = nullptr;
      if (!ev_root0) { CM_HIP(hipEventCreateWithFlags(&ev_root0, hipEventDisableTiming)); thread_event_owned(ev_root0); }
      hipStream_t ps = tree0_stream;
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_ROOT0, P.trees[0].merkle.layers[0].p, 32, hipMemcpyDeviceToHost, ps));
      CM_HIP(hipEventRecord(ev_root0, ps));
      if (pp_fork) pp_fork->join();
      else CM_HIP(hipStreamWaitEvent(st, ev_root0, 0));   // what follows on the main stream reads tree 0's LDE
      tree0_guard.joined = true;
      CM_HIP(hipEventSynchronize(ev_root0));
      ht.mark("trace_commit: root 0 arrived");
      memcpy(P.trees[0].root.data(), pinned_words() + PIN_ROOT0, 32);
      ch.mix_root(P.trees[0].root);
    }
    mix_claim(ch, pf, clog);
    // Everything from root 1 to the relation challenges happens on the device, right behind the tree (k_step_pow_relations:
    // mix_root, interaction proof of work, mix_u64(nonce), Relations::draw + alpha powers): the LogUp kernels start without a
    // host round trip.  The host replays the steps from the copied-back root / nonce when it waits for the claimed sums.
    {
      static_assert(sizeof(DevRelations) == 4 * 4 * (air::N_RELATIONS + air::N_RELATIONS * air::MAX_REL_SIZE), "DevRelations layout");
      uint32_t cw[9];
      channel_words(ch, cw);
      drel.alloc(sizeof(DevRelations));
      d_step1.alloc(16 * 4);
      uint32_t* rel = drel.u32();
      step_pow_relations(cw, P.trees[1].merkle.layers[0].u32(), INTERACTION_POW_BITS, air::N_RELATIONS, air::MAX_REL_SIZE, rel,
                         rel + 4 * air::N_RELATIONS, d_step1.u32(), st);
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_STEP1, d_step1.p, 16 * 4, hipMemcpyDeviceToHost, st));
      ht.mark("trace_commit: enqueued");
      parked().reset();   // the previous proof's parked teardown: the host is about to wait ~0.9 ms anyway
      ht.mark("trace_commit: previous proof's teardown");
      P.pace(&P.trees[1].merkle);
      ht.mark("trace_commit: paced (tree 1 at its top)");
    }
    P.tick("trace_commit");

  }

  // interaction PoW, relation draws, tree 2: LogUp columns + commitment enqueue, claimed sums (prover.rs:90-102)
  void interaction() {
    // ---- tree 2: interaction trace (prover.rs:96-102) ----
    hipEvent_t sums_ready = nullptr;
    ColumnSet it_evals;
    // The LogUp tail (claimed sums, the running-sum columns' prefix scans: ~0.15 ms of short memory-bound kernels) runs on a side
    // stream while the tree-2 transforms of every OTHER column start; the running-sum columns go last in their size group.
    // CM_LOGUP_DEFER=0: the tail on the main stream in front of the tree (the round-3 order).
    const bool defer_tail = tune(T_LOGUP_DEFER) != 0;
    std::vector<DevBuf> tail_scratch;   // alive until the host has seen the sums
    Prover::DeferredCols late;
    Prover::CommitPrep tree2_prep;
    bool tree2_prepared = false;
    ht.mark("interaction: entered");
    it_evals.alloc(it_logs, st);
    ht.mark("interaction: columns allocated");
    {
      tail_scratch.emplace_back(air::N_COMPONENTS * 16);
      uint32_t* const d_sums = tail_scratch.back().u32();
      std::vector<LogupTailJob> jobs(air::N_COMPONENTS);
      // small components (idle opcode components = 16 padding rows, the tiny builtins): ONE launch for all of them
      std::vector<SmallLogupJob> small_jobs;
      uint32_t small_max_log = 0;
      for (int c = 0; c < air::N_COMPONENTS; c++)
        if (clog[c] <= SMALL_COMPONENT_MAX_LOG && !no_small_batch()) {
          small_jobs.push_back(SmallLogupJob{(const uint32_t* const*)tr_evals.dev(tr0[c]), it_evals.dev(it0[c]), clog[c], c});
          small_max_log = std::max(small_max_log, clog[c]);
        }
      DevBuf d_small = upload(small_jobs, st);
      ht.mark("interaction: small jobs uploaded");
      KProfRegion kreg("k_logup(region)", st);
      Fork fk(st);
      // Side streams of this region: every stream the join waits on is one barrier packet at the head of the main queue, ~5.5 us
      // each even when its event has long fired (tools/join_lab.hip: 15 us for three, 42-49 us for seven).  The ~15 LogUp kernels
      // lose nothing on five streams (interaction_gen + interaction_commit 2.66 -> 2.61 ms, profiles/r04n_ab_logup_width.txt); the
      // constraint and quotient regions do (1.0 -> 1.3 ms with four) and keep all eight.  CM_LOGUP_WIDTH: side streams used here.
      const int lw = std::max(1, std::min(tune(T_LOGUP_WIDTH), Fork::N - 1));
      // (which side stream: the streams share a few hardware queues and a queue runs its packets in order — on the stream that
      // shares the MAIN stream's queue this ~90 us latency-bound launch sat in front of the region's largest kernel, round-5
      // timeline.  "logup_small_stream" >= 0 picks the stream, -1 = stream `lw`.)
      const int lss = tune(T_LOGUP_SMALL_STREAM);
      launch_logup_small(d_small.as<SmallLogupJob>(), (uint32_t)small_jobs.size(), small_max_log, (const uint32_t* const*)pp_evals.dev(),
                         drel.as<DevRelations>(), fk.stream(lss >= 0 ? lss : lw));   // first: latency-bound, hidden under the large kernels
      int spos = 0;
      for (int pos = 0; pos < air::N_COMPONENTS; pos++) {   // large components first (see trace generation)
        const int c = by_size_all[pos];
        const air::ComponentInfo& info = air::component_info(c);
        for (int k = 0; k < 4; k++) jobs[c].col[k] = it_evals.ptrs[it0[c] + info.n_interaction - 4 + k];
        jobs[c].log_size = clog[c];
        if (clog[c] <= SMALL_COMPONENT_MAX_LOG && !no_small_batch()) continue;
        launch_logup(c, (const uint32_t* const*)tr_evals.dev(tr0[c]), (const uint32_t* const*)pp_evals.dev(), clog[c],
                     drel.as<DevRelations>(), it_evals.dev(it0[c]), fk.stream(spos == 0 ? Fork::main_or(0) : spos % lw));
        spos++;
      }
      // Tree 2's host-side preparation (size groups, pointer tables, layer buffers, launch plan: ~0.1 ms for 1036 columns) HERE,
      // while the LogUp kernels just launched execute — it used to sit between the LogUp tail and the first transform with the
      // GPU idle (50 us in the round-5 timeline).  Its one host->device copy lands on the main stream behind the region's
      // largest kernel.  CM_COMMIT_PREP_EARLY=0: prepared at the launch (A/B).
      const bool prep_early = tune(T_COMMIT_PREP_EARLY) != 0;
      if (defer_tail) {
        late.late.assign(it_evals.ptrs.size(), 0);
        for (int c = 0; c < air::N_COMPONENTS; c++)
          for (int k = 0; k < 4; k++) late.late[it0[c] + air::component_info(c).n_interaction - 4 + k] = 1;
      }
      if (prep_early) {
        CommittedTree& t = P.trees[2];
        t.coeffs = std::move(it_evals);   // (the kernels above hold the column pointers; the arena just changes its owner)
        t.merkle.pace_ev = Prover::pace_event(2);
        tree2_prep = P.commit_prepare(t, nullptr, true, st, true, /*evals_in_place=*/true, P.pipe_stream(), defer_tail ? &late : nullptr);
        tree2_prepared = true;
      }
      fk.join();
      kreg.close();
      ht.mark("interaction: logup launched + joined");
      hipStream_t sf = st;
      if (defer_tail) {
        sf = thread_side_stream(1);   // (side stream 0 is the pipeline's transform stream)
        hipEvent_t e = Prover::pipe_event();
        CM_HIP(hipEventRecord(e, st));
        CM_HIP(hipStreamWaitEvent(sf, e, 0));
      }
      logup_finalize_all(jobs, d_sums, sf, defer_tail ? &tail_scratch : nullptr);
      static_assert(PIN_SUMS + air::N_COMPONENTS * 4 <= PIN_COEFF, "pinned slot layout");
      const uint32_t* sums = pinned_words() + PIN_SUMS;
      CM_HIP(hipMemcpyAsync((void*)sums, d_sums, air::N_COMPONENTS * 16, hipMemcpyDeviceToHost, sf));
      // the host only waits for THIS copy (an event), after the tree-2 transforms and hashes have been enqueued behind it:
      // no GPU idle time while the host reads and mixes the 34 sums
      static thread_local hipEvent_t ev_sums = nullptr;
      CM_HIP(hipEventRecord(thread_event(ev_sums), sf));
      sums_ready = ev_sums;
      late.ready = ev_sums;
    }
    ht.mark("interaction: tail enqueued");
    P.tick("interaction_gen");
    // interpolate in place: coeffs alias the evaluation buffer (every size group right in front of its extension)
    if (tree2_prepared) P.commit_launch(tree2_prep);
    else {
      CommittedTree& t = P.trees[2];
      t.coeffs = std::move(it_evals);
      t.merkle.pace_ev = Prover::pace_event(2);
      P.commit_enqueue(t, nullptr, true, st, true, /*evals_in_place=*/true, P.pipe_stream(), defer_tail ? &late : nullptr);
    }
    ht.mark("interaction: tree 2 enqueued");
    {
      CM_HIP(hipEventSynchronize(sums_ready));
      tail_scratch.clear();
      // host replay of the device-side step behind tree 1 (its results were copied back in front of the sums)
      {
        const uint32_t* s1 = pinned_words() + PIN_STEP1;
        CM_CHECK(pinned_words()[PIN_FLAG] == 0, "trace generation: a range-check / bitwise lookup value is out of range");
        memcpy(P.trees[1].root.data(), s1, 32);
        ch.mix_root(P.trees[1].root);
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
      const uint32_t* sums = pinned_words() + PIN_SUMS;
      for (int c = 0; c < air::N_COMPONENTS; c++) pf.claimed_sums.push_back(QM31::from_u32(sums + 4 * c));
      for (auto& cs : pf.claimed_sums) ch.mix_felts(&cs, 1);
    }
    tr_evals.buf.release();
  }

  // stwo prove: constraint quotients of all components -> composition polynomial, tree 3 enqueued
  void composition() {
    // ---- stwo prove: composition polynomial.  Everything that does not depend on the random coefficient (accumulators,
    // slots, per-component arguments, their uploads and memsets) is prepared and enqueued here, behind the tree-2 kernels;
    // the root is read back, the coefficient drawn and its powers uploaded right before the launches. ----
    const size_t total_constraints = powers.size();
    d_powers.alloc(16 * total_constraints);
    // the accumulators of every evaluation log (constraint_plan.hpp): pointer tables in the phase's one upload below, zeroing in
    // one launch together with the slot buffer
    ConstraintAccumulators acc;
    acc.plan(clog, comp_log, [](int) { return true; });
    CM_CHECK(acc.cgroups.count(comp_log), "composition polynomial log size mismatch");
    acc.alloc(st, /*upload_ptrs=*/false, /*top_contiguous=*/false);
    const std::map<uint32_t, std::vector<int>>& cgroups = acc.cgroups;
    ColumnSet &acc_top = acc.top, &acc_rest = acc.rest;
    CM_CHECK(cfg.log_blowup_factor >= 1 && cfg.log_blowup_factor <= 4, "PcsConfig: log_blowup_factor must be in 1..4");
    ColumnSet cdom[3];   // evaluation-domain copies of trees 0..2 (only when log_blowup_factor > 1)
    if (cfg.log_blowup_factor > 1) {
      const ColumnSet* const src[3] = {&P.trees[0].coeffs, &P.trees[1].coeffs, &P.trees[2].coeffs};
      eval_domain_copies(cdom, src, *P.tw, st);
    }
    auto cdom_cols = [&](int t, size_t first) -> const uint32_t* const* {
      return (const uint32_t* const*)(cfg.log_blowup_factor > 1 ? cdom[t].dev(first) : P.trees[t].lde.dev(first));
    };
    {
      // Components are independent except for the shared per-size accumulator.  Small sizes (many idle
      // components of 2^4 rows, each a latency-bound launch) get a private zeroed accumulator slot per
      // component and run concurrently on side streams; the slots are summed afterwards (field addition is
      // exact, so the order is irrelevant).  Large sizes keep the shared accumulator and one stream per size.
      constexpr uint32_t SLOT_MAX_LOG = 15;
      struct SlotGroup { uint32_t el; uint32_t n; size_t off_words; size_t tab0; };
      std::vector<SlotGroup> sgroups;
      std::vector<int> slot_of(air::N_COMPONENTS, -1);
      std::vector<uint32_t*> slot_tab;
      size_t slot_words = 0;
      for (auto& kv : cgroups)
        if (kv.second.size() > 1 && kv.first <= SLOT_MAX_LOG) {
          SlotGroup g{kv.first, (uint32_t)kv.second.size(), slot_words, slot_tab.size()};
          for (size_t k = 0; k < kv.second.size(); k++) slot_of[kv.second[k]] = (int)(slot_tab.size() / 4 + k);
          slot_tab.resize(slot_tab.size() + 4 * kv.second.size());
          slot_words += (size_t)4 * kv.second.size() << kv.first;
          sgroups.push_back(g);
        }
      DevBuf slots(((slot_words * 4 + 15) & ~(size_t)15) + 16);
      if (slot_words)
        for (auto& g : sgroups)
          for (uint32_t k = 0; k < 4 * g.n; k++) slot_tab[g.tab0 + k] = slots.u32() + g.off_words + ((size_t)k << g.el);
      acc.zero(slots.p, slot_words, st);
      // ONE device table for the phase: [acc_top pointers | acc_rest pointers | slot table | small-component arguments | their ids];
      // its address is known before the arguments (which point into it) are built
      const size_t o_top = 0, o_rest = 64, o_slot = (o_rest + acc_rest.ptrs.size() * sizeof(void*) + 15) & ~(size_t)15;
      const size_t o_args = (o_slot + slot_tab.size() * sizeof(void*) + 15) & ~(size_t)15;
      const size_t o_cids = o_args + air::N_COMPONENTS * sizeof(ConstraintArgs);
      d_ctab.alloc(o_cids + air::N_COMPONENTS * sizeof(int) + 16);
      uint8_t* const ctab = d_ctab.as<uint8_t>();
      acc_top.d_view = (uint32_t**)(ctab + o_top);
      acc_rest.d_view = (uint32_t**)(ctab + o_rest);
      uint32_t** const d_slot_tab = (uint32_t**)(ctab + o_slot);
      // arguments of every component first: the small ones (<= 2^SMALL_COMPONENT_MAX_LOG rows) go to ONE batched launch
      // whose argument array has to be uploaded before the fork
      std::vector<ConstraintArgs> cargs(air::N_COMPONENTS);
      std::vector<ConstraintArgs> small_args;
      std::vector<int> small_cids;
      uint32_t small_max_log = 0;
      for (auto it = cgroups.rbegin(); it != cgroups.rend(); ++it) {
        for (int c : it->second) {
          ConstraintArgs& a = cargs[c];
          a.tr = cdom_cols(1, tr0[c]);
          a.it = cdom_cols(2, it0[c]);
          a.pp = cdom_cols(0, 0);
          a.acc = slot_of[c] >= 0 ? d_slot_tab + 4 * slot_of[c] : acc.of(it->first);
          fill_constraint_args(a, c, clog[c], pf.claimed_sums[c], drel.as<DevRelations>(), d_powers.u32() + 4 * coff[c]);
          // a small component either owns a private slot or is alone in its size group: no accumulator is shared inside the batch
          if (clog[c] <= SMALL_COMPONENT_MAX_LOG && !no_small_batch() && (slot_of[c] >= 0 || it->second.size() == 1)) {
            small_args.push_back(a);
            small_cids.push_back(c);
            small_max_log = std::max(small_max_log, clog[c]);
          }
        }
      }
      {
        std::vector<uint8_t> blob(o_cids + small_cids.size() * sizeof(int));
        memcpy(blob.data() + o_top, acc_top.ptrs.data(), acc_top.ptrs.size() * sizeof(void*));
        if (!acc_rest.ptrs.empty()) memcpy(blob.data() + o_rest, acc_rest.ptrs.data(), acc_rest.ptrs.size() * sizeof(void*));
        if (!slot_tab.empty()) memcpy(blob.data() + o_slot, slot_tab.data(), slot_tab.size() * sizeof(void*));
        if (!small_args.empty()) memcpy(blob.data() + o_args, small_args.data(), small_args.size() * sizeof(ConstraintArgs));
        if (!small_cids.empty()) memcpy(blob.data() + o_cids, small_cids.data(), small_cids.size() * sizeof(int));
        stage_upload(d_ctab.p, blob.data(), blob.size(), st);
      }
      const ConstraintArgs* const d_small_args = (const ConstraintArgs*)(ctab + o_args);
      const int* const d_small_cids = (const int*)(ctab + o_cids);
      // Transcript step on the device (prover.rs:131, stwo prove: mix the interaction root, draw the random coefficient): the
      // channel state goes over in the kernel arguments, k_chan_init_mix_root_draw mixes root 2 and draws the coefficient,
      // k_coeff_powers expands its powers — the constraint kernels start right behind the tree, with no host round trip.  The
      // host replays both steps on its own channel when root 3 comes back (oods_sampling) and checks the coefficients agree.
      {
        uint32_t cw[9];
        channel_words(ch, cw);
        d_step2.alloc(4 * (16 + 4 + 8));
        uint32_t* d_chan = d_step2.u32();
        chan_init_mix_root_draw(cw, d_chan, P.trees[2].merkle.layers[0].u32(), d_chan + 16, d_chan + 20, st);
        coeff_powers(d_chan + 16, d_powers.u32(), (uint32_t)total_constraints, st);
        static_assert(PIN_COEFF + 4 == PIN_ROOT2, "{coefficient, root 2} come back in one copy");
        CM_HIP(hipMemcpyAsync(pinned_words() + PIN_COEFF, d_chan + 16, 48, hipMemcpyDeviceToHost, st));
      }
      P.tick("interaction_commit");
      for (int t = 0; t < 3; t++) for (auto l : P.trees[t].coeffs.logs) pf.cells += 1ull << l;
      P.pace(&P.trees[2].merkle);
      KProfRegion kreg("k_constraints(region)", st);
      Fork fk(st);
      // side-stream plan of the region (A/B: tuning key "cons_plan" = g0,g1,g2,g3,small,slot0,slot1,slot2 = stream index of the size
      // groups in descending size, of the batched small components and of the slotted ones)
      // ("cons_plan": eight octal digits, default 01237456 = streams {0,1,2,3 | 7 | 4,5,6})
      std::vector<int> cplan(8);
      {
        const int code = tune(T_CONS_PLAN);
        for (int k = 0; k < 8; k++) cplan[k] = (code >> (3 * (7 - k))) & 7;
      }
      launch_constraints_small(d_small_args, d_small_cids, (uint32_t)small_args.size(), small_max_log,
                               fk.stream(cplan[4]));   // first: latency-bound, hidden under the large kernels
      ht.mark("constraints: small batch launched");
      int gi = 0, small_rr = 0;
      static const bool early_interp = getenv("CM_NO_EARLY_ACC_INTERP") == nullptr;   // A/B switch
      // the wide component of few rows first (round-5 timeline: 5570 -> 5905 us of a region that the large groups had left at ~5720)
      auto is_wide = [&](int c) { return is_wide_component(c, clog); };
      std::vector<hipStream_t> cstream(air::N_COMPONENTS, nullptr);
      for (auto it = cgroups.rbegin(); it != cgroups.rend(); ++it, ++gi)
        for (int c : it->second) {
          if (std::find(small_cids.begin(), small_cids.end(), c) != small_cids.end()) continue;
          // the components of a size group share its accumulator: one stream for all of them; slotted ones are independent
          cstream[c] = slot_of[c] >= 0 ? fk.stream(cplan[5 + (small_rr++ % 3)]) : fk.stream(gi == 0 ? Fork::main_or(cplan[0]) : cplan[gi % 4]);
          if (is_wide(c)) launch_constraints(c, cargs[c], cstream[c]);
        }
      gi = 0;
      // large groups first (descending size) so the long kernels start early
      for (auto it = cgroups.rbegin(); it != cgroups.rend(); ++it, ++gi) {
        bool one_stream = true;   // every component of the group ran on the group's stream (no slots, no batched small ones)
        for (int c : it->second) {
          if (std::find(small_cids.begin(), small_cids.end(), c) != small_cids.end()) { one_stream = false; continue; }
          if (slot_of[c] >= 0) one_stream = false;
          if (!is_wide(c)) launch_constraints(c, cargs[c], cstream[c]);
        }
        // DomainEvaluationAccumulator::finalize starts here for such a group: its accumulator is interpolated on the same
        // stream right behind its constraint kernels — no second fork/join region for the large accumulators
        if (one_stream && early_interp) {
          interpolate(acc.of(it->first), 4, it->first, *P.tw, fk.stream(gi == 0 ? Fork::main_or(cplan[0]) : cplan[gi % 4]));
          acc.interpolated.insert(it->first);
        }
        ht.mark("constraints: size group launched");
      }
      fk.join();
      kreg.close();
      for (auto& g : sgroups) sum_slots(acc.of(g.el), slots.u32() + g.off_words, g.n, g.el, st);
    }
    P.tick("constraints");
    // DomainEvaluationAccumulator::finalize (constraint_plan.hpp)
    {
      CommittedTree& t = P.trees[3];
      if (acc.interpolated.empty()) {   // nothing interpolated inside the region (CM_NO_EARLY_ACC_INTERP): every size on a side stream of its own
        Fork fk(st);
        int k = 0;
        for (auto it = cgroups.rbegin(); it != cgroups.rend(); ++it, ++k) {
          interpolate(acc.of(it->first), 4, it->first, *P.tw, fk.stream(k));
          acc.interpolated.insert(it->first);
        }
        fk.join();
      }
      finalize_accumulators(acc, *P.tw, st);
      t.coeffs = std::move(acc_top);
      oods_prepare();   // needs tree 3's coefficient pointers, nothing of its commitment
      KProfAloneScope kprof_alone_scope;   // (measurement only: the composition tree has the GPU to itself, kprof.hpp)
      P.commit_enqueue(t, nullptr, true, st, true, false, P.pipe_stream());
    }
  }

  // Sampling jobs = (log size, point): every column at the OODS point, plus the previous-row mask
  // (oods - trace_step(log)) of each component's last LogUp column group.  All jobs share one pointer-table
  // upload, one scratch buffer and ONE device->host copy of the results.  Everything but the points themselves is
  // built and uploaded HERE, in front of the composition tree's kernels in stream order (called by composition() right
  // before that tree is enqueued): the table's host->device copy is off the path root 3 -> evaluation kernels.
  void oods_prepare() {
    ojobs.clear();
    n_oods_out = 0;
    {
      // Two chunks in the transcript's flat order (tree, column, mask): the sampled values of chunk 0 come back first and the
      // host hashes them (channel.mix_felts, ~0.1 ms of sequential Blake2s over ~30 KB) while the GPU evaluates chunk 1 — the
      // split makes the two take about as long (CM_OODS_SPLIT: per mille of the samples in chunk 0; 1000 = one chunk)
      const uint32_t split_pm = (uint32_t)tune(T_OODS_SPLIT);
      std::vector<std::vector<char>> has_prev(4);
      size_t total = 0;
      for (int t = 0; t < 4; t++) { has_prev[t].assign(P.trees[t].coeffs.size(), 0); total += P.trees[t].coeffs.size(); }
      for (int c = 0; c < air::N_COMPONENTS; c++) {
        const int ni = air::component_info(c).n_interaction;
        for (int k = ni - 4; k < ni; k++) { has_prev[2][it0[c] + k] = 1; total++; }
      }
      const size_t split = split_pm >= 1000 ? total : total * split_pm / 1000;
      std::map<std::tuple<int, bool, uint32_t>, std::vector<ORef>> groups;   // (chunk, previous-row mask, log size)
      size_t cum = 0;
      n_flat0 = 0;
      for (int t = 0; t < 4; t++)
        for (uint32_t c = 0; c < P.trees[t].coeffs.size(); c++) {
          const int chunk = cum < split ? 0 : 1;
          const uint32_t log = P.trees[t].coeffs.logs[c];
          if (has_prev[t][c]) groups[{chunk, true, log}].push_back({t, c, true});
          groups[{chunk, false, log}].push_back({t, c, false});
          cum += has_prev[t][c] ? 2 : 1;
          if (chunk == 0) n_flat0 = cum;
        }
      for (auto& kv : groups) {
        OJob j{std::get<2>(kv.first), std::get<1>(kv.first), {}, kv.second};
        j.chunk = std::get<0>(kv.first);
        ojobs.push_back(std::move(j));
      }
    }
    {
      std::vector<const uint32_t*> table;
      for (auto& j : ojobs) {
        j.off = table.size();
        j.out_off = n_oods_out;
        for (auto& r : j.refs) table.push_back(P.trees[r.t].coeffs.ptrs[r.c]);
        n_oods_out += j.refs.size();
        if (j.chunk == 0) n_oods_out0 = n_oods_out;
      }
      d_oods_table = upload(table, st);
      d_oods_out.alloc(n_oods_out * 16);
    }
  }

  // OODS point, mask values of every column (eval_at_point), DEEP-quotient plan built while the kernels run
  void oods_sampling() {
    // where the sampled value of (tree, column) lands in d_oods_out: the DEEP-quotient coefficients are computed on the
    // device straight from there (k_quotient_coeffs)
    std::vector<std::vector<uint32_t>> sidx_cur(4), sidx_prev(4);
    for (int t = 0; t < 4; t++) { sidx_cur[t].assign(P.trees[t].coeffs.size(), 0); sidx_prev[t].assign(P.trees[t].coeffs.size(), 0); }
    for (auto& j : ojobs)
      for (size_t i = 0; i < j.refs.size(); i++)
        (j.refs[i].prev ? sidx_prev : sidx_cur)[j.refs[i].t][j.refs[i].c] = (uint32_t)(j.out_off + i);
    pf.sampled_values.resize(4);
    for (int t = 0; t < 4; t++) pf.sampled_values[t].resize(P.trees[t].coeffs.size());
    // Device-side OODS step (A/B: CM_HOST_OODS=1 restores the host form): the channel state after the coefficient draw is still
    // in HBM (d_step2), so mix_root(root 3) + the draw of CirclePoint::get_random_point run on the device right behind the
    // composition tree, k_oods_maps turns the felt into every job's point and per-bit factors, and the evaluation kernels
    // start without the host having seen root 3 (it used to cost the host replay + the launches: ~60 us of idle GPU).  The host
    // replays the same steps when root 3 arrives and checks the drawn felt.
    static const bool dev_oods = getenv("CM_HOST_OODS") == nullptr;
    oods_poll = dev_oods && tune(T_OODS_POLL) != 0;
    static thread_local hipEvent_t ev_root3 = nullptr, ev_chunk0 = nullptr;
    bool chunk0_event = false;
    if (dev_oods) P.tick("composition_commit");
    const uint32_t* oods_w = nullptr;
    DevBuf d_step3;
    if (dev_oods) {
      d_step3.alloc(4 * (4 + 8));
      uint32_t* d_chan = d_step2.u32();
      chan_mix_root_draw(d_chan, P.trees[3].merkle.layers[0].u32(), d_step3.u32(), d_step3.u32() + 4, st);
      // root 3 and the felt come back HERE in stream order — in front of the evaluation kernels enqueued next
      CM_HIP(hipMemcpyAsync(pinned_words() + PIN_STEP3, d_step3.p, 48, hipMemcpyDeviceToHost, st));   // {felt[4], root 3 [8]}: one copy
      CM_HIP(hipEventRecord(thread_event(ev_root3), st));
      std::vector<EapJob> ej[2];
      for (auto& j : ojobs) {
        EapJob e{j.log, (uint32_t)j.refs.size(), d_oods_table.as<const uint32_t*>() + j.off, QM31(), QM31(), d_oods_out.u32() + 4 * j.out_off};
        if (j.prev) {
          CPoint<M31> step = point_at_index(subgroup_gen_index(j.log));
          e.has_shift = true; e.shift_x = step.x.v; e.shift_y = (-step.y).v;
        }
        ej[j.chunk].push_back(e);
      }
      // chunk 0, its values to the host, chunk 1, its values (one pinned landing buffer)
      uint8_t* land = (uint8_t*)stage_landing(n_oods_out * 16, st);
      oods_w = (const uint32_t*)land;
      // Polling form (default; A/B: CM_OODS_POLL=0 = copy commands + event / stream synchronisation): the reduction kernel writes
      // every sampled value into the landing buffer itself, next to its copy in HBM — the 12.5 KB copy of chunk 0 went through the
      // SDMA engine and cost 27 us between the two chunks' kernels — and the host does not wait for an event: it fills the landing
      // words with a value no M31 word takes and watches them change.
      const bool host_write = oods_poll && tune(T_OODS_HOST_WRITE) != 0;
      if (oods_poll) memset(land, 0xFF, n_oods_out * 16);
      if (host_write)
        for (int c = 0; c < 2; c++)
          for (auto& e : ej[c]) e.h_out = (uint32_t*)land + (e.d_out - d_oods_out.u32());
      eval_at_point_multi(ej[0], st, d_step3.u32());
      if (n_oods_out0 && !host_write) CM_HIP(hipMemcpyAsync(land, d_oods_out.p, n_oods_out0 * 16, hipMemcpyDeviceToHost, st));
      if (!ej[1].empty()) {
        if (!oods_poll) {
          CM_HIP(hipEventRecord(thread_event(ev_chunk0), st));
        }
        chunk0_event = true;
        eval_at_point_multi(ej[1], st, d_step3.u32());
        if (!host_write)
          CM_HIP(hipMemcpyAsync(land + n_oods_out0 * 16, d_oods_out.as<uint8_t>() + n_oods_out0 * 16, (n_oods_out - n_oods_out0) * 16, hipMemcpyDeviceToHost, st));
      }
    }
    // ONE round trip for two roots: root 3 is waited for; root 2 and the random coefficient of the device-side step are
    // already in pinned memory.  Host replay in transcript order.
    ht.mark("composition: enqueued, waiting for root 3");
    if (dev_oods) {   // the root comes back behind the tree, NOT behind the evaluation kernels enqueued after it
      CM_HIP(hipEventSynchronize(ev_root3));
      memcpy(P.trees[3].root.data(), pinned_words() + PIN_STEP3 + 4, 32);
    } else {
      P.trees[3].merkle.root(P.trees[3].root.data(), st);
    }
    ht.mark("composition: root 3 arrived");
    {
      memcpy(P.trees[2].root.data(), pinned_words() + PIN_ROOT2, 32);
      ch.mix_root(P.trees[2].root);
      const QM31 rho = ch.draw_felt();
      CM_CHECK(rho == QM31::from_u32(pinned_words() + PIN_COEFF), "composition: device transcript diverged from the host channel");
      QM31 cur(M31(1));
      for (size_t g = powers.size(); g-- > 0;) { powers[g] = cur; cur = cur * rho; }   // host copy: the OODS check needs it
    }
    ch.mix_root(P.trees[3].root);
    ht.mark("composition: host replay of the coefficient step");
    if (!dev_oods) P.tick("composition_commit");

    ht.mark("(composition commit done)");
    // ---- OODS sampling ----
    {
      QM31 t;
      oods = draw_oods_point(ch, &t);
      if (dev_oods) CM_CHECK(t == QM31::from_u32(pinned_words() + PIN_STEP3), "oods: device transcript diverged from the host channel");
    }
    ht.mark("oods: point drawn");
    std::map<uint32_t, CPoint<QM31>> prev_points;
    {
      std::vector<OJob>& jobs = ojobs;
      const size_t n_out = n_oods_out;
      DevBuf& dout = d_oods_out;
      {
        std::vector<EapJob> ej;
        for (auto& j : jobs) {
          j.pt = oods;
          if (j.prev) {
            CPoint<M31> step = point_at_index(subgroup_gen_index(j.log));
            CPoint<QM31> neg{QM31(step.x), QM31(-step.y)};
            j.pt = cadd(oods, neg);
            prev_points[j.log] = j.pt;
          }
          ej.push_back(EapJob{j.log, (uint32_t)j.refs.size(), d_oods_table.as<const uint32_t*>() + j.off, j.pt.x, j.pt.y,
                              dout.u32() + 4 * j.out_off});
        }
        if (!dev_oods) eval_at_point_multi(ej, st);   // (device form: already running, from the felt of the device-side step)
      }
      const uint32_t* w = dev_oods ? oods_w : (const uint32_t*)stage_download_async(dout.p, n_out * 16, st);   // read after the sync below
      ht.mark("oods: enqueued");
      // ---- while the evaluation kernels run: everything about the sampled values and the DEEP quotients
      // (compute_fri_quotients) that does not depend on the values themselves ----
      for (auto& j : jobs)
        for (auto& r : j.refs) pf.sampled_values[r.t][r.c].push_back(QM31());   // mask order [-1, 0]: sized now, filled below
      size_t n_samples = 0;
      for (auto& t : pf.sampled_values) for (auto& c : t) n_samples += c.size();
      // compute_fri_quotients' host side (quotient_plan.hpp): to the device now, behind the OODS kernels; only the random coefficient is missing
      {
        std::vector<QuotientCol> qcols;
        for (int t = 0; t < 4; t++)
          for (uint32_t c = 0; c < P.trees[t].lde.size(); c++) qcols.push_back({t, c, P.trees[t].lde.logs[c], P.trees[t].lde.ptrs[c]});
        QuotientPlan plan;
        plan.build(qcols, pf.sampled_values, sidx_cur, sidx_prev, oods, prev_points, cfg.log_blowup_factor, QuotientWindow(), st);
        d_qblob.alloc(plan.blob.size());
        plan.bind(d_qblob.as<uint8_t>());
        stage_upload(d_qblob.p, plan.blob.data(), plan.blob.size(), st);
        o_qjobs = plan.o_jobs; n_qjobs = plan.n_jobs;
        qg = std::move(plan.groups);
      }
      ht.mark("oods: overlapped quotient planning");
      // channel.mix_felts(flattened sampled values): chunk 0 is hashed as soon as it has landed, while chunk 1 is evaluated
      Channel::FeltMixer fm;
      ch.mix_felts_begin(fm);
      std::vector<QM31> flat;
      flat.reserve(n_samples);
      auto fill = [&](int chunk) {
        for (auto& j : jobs)
          if (j.chunk == chunk)
            for (size_t i = 0; i < j.refs.size(); i++) {
              auto& sv = pf.sampled_values[j.refs[i].t][j.refs[i].c];
              (j.refs[i].prev ? sv.front() : sv.back()) = QM31::from_u32(&w[4 * (j.out_off + i)]);
            }
      };
      size_t ft = 0, fc = 0, n_mixed = 0;   // cursor of the flat order: (tree, column)
      auto mix_upto = [&](size_t n_flat) {
        flat.clear();
        while (ft < 4 && n_mixed + flat.size() < n_flat) {
          auto& tr = pf.sampled_values[ft];
          if (fc == tr.size()) { ft++; fc = 0; continue; }
          for (auto& sm : tr[fc]) flat.push_back(sm);
          fc++;
        }
        ch.mix_felts_update(fm, flat.data(), flat.size());
        n_mixed += flat.size();
      };
      // all words of [w0, w1) have arrived from the device (every word the copy writes is < 2^31); gives up after ~2 ms of
      // spinning and lets the caller synchronise instead
      auto landed = [&](size_t q0, size_t q1) {
        const volatile uint32_t* v = w;
        for (int spin = 0; spin < 200000; spin++) {
          size_t i = 4 * q1;
          while (i > 4 * q0 && v[i - 1] != 0xFFFFFFFFu) i--;
          if (i == 4 * q0) { std::atomic_thread_fence(std::memory_order_acquire); return true; }
          cpu_relax();
        }
        return false;
      };
      if (chunk0_event) {
        if (!oods_poll) CM_HIP(hipEventSynchronize(ev_chunk0));
        else if (!landed(0, n_oods_out0)) CM_HIP(hipStreamSynchronize(st));
        ht.mark("oods: chunk 0 landed");
        fill(0);
        mix_upto(n_flat0);
        ht.mark("oods: chunk 0 filled + mixed");
      }
      if (!(oods_poll && landed(chunk0_event ? n_oods_out0 : 0, n_out))) CM_HIP(hipStreamSynchronize(st));
      ht.mark("oods: waited for gpu");
      if (!chunk0_event) fill(0);
      fill(1);
      mix_upto(n_samples);
      CM_CHECK(n_mixed == n_samples, "oods: flat sample count");
      ch.mix_felts_end(fm);
      ht.mark("oods: fill + mix_felts");
    }
    P.tick("oods_sampling");
  }

  // compute_fri_quotients: one launch per size group
  void deep_quotients() {
    // ---- DEEP quotients (compute_fri_quotients): the value-dependent coefficients, one upload, the launches ----
    QM31 qcoeff = ch.draw_felt();
    {
      // per-sample coefficients, batch sums and batch coefficients: one small kernel on the sampled values in HBM
      quotient_coeffs((const QuotientCoefJob*)(d_qblob.as<uint8_t>() + o_qjobs), (uint32_t)n_qjobs, d_oods_out.u32(), qcoeff, st);
      const uint8_t* base = d_qblob.as<uint8_t>();
      // one kernel per size group, independent outputs: the small groups (latency-bound, ~140 us in a row) overlap the large
      KProfRegion kregq("k_quotients", st);   // concurrent launches: timed as one interval
      Fork fkq(st);
      int qk = 0;
      std::vector<std::pair<QuotientArgs, double>> qargs = quotient_args(qg, base, *P.tw);
      for (auto& g : qg) { q_logs.push_back(g.log); quotients.push_back(std::move(g.out)); }
      // (round 6) The FRI first-layer tree's leaf layer — 2^log hashes of four words each, 8.4 M compressions at the metric config,
      // 0.21 ms as a launch of its own with the GPU otherwise idle — is written by the quotient kernel of the LARGEST size group:
      // that kernel waits on HBM (4 B per LDE cell in, 4.1 TB/s) and its VALU ports are half idle.  "quot_leaf" = 0: separate launch.
      if (quotient_leaf_wanted(qargs)) {
        fri.first_tree.leaf_prealloc.alloc((size_t)32 << qargs[0].first.log_size);
        qargs[0].first.leaf_hashes = fri.first_tree.leaf_prealloc.u32();
        fri.first_leaf_done = true;
      }
      // the small groups (latency-bound column-slice kernels, ~170 us in a row) go FIRST, together on one side stream, so that
      // they hide under the large groups instead of trailing them (they ended the region ~90 us after the last large kernel);
      // the large groups follow by descending size, one stream each
      for (auto& qa : qargs) if (qa.first.log_size < 14) launch_quotients(qa.first, qa.second, fkq.stream(Fork::N - 1));
      for (auto& qa : qargs)
        if (qa.first.log_size >= 14) { launch_quotients(qa.first, qa.second, fkq.stream(qk == 0 ? Fork::main_or(0) : qk % fork_width(Fork::N - 1))); qk++; }
      fkq.join();
      kregq.close();
    }
    P.tick("quotients");
    ht.mark("quotients: gpu done");

  }

  // FRI commit phase (FriPhase), proof of work, and — device-side tail (tail_device.hpp) — the whole rest of the proof
  DeviceTail tail;
  bool tail_done = false;
  void fri_and_pow() {
    // ---- FRI commit (FriPhase::commit) ----
    fri.commit_enqueue(P, cfg, quotients, q_logs);
    const bool dev_tail = DeviceTail::supported(cfg, q_logs, fri);
    // last layer -> PoW -> queries -> decommitment of every tree, enqueued behind the last fold: no host round trip
    if (dev_tail) tail.enqueue(P, fri, quotients, q_logs);
    check_composition_at_oods(pf, tr0, it0, clog, hrel, powers, coff, oods);   // host-only, overlapped with the kernels enqueued above
    ht.mark("fri: enqueued, oods check done");
    // The host now waits ~2 ms for the FRI layers: give back what nothing enqueued later can need — the trace-domain evaluations,
    // the coefficient columns of the four trees, the small per-phase tables — instead of doing it between two proofs with the GPU
    // idle.  (Pool blocks are reused in stream order on this thread's stream: releasing them under running kernels is safe.)
    if (defer_teardown()) {
      tr_evals = ColumnSet();
      if (!pp_cache_enabled()) pp_evals = ColumnSet();
      for (int t = pp_cache_enabled() ? 1 : 0; t < 4; t++) P.trees[t].coeffs = ColumnSet();
      drel = DevBuf(); d_powers = DevBuf(); d_step1 = DevBuf(); d_step2 = DevBuf(); d_ctab = DevBuf(); d_oods_table = DevBuf(); d_qblob = DevBuf();
      ht.mark("fri: early teardown");
    }
    if (dev_tail) {
      tail.wait_last(st);                                // challenges, roots and the last layer are in pinned memory ...
      ht.mark("tail: last layer landed");
      fri.commit_finish(P, cfg, pf, true);               // ... replayed while the proof of work and the tables run
      ht.mark("tail: commit phase replayed");
      tail.wait_tables(st);
      if (tail.nonce_found()) {
        pf.proof_of_work = tail.nonce();
        ch.mix_u64(pf.proof_of_work);
        CM_CHECK(ch.trailing_zeros() >= cfg.pow_bits, "pow: the device's nonce fails the host's check");
        tail.plan(Queries::draw(ch, cfg.n_queries, q_logs[0]));   // host tables while the gathers write the witnesses
        tail_done = true;
        ht.mark("tail: nonce, queries, host tables");
        return;
      }
      // (no nonce within 16x the expected range, probability e^-16: search on with the host-driven form; the decommitment
      // the device made from nothing is discarded)
      CM_HIP(hipStreamSynchronize(st));
    } else {
      fri.commit_finish(P, cfg, pf, false);
      P.tick("fri_commit");
    }
    pf.proof_of_work = grind_gpu(ch.digest.data(), cfg.pow_bits, st);
    ch.mix_u64(pf.proof_of_work);
    if (!dev_tail) P.tick("pow");
    ht.mark("pow done");

  }

  // queries, one batched gather for every tree, proof assembly
  void decommit() {
    if (tail_done) {   // the witnesses land in pinned memory in proof order: wait for the last gather, copy them
      CM_HIP(hipStreamSynchronize(st));
      ht.mark("tail: gpu done");
      tail.copy(P, fri, pf);
      ht.mark("decommit: copied the device tail's witnesses");
      return;
    }
    // ---- queries + decommitment ----
    Queries queries = Queries::draw(ch, cfg.n_queries, q_logs[0]);
    ht.mark("decommit: queries drawn");
    const bool ticked = tail.enqueued;   // (device tail without a nonce: its phase events are already in the stream)
    std::map<uint32_t, std::vector<uint32_t>> qpos;
    for (auto l : q_logs) qpos[l] = queries.fold(queries.log_domain_size - l).positions;
    ht.mark("decommit: qpos");
    {
      // One batched gather for every tree of the proof: FRI first layer, inner layers, the 4 commitment trees.
      GatherBatch gb;
      {  // ~ n_queries x tree depth x (2 siblings) per tree; growing these vectors dominated the planning time
        const size_t per_tree = (size_t)cfg.n_queries * 2 * (q_logs[0] + 2);
        gb.hash_addrs.reserve(per_tree * (fri.inner.size() + 5));
        gb.word_addrs.reserve((size_t)cfg.n_queries * 8 * (fri.inner.size() + 1));
        gb.runs.reserve((size_t)cfg.n_queries * 4 * (q_logs[0] + 2));
      }
      fri.plan_decommit(queries, qpos, quotients, q_logs, gb);
      DecommitPlan tree_plan[4];
      ht.mark("decommit: fri plans");
      for (int t = 0; t < 4; t++) tree_plan[t] = P.trees[t].merkle.plan_decommit(qpos, gb);
      ht.mark("decommit: tree plans");
      gb.run(st);
      ht.mark("decommit: gather run (upload+kernel+d2h)");
      fri.finish_decommit(gb, pf);
      ht.mark("decommit: finish fri");
      pf.decommitments.resize(4);
      pf.queried_values.resize(4);
      for (int t = 0; t < 4; t++) {
        MerkleTree::finish_decommit(tree_plan[t], gb, pf.queried_values[t], pf.decommitments[t]);
        pf.commitments.push_back(P.trees[t].root);
      }
      ht.mark("decommit: finish trees");
    }
    ht.mark("decommit: finish (locals released)");
    if (!ticked) P.tick("decommit");
  }
};
ProofData* prove(const DeviceInput& din, const cm_pcs_config& cfg) {
  static const bool marks = getenv("CM_HOST_MARKS") != nullptr;
  static thread_local std::chrono::steady_clock::time_point last_return;
  static thread_local bool have_last = false;
  auto now = [] { return std::chrono::steady_clock::now(); };
  if (marks && have_last) fprintf(stderr, "[host] %-40s %8.1f us\n", "(between two proofs: caller)", std::chrono::duration<double, std::micro>(now() - last_return).count());
  const auto t0 = now();
  ProofData* r;
  std::chrono::steady_clock::time_point t1;
  if (const uint64_t budget = mem_budget()) check_item_fits(item_bytes(din.meta, device_input_bytes(din), cfg, 1), budget, "cm_prove");
  struct InFlight { InFlight() { mem_proof_enter(); } ~InFlight() { mem_proof_leave(); } } mem_in_flight;
  {
    SegmentProver sp(din, cfg);
    if (marks) fprintf(stderr, "[host] %-40s %8.1f us\n", "(prover object constructed)", std::chrono::duration<double, std::micro>(now() - t0).count());
    r = sp.run();
    t1 = now();
  }
  if (marks) fprintf(stderr, "[host] %-40s %8.1f us\n", "(prover object destroyed)", std::chrono::duration<double, std::micro>(now() - t1).count());
  last_return = now(); have_last = true;
  return r;
}

#include "prover_sharded.inc"

}  // namespace cm

// ---- segment pipeline: several independent segment proofs in flight on one GPU ---------------
// Continuation segments are independent proofs (runner/src/vm/mod.rs:184-240).  Every worker is a persistent
// host thread with its own main stream, side streams, device pool and upload ring (all thread-local), so the
// launch gaps, host round trips and latency-bound kernels of one proof overlap with the others' work.
namespace cm {
namespace {
struct ProveWorkers {
  std::mutex mu;
  std::condition_variable cv;
  std::deque<std::function<void()>> jobs;
  std::vector<std::thread> threads;
  void ensure(unsigned n) {
    std::lock_guard<std::mutex> lk(mu);
    while (threads.size() < n) {
      threads.emplace_back([this] {
        bool placed = false;
        for (;;) {
          std::function<void()> job;
          {
            std::unique_lock<std::mutex> lk2(mu);
            cv.wait(lk2, [this] { return !jobs.empty(); });
            job = std::move(jobs.front());
            jobs.pop_front();
          }
          // library-owned thread: it stays next to the GPU (cm_init has run by the time a job arrives)
          if (!placed) { bind_worker_thread_cpus(); placed = true; }
          job();
        }
      });
      threads.back().detach();
    }
  }
  void submit(std::function<void()> f) {
    { std::lock_guard<std::mutex> lk(mu); jobs.push_back(std::move(f)); }
    cv.notify_one();
  }
};
ProveWorkers& prove_workers() { static ProveWorkers* w = new ProveWorkers(); return *w; }
}  // namespace

// ---- the drivers behind cm_prove_many* and cm_prove_run* (api_prove.hip, api_run.hip): they return when every item has been
// proved or given up, and throw the first error of a worker or producer ----
void prove_many(const cm_device_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs) {
  if (!n) return;
  if (inflight < 1) inflight = 1;
  if (inflight > 8) inflight = 8;
  cm_pcs_config cfg = config ? *config : default_cfg();
  ProveWorkers& w = prove_workers();
  w.ensure(inflight);
  struct Shared { std::mutex mu; std::condition_variable cv; uint32_t done = 0, next = 0; int32_t rc = 0; std::string err; } sh;
  for (uint32_t i = 0; i < n; i++) outs[i] = nullptr;
  const uint32_t runners = inflight < n ? inflight : n;
  // under a memory budget the caller's inputs count as resident for the whole call (Admission)
  uint64_t resident = 0;
  if (mem_budget()) for (uint32_t i = 0; i < n; i++) if (inputs[i] && inputs[i]->d) resident += device_input_bytes(*inputs[i]->d);
  struct Resident { uint64_t b; Resident(uint64_t b_) : b(b_) { if (b) admission().add_inputs(b); } ~Resident() { if (b) admission().sub_inputs(b); } } resident_scope(resident);
  // `runners` jobs, each pulling segment indices until none is left: exactly that many proofs are in flight
  for (uint32_t r = 0; r < runners; r++) {
    w.submit([&] {
      struct InFlight { InFlight() { g_proofs_in_flight.fetch_add(1); } ~InFlight() { g_proofs_in_flight.fetch_sub(1); } } in_flight;
      for (;;) {
        uint32_t i;
        { std::lock_guard<std::mutex> lk(sh.mu); i = sh.next++; }
        if (i >= n) break;
        int32_t rc = 0;
        std::string err;
        try {
          std::unique_ptr<cm_proof> p(new cm_proof());
          p->d = prove_admitted(*inputs[i]->d, cfg, "cm_prove_many");
          outs[i] = p.release();
        } catch (const CmError& e) { rc = e.code ? e.code : 1; err = e.what(); }
        catch (const std::exception& e) { rc = 1; err = e.what(); }
        if (rc) { std::lock_guard<std::mutex> lk(sh.mu); if (!sh.rc) { sh.rc = rc; sh.err = err; } }
      }
      std::lock_guard<std::mutex> lk(sh.mu);
      sh.done++;
      sh.cv.notify_all();
    });
  }
  std::unique_lock<std::mutex> lk(sh.mu);
  sh.cv.wait(lk, [&] { return sh.done == runners; });
  lk.unlock();
  if (sh.rc) throw CmError(sh.rc, sh.err);
}
// ---- streaming ingest (prover.rs:23-29 takes a HOST `&mut ProverInput`, the reference's bench clones one per
// iteration, benches/prover_speed_benchmark.rs:65) ---------------------------------------------------------------------------
// The calling thread is the PRODUCER: it turns item i into a device-resident input (upload of a host ProverInput, or the device
// adapter on a runner segment) on its own stream and device pool while up to `inflight` worker threads prove the items before
// it.  At most inflight + 1 device inputs are alive (the ones being proved and the one being produced); a spent input goes back
// to the producer, which releases it into ITS pool — the next upload reuses the same blocks, so a steady stream of equal-sized
// n_producers: threads that turn items into device inputs (the calling thread + n_producers - 1 library threads).  One is enough
// for plain uploads (6 ms of PCIe per 10 ms proof); the device adapter is ~13 ms of uploads, kernels and five host round trips per
// segment while the GPU is busy proving, so runner segments get two.  An input is released by the producer that made it (its
// device pool owns the blocks).
// need(i, cfg, known): the bytes item i takes (ItemBytes), for the memory budget; known = false when only an upper guess of the
// input can be made before the item exists (runner segments: the refusal then happens in front of the proof, not the adapter)
template <class Produce, class Need>
static void prove_streamed(uint32_t n, Produce&& produce, Need&& need, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs,
                           uint32_t n_producers = 1) {
  if (!n) return;
  if (inflight < 1) inflight = 1;
  if (inflight > 8) inflight = 8;
  if (n_producers < 1) n_producers = 1;
  if (n_producers > 3) n_producers = 3;
  if (n_producers > n) n_producers = n;
  const cm_pcs_config cfg = config ? *config : default_cfg();
  for (uint32_t i = 0; i < n; i++) outs[i] = nullptr;
  ProveWorkers& w = prove_workers();
  w.ensure(inflight + n_producers - 1);
  struct Job { uint32_t i; DeviceInput* d; uint32_t pid; uint64_t bytes; };   // bytes: what Admission counts as resident for it
  struct Shared {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Job> ready;                         // produced, not yet picked up
    std::deque<std::pair<DeviceInput*, uint64_t>> spent[3];   // proved: back to the producer that made them (with Job::bytes)
    uint32_t outstanding[3] = {0, 0, 0};           // inputs of producer p that exist (being produced, ready, being proved, spent)
    uint32_t alive = 0, next_i = 0, workers_done = 0, producers_done = 0, n_producers = 1;
    uint32_t extra_done = 0;                       // library-thread producers that have left `sh` for good (counted under `mu`)
    bool no_more = false, stop = false;
    int32_t rc = 0;
    std::string err;
  } sh;
  sh.n_producers = n_producers;
  const uint32_t cap = inflight + n_producers;     // device inputs alive at once
  const uint32_t runners = inflight < n ? inflight : n;
  for (uint32_t r = 0; r < runners; r++) {
    w.submit([&sh, &cfg, outs] {
      struct InFlight { InFlight() { g_proofs_in_flight.fetch_add(1); } ~InFlight() { g_proofs_in_flight.fetch_sub(1); } } in_flight;
      for (;;) {
        Job job;
        {
          std::unique_lock<std::mutex> lk(sh.mu);
          sh.cv.wait(lk, [&] { return !sh.ready.empty() || sh.no_more; });
          if (sh.ready.empty()) break;
          job = sh.ready.front();
          sh.ready.pop_front();
        }
        int32_t rc = 0;
        std::string err;
        try {
          std::unique_ptr<cm_proof> p(new cm_proof());
          p->d = prove_admitted(*job.d, cfg, "cm_prove_many (streamed)");
          outs[job.i] = p.release();
        } catch (const CmError& e) { rc = e.code ? e.code : 1; err = e.what(); }
        catch (const std::exception& e) { rc = 1; err = e.what(); }
        catch (...) { rc = 1; err = "unknown error"; }
        std::lock_guard<std::mutex> lk(sh.mu);
        if (rc && !sh.rc) { sh.rc = rc; sh.err = err; }
        sh.spent[job.pid].push_back({job.d, job.bytes});
        sh.cv.notify_all();
      }
      std::lock_guard<std::mutex> lk(sh.mu);
      sh.workers_done++;
      sh.cv.notify_all();
    });
  }
  // one producer: takes the next index while a slot is free, makes the device input, hands it to the workers; frees what comes back
  auto producer = [&sh, &produce, &need, &cfg, n, cap](uint32_t pid) {
    bind_thread_to_library_device();
    auto release_spent = [&](std::unique_lock<std::mutex>& lk) {   // lock held on entry and exit; the frees run outside of it
      std::deque<std::pair<DeviceInput*, uint64_t>> v;
      v.swap(sh.spent[pid]);
      sh.alive -= (uint32_t)v.size();
      sh.outstanding[pid] -= (uint32_t)v.size();
      lk.unlock();
      for (auto& d : v) { delete d.first; if (d.second) admission().sub_inputs(d.second); }
      lk.lock();
      sh.cv.notify_all();
    };
    for (;;) {
      uint32_t i;
      {
        std::unique_lock<std::mutex> lk(sh.mu);
        sh.cv.wait(lk, [&] { return !sh.spent[pid].empty() || sh.stop || sh.next_i >= n || sh.alive < cap; });
        if (!sh.spent[pid].empty()) { release_spent(lk); continue; }
        if (sh.stop || sh.next_i >= n) break;
        if (sh.alive >= cap) continue;
        i = sh.next_i++;
        sh.alive++;
        sh.outstanding[pid]++;
      }
      DeviceInput* d = nullptr;
      int32_t rc = 0;
      std::string err;
      uint64_t counted = 0;     // bytes Admission holds as resident for this item
      bool refused = false;     // over the memory budget on its own: this item fails, the others go on
      try {
        if (const uint64_t budget = mem_budget()) {
          bool known = true;
          const ItemBytes b = need(i, cfg, known);
          if (known) { refused = true; check_item_fits(b, budget, "cm_prove_many (streamed)"); refused = false; }
          // while this producer waits for room, the inputs it is asked to release must still go back (a worker's proof ends,
          // its input comes back here, and only its release makes the room)
          while (!admission().try_admit_input(b.input)) {
            std::unique_lock<std::mutex> lk(sh.mu);
            if (!sh.spent[pid].empty()) release_spent(lk);
            else sh.cv.wait_for(lk, std::chrono::milliseconds(1));   // (a finished proof notifies; the limit covers other pipelines' proofs)
          }
          counted = b.input;
        }
        d = produce(i);
        if (counted) {   // the real size, once the input exists
          const uint64_t real = device_input_bytes(*d);
          if (real > counted) admission().add_inputs(real - counted); else admission().sub_inputs(counted - real);
          counted = real;
        }
      }
      catch (const CmError& e) { rc = e.code ? e.code : 1; err = e.what(); }
      catch (const std::exception& e) { rc = 1; err = e.what(); }
      catch (...) { rc = 1; err = "unknown error"; }
      if (!d && counted) admission().sub_inputs(counted);
      std::lock_guard<std::mutex> lk(sh.mu);
      if (!d) {   // this item cannot be made: report it, stop producing (the items already handed over are still proved)
        if (!sh.rc) { sh.rc = rc ? rc : 1; sh.err = err; }
        if (!refused) sh.stop = true;
        sh.alive--;
        sh.outstanding[pid]--;
      } else sh.ready.push_back(Job{i, d, pid, counted});
      sh.cv.notify_all();
    }
    std::unique_lock<std::mutex> lk(sh.mu);
    if (++sh.producers_done == sh.n_producers) sh.no_more = true;
    sh.cv.notify_all();
    // its inputs come back as the workers finish: release them here, on the thread whose pool owns them
    while (sh.outstanding[pid] > 0) {
      sh.cv.wait(lk, [&] { return !sh.spent[pid].empty(); });
      release_spent(lk);
    }
  };
  // (the completion count is bumped INSIDE the lock, like workers_done: the caller's wait below reads it under the same lock, so it
  // cannot return — and destroy `sh` — between the count and the notify; the job touches nothing of `sh` after the guard)
  for (uint32_t pid = 1; pid < n_producers; pid++)
    w.submit([&producer, &sh, pid] { producer(pid); std::lock_guard<std::mutex> lk(sh.mu); sh.extra_done++; sh.cv.notify_all(); });
  {
    AffinityScope cpu_scope;
    producer(0);
  }
  {
    std::unique_lock<std::mutex> lk(sh.mu);
    sh.cv.wait(lk, [&] { return sh.workers_done == runners && sh.extra_done == n_producers - 1; });
  }
  if (sh.rc) throw CmError(sh.rc, sh.err);
}
void prove_many_host(const cm_prover_input* const* inputs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs) {
  prove_streamed(n, [&](uint32_t i) {
    CM_CHECK(inputs && inputs[i], "cm_prove_many_host: null input");
    return upload_input(*inputs[i], thread_main_stream());
  }, [&](uint32_t i, const cm_pcs_config& cfg, bool& known) {
    CM_CHECK(inputs && inputs[i], "cm_prove_many_host: null input");
    known = true;
    return item_bytes(*inputs[i], estimate_input_bytes(*inputs[i]), cfg, 1);
  }, config, inflight, outs);
}
void prove_many_segments(const cm_runner_segment* const* segments, uint32_t n, const cm_pcs_config* config, uint32_t inflight,
                         cm_proof** outs) {
  prove_streamed(n, [&](uint32_t i) {
    CM_CHECK(segments && segments[i], "cm_prove_many_segments: null segment");
    return adapt_segment_device(*segments[i]);
  }, [&](uint32_t i, const cm_pcs_config&, bool& known) {
    CM_CHECK(segments && segments[i], "cm_prove_many_segments: null segment");
    // before the adapter has run only the step and access counts are known: one bundle per step, one data access and at most one
    // clock update per logged access, boundary memory and its two Merkle paths from the cells the accesses can touch
    known = false;
    const cm_runner_segment& g = *segments[i];
    const uint64_t cells = g.n_initial_memory + g.n_initial_heap + g.n_memory_trace;
    return ItemBytes{g.n_trace * sizeof(cm_bundle) + g.n_memory_trace * (sizeof(cm_data_access) + sizeof(cm_clock_update)) +
                             2 * cells * sizeof(cm_memory_cell), 0};
  }, config, inflight, outs, /*n_producers=*/2);
}
void check_run_segment(const cm_run_segment* seg, const char* who) {
  CM_CHECK(seg, (std::string(who) + ": null segment").c_str());
  CM_CHECK(seg->trace && seg->memory_trace, (std::string(who) + ": null trace or memory trace").c_str());
}
// The ingest loop of cm_prove_run and cm_prove_run_transitions.  transitions (null for cm_prove_run): segment i's write-set transition
// (mem_transition.hip) is opened on the adapting thread right after the adapter, before the input is handed to a worker; when that
// throws the segment counts as one that could not be made.
void prove_run(const char* who, Run& run, const cm_run_segment* const* segs, uint32_t n, const cm_pcs_config* config, uint32_t inflight, cm_proof** outs,
               cm_mem_transition** transitions) {
  // the image is serial: ONE producer (the calling thread) adapts the segments in order, the workers prove behind it
  std::lock_guard<std::mutex> lk(run_mutex(run));
  prove_streamed(n, [&](uint32_t i) {
    check_run_segment(segs[i], who);
    std::unique_ptr<DeviceInput> d(run_adapt_next(run, *segs[i]));
    if (transitions) transitions[i] = open_transition(*d, nullptr, 0);
    return d.release();
  }, [&](uint32_t i, const cm_pcs_config&, bool& known) {
    check_run_segment(segs[i], who);
    known = false;   // as for cm_prove_many_segments: the component sizes exist once the adapter has run
    const cm_run_segment& g = *segs[i];
    const uint64_t cells = run_rows_bound(run, g.n_memory_trace);   // (the image as it is now: this thread is its only writer)
    return ItemBytes{g.n_trace * sizeof(cm_bundle) + g.n_memory_trace * (sizeof(cm_data_access) + sizeof(cm_clock_update)) +
                             2 * cells * sizeof(cm_memory_cell), 0};
  }, config, inflight, outs, /*n_producers=*/1);
}
}  // namespace cm
