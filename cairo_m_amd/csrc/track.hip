// Relation tracker (reference: debug_tools/relation_tracker.rs:21-31, RelationSummary::summarize_relations(..).cleaned()): the
// relation tuples of a segment, or of one component's columns, whose multiplicities do not sum to zero modulo P, each with its net
// multiplicity, the lowest (component, row) that holds it and the number of entries merged.  Where the reference pushes every entry
// through a HashMap on the CPU, this runs per tracked relation, one after the other (the buffers are bounded by the largest one):
//   emit     k_track_emit / k_track_emit_small (kernels_track.inc): one record per entry in a fixed slot; the public data's entries
//            (the terms of the verifier's initial_logup_sum, enumerated) are appended by the host
//   group    two stable 64-bit radix sorts over a permutation (low half of the key, then the high half)
//   net      a run-length reduction over the sorted order: sum of the multiplicities (64-bit, reduced modulo P once), lowest
//            locator, count; then a stable selection of the runs whose net is not zero
//   recover  k_track_recover re-evaluates the survivors' rows for their values; public survivors are filled in here
// Grouping key: the entry's LogUp denominator sum_i alpha^i v_i - z (4 words = 124 bits).  Two different tuples of one relation of
// at most 16 values share it with probability <= 16 / |QM31| ~ 2^-120 over drawn (z, alpha) — the same event that blinds the LogUp
// argument itself; trailing zeros drop out by construction.  Degenerate caller-supplied relations (alpha = 0) merge tuples here
// exactly as they do in the sum check.
#include "../../include/cairom_hip.h"
#include "segment_input.hpp"
#include "handles.hpp"
#include "abi.hpp"
#include "track_kernels.hpp"
#include "air_kernels.hpp"
#include "kprof.hpp"
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

constexpr int NC = air::N_COMPONENTS;

struct PublicTuple { uint32_t mult; int n; uint32_t v[air::MAX_REL_SIZE]; };
// the terms of initial_logup_sum (verifier.hip; public_data.rs:287-394), one tuple per term
void public_tuples(const PublicData& d, std::vector<PublicTuple> out[air::N_RELATIONS]) {
  const uint32_t minus_one = P - 1;
  const auto push = [&](int r, uint32_t mult, std::initializer_list<M31> vals) {
    PublicTuple t{};
    t.mult = mult;
    for (M31 v : vals) t.v[t.n++] = v.v;
    out[r].push_back(t);
  };
  const M31 one(1), zero;
  push(air::REL_REGISTERS, 1, {M31(d.initial_pc), M31(d.initial_fp), one});
  push(air::REL_REGISTERS, minus_one, {M31(d.final_pc), M31(d.final_fp), M31(d.clock) + one});
  push(air::REL_MERKLE, 1, {zero, zero, M31(d.initial_root), M31(d.initial_root)});
  push(air::REL_MERKLE, 1, {zero, zero, M31(d.final_root), M31(d.final_root)});
  const auto add = [&](const std::vector<PublicEntry>& es, bool emit) {
    const M31 root(emit ? d.initial_root : d.final_root), height(air::TREE_HEIGHT), four(4);
    for (auto& e : es) {
      if (!e.present) continue;
      push(air::REL_MEMORY, emit ? 1 : minus_one, {M31(e.addr), M31(e.clock), M31(e.value[0]), M31(e.value[1]), M31(e.value[2]), M31(e.value[3])});
      for (uint32_t k = 0; k < 4; k++) push(air::REL_MERKLE, minus_one, {four * M31(e.addr) + M31(k), height, M31(e.value[k]), root});
    }
  };
  add(d.program, true);
  add(d.input, true);
  add(d.output, false);
}

struct Net { unsigned long long sum, loc, count; };
struct NetSum {
  __host__ __device__ Net operator()(const Net& a, const Net& b) const { return Net{a.sum + b.sum, a.loc < b.loc ? a.loc : b.loc, a.count + b.count}; }
};
struct Key128 {
  unsigned long long hi, lo;
  __host__ __device__ bool operator==(const Key128& o) const { return hi == o.hi && lo == o.lo; }
  __host__ __device__ bool operator!=(const Key128& o) const { return !(*this == o); }
};
// sorted position -> key / record, through the permutation
struct SortedKey {
  const unsigned long long* hi_sorted; const unsigned long long* lo; const uint32_t* perm;
  __host__ __device__ Key128 operator()(uint32_t i) const { return Key128{hi_sorted[i], lo[perm[i]]}; }
};
struct SortedNet {
  const uint32_t* mult; const unsigned long long* loc; const uint32_t* perm;
  __host__ __device__ Net operator()(uint32_t i) const { const uint32_t j = perm[i]; return Net{mult[j], loc[j], 1ull}; }
};
struct NonZeroNet {
  __host__ __device__ bool operator()(const Net& a) const { return a.sum % P != 0; }
};

__global__ void __launch_bounds__(256) k_track_iota(uint32_t* __restrict__ idx, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) idx[i] = i;
}
__global__ void __launch_bounds__(256) k_track_gather(const unsigned long long* __restrict__ src, const uint32_t* __restrict__ idx,
                                                      unsigned long long* __restrict__ dst, uint32_t n) {
  for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) dst[i] = src[idx[i]];
}
uint32_t stream_grid(uint32_t n) { return std::min<uint32_t>((n + 255) / 256, 2048); }

template <class F>
void with_temp(F&& f) {
  size_t bytes = 0;
  f(nullptr, bytes);
  DevBuf tmp(bytes);
  f(tmp.p, bytes);
}

struct Source { int cid; const uint32_t* const* d_tr; uint32_t log_size; };
struct Survivor { int relation; Net net; };

// the survivors of ONE relation, in key order: at most `want` of them are returned, *n_sel counts all
void track_one_relation(int r, const std::vector<Source>& src, const uint32_t* const* d_pp, const DevRelations* d_rels,
                        const HostRelations& hrel, const std::vector<PublicTuple>& pub, uint64_t want, std::vector<Net>& out, uint64_t& n_sel,
                        uint64_t& n_records, hipStream_t st) {
  n_sel = 0;
  // slots: every component's entries of relation r, then the public tuples
  std::vector<unsigned long long> base(src.size());
  unsigned long long n64 = 0;
  for (size_t k = 0; k < src.size(); k++) { base[k] = n64; n64 += (unsigned long long)air::component_info(src[k].cid).rel_count[r] << src[k].log_size; }
  const unsigned long long pub0 = n64;
  n64 += pub.size();
  n_records = n64;
  if (n64 == 0) return;
  CM_CHECK(n64 < (1ull << 31), std::string("relation tracker: ") + std::to_string(n64) + " entries of one relation exceed one pass (2^31)");
  const uint32_t n = (uint32_t)n64;
  // record arrays (28 bytes per slot) + the sort's double buffers (36) + the runs (24, released arrays are reused by the pool)
  const unsigned long long need = 88ull * n;
  DevBuf b_hi, b_lo, b_loc, b_mult, b_idx0, b_idx1, b_perm, b_lo_s, b_hi_g, b_hi_s, b_runs, b_nruns;
  try {
    b_hi.alloc(8ull * n); b_lo.alloc(8ull * n); b_loc.alloc(8ull * n); b_mult.alloc(4ull * n);
    b_idx0.alloc(4ull * n); b_idx1.alloc(4ull * n); b_perm.alloc(4ull * n);
    b_lo_s.alloc(8ull * n); b_hi_g.alloc(8ull * n); b_hi_s.alloc(8ull * n);
    b_runs.alloc(sizeof(Net) * (size_t)n); b_nruns.alloc(16);
  } catch (const CmError& e) {
    throw CmError(2, std::string("relation tracker: relation ") + std::to_string(r) + " has " + std::to_string(n) + " entries and needs " +
                         std::to_string(need) + " bytes of device memory (" + e.what() + ")");
  }
  TrackRecords rec{b_hi.as<unsigned long long>(), b_lo.as<unsigned long long>(), b_loc.as<unsigned long long>(), b_mult.u32()};

  // ---- emit ----
  {
    std::vector<TrackEmitArgs> small;
    std::vector<int> ids;
    for (size_t k = 0; k < src.size(); k++) {
      if (!air::component_info(src[k].cid).rel_count[r]) continue;
      TrackEmitArgs a;
      a.tr = src[k].d_tr; a.pp = d_pp; a.rels = d_rels; a.rec = rec; a.base = base[k]; a.log_size = src[k].log_size; a.relation = r; a.cid = src[k].cid;
      if (src[k].log_size <= SMALL_COMPONENT_MAX_LOG) { small.push_back(a); ids.push_back(src[k].cid); }
      else launch_track_emit(src[k].cid, a, st);
    }
    UploadBatch ub;
    TrackEmitArgs* d_small = nullptr; int* d_ids = nullptr;
    ub.add(small, &d_small); ub.add(ids, &d_ids);
    DevBuf tabs = ub.flush(st);
    launch_track_emit_small(d_small, d_ids, (uint32_t)ids.size(), st);
    if (!pub.empty()) {
      std::vector<unsigned long long> hi(pub.size()), lo(pub.size()), loc(pub.size());
      std::vector<uint32_t> mult(pub.size());
      for (size_t i = 0; i < pub.size(); i++) {
        QM31 d;
        for (int k = 0; k < pub[i].n; k++) d += hrel.alpha_pow[r][k] * M31(pub[i].v[k]);
        d = d - hrel.z[r];
        uint32_t w[4];
        d.to_u32(w);
        hi[i] = ((unsigned long long)w[0] << 32) | w[1]; lo[i] = ((unsigned long long)w[2] << 32) | w[3];
        loc[i] = TRACK_LOC(NC, 0, i); mult[i] = pub[i].mult;
      }
      CM_HIP(hipMemcpyAsync(rec.key_hi + pub0, hi.data(), 8 * pub.size(), hipMemcpyHostToDevice, st));
      CM_HIP(hipMemcpyAsync(rec.key_lo + pub0, lo.data(), 8 * pub.size(), hipMemcpyHostToDevice, st));
      CM_HIP(hipMemcpyAsync(rec.loc + pub0, loc.data(), 8 * pub.size(), hipMemcpyHostToDevice, st));
      CM_HIP(hipMemcpyAsync(rec.mult + pub0, mult.data(), 4 * pub.size(), hipMemcpyHostToDevice, st));
    }
    CM_HIP(hipStreamSynchronize(st));   // the host vectors and `tabs` above stay alive until the copies and kernels have read them
  }

  // ---- group: stable LSD sort of the permutation by (key_hi, key_lo) ----
  {
    KProfScope kp("k_track_sort", (4.0 + 2 * (12.0 + 12.0) * 8 + 16.0) * n, st);   // iota, 2 x 8 radix passes of (key, index), gather
    hipLaunchKernelGGL(k_track_iota, dim3(stream_grid(n)), dim3(256), 0, st, b_idx0.u32(), n);
    with_temp([&](void* t, size_t& b) {
      CM_HIP(hipcub::DeviceRadixSort::SortPairs(t, b, rec.key_lo, b_lo_s.as<unsigned long long>(), b_idx0.u32(), b_idx1.u32(), (int)n, 0, 63, st));
    });
    hipLaunchKernelGGL(k_track_gather, dim3(stream_grid(n)), dim3(256), 0, st, rec.key_hi, b_idx1.u32(), b_hi_g.as<unsigned long long>(), n);
    with_temp([&](void* t, size_t& b) {
      CM_HIP(hipcub::DeviceRadixSort::SortPairs(t, b, b_hi_g.as<unsigned long long>(), b_hi_s.as<unsigned long long>(), b_idx1.u32(), b_perm.u32(),
                                                (int)n, 0, 63, st));
    });
    CM_HIP(hipGetLastError());
  }

  // ---- net: one run per distinct key ----
  uint32_t n_runs = 0;
  {
    KProfScope kp("k_track_net", (8.0 + 4.0 + 8.0 + 4.0 + 8.0) * n, st);   // sorted high half, permutation, gathered low half / multiplicity / locator
    hipcub::CountingInputIterator<uint32_t> pos(0);
    hipcub::TransformInputIterator<Key128, SortedKey, hipcub::CountingInputIterator<uint32_t>> keys(
        pos, SortedKey{b_hi_s.as<unsigned long long>(), rec.key_lo, b_perm.u32()});
    hipcub::TransformInputIterator<Net, SortedNet, hipcub::CountingInputIterator<uint32_t>> vals(pos, SortedNet{rec.mult, rec.loc, b_perm.u32()});
    hipcub::DiscardOutputIterator<> no_keys;
    with_temp([&](void* t, size_t& b) {
      CM_HIP(hipcub::DeviceReduce::ReduceByKey(t, b, keys, no_keys, vals, b_runs.as<Net>(), b_nruns.u32(), NetSum(), (int)n, st));
    });
    CM_HIP(hipMemcpyAsync(&n_runs, b_nruns.p, 4, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  CM_CHECK(n_runs >= 1 && n_runs <= n, "relation tracker: run count out of range");
  // the records are no longer needed: the pool hands their blocks to the selection's output
  b_hi.release(); b_lo.release(); b_loc.release(); b_lo_s.release(); b_hi_g.release(); b_hi_s.release();
  DevBuf b_sel(sizeof(Net) * (size_t)n_runs), b_nsel(16);
  uint32_t ns = 0;
  {
    KProfScope kp("k_track_select", 24.0 * n_runs, st);
    with_temp([&](void* t, size_t& b) {
      CM_HIP(hipcub::DeviceSelect::If(t, b, b_runs.as<Net>(), b_sel.as<Net>(), b_nsel.u32(), (int)n_runs, NonZeroNet(), st));
    });
    CM_HIP(hipMemcpyAsync(&ns, b_nsel.p, 4, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  CM_CHECK(ns <= n_runs, "relation tracker: selection count out of range");
  n_sel = ns;
  const size_t take = (size_t)std::min<uint64_t>(ns, want);
  out.resize(take);
  if (take) {
    CM_HIP(hipMemcpyAsync(out.data(), b_sel.p, sizeof(Net) * take, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
}

}  // namespace

// mask: the relations to track.  entries[0, min(*n_total, cap)) are written, ordered by relation id, then by key.
void track_relations(const std::vector<int>& cids, const std::vector<const uint32_t* const*>& d_tr, const uint32_t* log_sizes,
                     const uint32_t* const* d_pp, const DevRelations* d_rels, const HostRelations& hrel, const PublicData* pubdata, uint32_t mask,
                     cm_relation_entry* entries, uint64_t cap, uint64_t* n_total, uint64_t* n_records, hipStream_t st) {
  static_assert(sizeof(cm_relation_entry) == 96 && sizeof(cm_relation_entry) % 8 == 0, "cm_relation_entry: plain words");
  static_assert(CM_MAX_RELATION_SIZE == air::MAX_REL_SIZE && TRACK_RECOVER_WORDS == air::MAX_REL_SIZE + 1, "tuple width");
  std::vector<Source> src;
  for (size_t k = 0; k < cids.size(); k++) src.push_back(Source{cids[k], d_tr[k], log_sizes[k]});
  std::vector<PublicTuple> pub[air::N_RELATIONS];
  if (pubdata) public_tuples(*pubdata, pub);
  uint64_t total = 0, written = 0, records = 0;
  std::vector<Survivor> sv;
  for (int r = 0; r < air::N_RELATIONS; r++) {
    if (!((mask >> r) & 1u)) continue;
    std::vector<Net> got;
    uint64_t n_sel = 0, n_rec = 0;
    track_one_relation(r, src, d_pp, d_rels, hrel, pub[r], cap - written, got, n_sel, n_rec, st);
    total += n_sel;
    records += n_rec;
    written += got.size();
    for (const Net& g : got) sv.push_back(Survivor{r, g});
  }
  *n_total = total;
  if (n_records) *n_records = records;
  if (sv.empty()) return;

  // ---- recover the values ----
  std::vector<TrackRecoverJob> jobs;
  std::vector<size_t> job_of(sv.size(), (size_t)-1);
  for (size_t i = 0; i < sv.size(); i++) {
    const int cid = (int)(sv[i].net.loc >> 56);
    if (cid >= NC) continue;
    size_t k = 0;
    while (k < src.size() && src[k].cid != cid) k++;
    CM_CHECK(k < src.size(), "relation tracker: locator names an unknown component");
    job_of[i] = jobs.size();
    jobs.push_back(TrackRecoverJob{src[k].d_tr, cid, sv[i].relation, (uint32_t)((sv[i].net.loc >> TRACK_ORD_BITS) & 0xffffffffu),
                                   (uint32_t)(sv[i].net.loc & ((1u << TRACK_ORD_BITS) - 1))});
  }
  std::vector<uint32_t> vals(jobs.size() * TRACK_RECOVER_WORDS);
  if (!jobs.empty()) {
    DevBuf d_jobs = upload(jobs, st), d_out(4 * vals.size());
    launch_track_recover(d_jobs.as<TrackRecoverJob>(), (uint32_t)jobs.size(), d_pp, d_out.u32(), st);
    CM_HIP(hipMemcpyAsync(vals.data(), d_out.p, 4 * vals.size(), hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  }
  for (size_t i = 0; i < sv.size(); i++) {
    cm_relation_entry& e = entries[i];
    memset(&e, 0, sizeof(e));
    e.relation = (uint32_t)sv[i].relation;
    e.multiplicity = (uint32_t)(sv[i].net.sum % P);
    e.first_component = (uint32_t)(sv[i].net.loc >> 56);
    e.first_row = (sv[i].net.loc >> TRACK_ORD_BITS) & 0xffffffffu;
    e.n_entries = sv[i].net.count;
    int n = 0;
    if (job_of[i] != (size_t)-1) {
      const uint32_t* w = vals.data() + job_of[i] * TRACK_RECOVER_WORDS;
      n = (int)std::min<uint32_t>(w[0], air::MAX_REL_SIZE);
      memcpy(e.values, w + 1, 4 * n);
    } else {
      const PublicTuple& t = pub[sv[i].relation].at((size_t)(sv[i].net.loc & ((1u << TRACK_ORD_BITS) - 1)));
      n = t.n;
      memcpy(e.values, t.v, 4 * n);
    }
    while (n > 0 && e.values[n - 1] == 0) n--;
    e.n_values = (uint32_t)n;
  }
}

}  // namespace cm

// ================================================================= C ABI
extern "C" {
int32_t cm_track_relations(const cm_device_input* input, const cm_relations* relations, uint32_t relation_mask, cm_check_report* report,
                           cm_relation_entry* entries, uint64_t cap, uint64_t* n_total) {
  return cm::abi_guard([&] {
    using namespace cm;
    CM_CHECK(input && input->d && n_total, "cm_track_relations: null input / n_total");
    CM_CHECK(entries || cap == 0, "cm_track_relations: null entries with a non-zero cap");
    CM_CHECK(relation_mask < (1u << air::N_RELATIONS), "cm_track_relations: relation_mask has bits beyond the 8 relations");
    *n_total = 0;
    cm_check_report local;
    cm_check_report& rep = report ? *report : local;
    memset(&rep, 0, sizeof(rep));
    CheckColumns cols;
    check_segment(*input->d, relations, rep, &cols);
    uint32_t mask = relation_mask;
    if (!mask)
      for (int r = 0; r < air::N_RELATIONS; r++) {
        QM31 s = QM31::from_u32(rep.public_sum[r]);
        for (int c = 0; c < air::N_COMPONENTS; c++) s += QM31::from_u32(rep.relation_sum[c][r]);
        if (!s.is_zero()) mask |= 1u << r;
      }
    if (!mask) return;
    std::vector<int> cids;
    std::vector<const uint32_t* const*> d_tr;
    for (int c = 0; c < air::N_COMPONENTS; c++) { cids.push_back(c); d_tr.push_back((const uint32_t* const*)cols.tr.dev(cols.tr0[c])); }
    track_relations(cids, d_tr, cols.clog, (const uint32_t* const*)cols.pp.dev(), cols.drel.as<DevRelations>(), cols.hrel,
                    &input->d->public_data, mask, entries, cap, n_total, nullptr, thread_main_stream());
  });
}
int32_t cm_relation_entries(int32_t c, const cm_handle* trace_cols, const cm_handle* preprocessed, uint32_t log_size,
                            const cm_relations* relations, uint32_t relation_mask, cm_relation_entry* entries, uint64_t cap,
                            uint64_t* n_total, cm_stream_t s) {
  return cm::abi_guard([&] {
    using namespace cm;
    CM_CHECK(c >= 0 && c < air::N_COMPONENTS, "bad component id");
    CM_CHECK(log_size >= 4 && log_size <= 26, "cm_relation_entries: log_size must be in 4..26");
    CM_CHECK(relations && n_total, "cm_relation_entries: null relations / n_total");
    CM_CHECK(trace_cols && preprocessed, "cm_relation_entries: null column array");
    CM_CHECK(entries || cap == 0, "cm_relation_entries: null entries with a non-zero cap");
    CM_CHECK(relation_mask < (1u << air::N_RELATIONS), "cm_relation_entries: relation_mask has bits beyond the 8 relations");
    *n_total = 0;
    bind_thread_to_library_device();
    const hipStream_t st = cm::as_stream(s);
    UploadBatch ub;
    uint32_t** d_tr = nullptr; uint32_t** d_pp = nullptr;
    ub.add(handles(trace_cols, air::component_info(c).n_trace), &d_tr);
    ub.add(handles(preprocessed, air::N_PREPROC), &d_pp);
    DevBuf tabs = ub.flush(st), drel(sizeof(DevRelations));
    stage_upload(drel.p, relations, sizeof(DevRelations), st);
    DevRelations w;
    memcpy(&w, relations, sizeof(w));
    HostRelations hrel;
    for (int r = 0; r < air::N_RELATIONS; r++) {
      hrel.z[r] = QM31::from_u32(w.z[r]);
      for (int i = 0; i < air::MAX_REL_SIZE; i++) hrel.alpha_pow[r][i] = QM31::from_u32(w.alpha_pow[r][i]);
    }
    track_relations({c}, {(const uint32_t* const*)d_tr}, &log_size, (const uint32_t* const*)d_pp, drel.as<DevRelations>(), hrel, nullptr,
                    relation_mask ? relation_mask : 0xFFu, entries, cap, n_total, nullptr, st);
    CM_HIP(hipStreamSynchronize(st));
  });
}
}  // extern "C"
