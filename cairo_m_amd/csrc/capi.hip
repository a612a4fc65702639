// extern "C" boundary of libcairom_hip.so (declared in include/cairom_hip.h).
// Thin wrappers: translate opaque handles into device pointers, upload pointer arrays, call the
// engine, map C++ exceptions to status codes + a thread-local error string.
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "fft_pass.hpp"
#include "merkle_tree.hpp"
#include "framing.hpp"
#include "abi.hpp"
#include <string.h>
#include <stdio.h>
#include <string>
#include <atomic>
#include <mutex>

using namespace cm;

// ---- process-wide framing switches (framing.hpp) -----------------------------------------------------------------------
namespace cm {
namespace {
std::mutex g_framing_mu;
Framing g_framing;
std::atomic<bool> g_framing_init{false};
int g_framing_users = 0;   // provers / verifiers alive (guarded by g_framing_mu)
}  // namespace
const Framing& framing() {
  if (!g_framing_init) {
    std::lock_guard<std::mutex> lk(g_framing_mu);
    if (!g_framing_init) {
      Framing f;
      if (const char* e = getenv("CM_FRAMING")) {
        const std::string err = Framing::parse(e, f);
        // a proof made under a framing the caller did not ask for is a wrong proof: refuse to run (every entry point reports it)
        if (!err.empty()) throw CmError(1, "CM_FRAMING: " + err);
      }
      g_framing = f;
      g_framing_init = true;
    }
  }
  return g_framing;
}
std::string set_framing(const char* spec) {
  Framing f;
  const std::string err = Framing::parse(spec, f);
  if (!err.empty()) return err;
  try { (void)framing(); } catch (const CmError&) { /* a malformed CM_FRAMING is replaced by this explicit setting */ }
  std::lock_guard<std::mutex> lk(g_framing_mu);
  if (g_framing_users > 0) return "framing: a proof or a verification is in flight; the setting can only change between them";
  g_framing = f;
  g_framing_init = true;
  return "";
}
FramingUse::FramingUse() {
  (void)framing();
  std::lock_guard<std::mutex> lk(g_framing_mu);
  g_framing_users++;
}
FramingUse::~FramingUse() {
  std::lock_guard<std::mutex> lk(g_framing_mu);
  g_framing_users--;
}
}  // namespace cm

namespace {
thread_local std::string g_last_error;
std::mutex g_init_mu;
bool g_inited = false;

std::vector<uint32_t*> ptrs(const cm_handle* hs, uint32_t n) {
  std::vector<uint32_t*> v(n);
  for (uint32_t i = 0; i < n; i++) v[i] = as_words(hs[i]);
  return v;
}
}  // namespace

extern "C" {

int32_t cm_set_last_error(const char* msg) {
  g_last_error = msg;
  return 1;
}

int32_t cm_last_error(char* buf, size_t buf_len) {
  if (!buf || !buf_len) return (int32_t)g_last_error.size();
  size_t n = g_last_error.size() < buf_len - 1 ? g_last_error.size() : buf_len - 1;
  memcpy(buf, g_last_error.data(), n);
  buf[n] = 0;
  return (int32_t)n;
}

int32_t cm_init(int32_t device) {
  return abi_guard_bound([&] {
    std::lock_guard<std::mutex> lk(g_init_mu);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
      throw CmError(3, "cm_init: no HIP device available (libcairom_hip has no CPU fallback)");
    CM_CHECK(device >= 0 && device < ndev, "cm_init: device index out of range");
    CM_HIP(hipSetDevice(device));
    set_library_device(device);
    g_inited = true;
  });
}
int32_t cm_shutdown(void) {
  return abi_guard_bound([&] {
    std::lock_guard<std::mutex> lk(g_init_mu);
    if (g_inited) {
      CM_HIP(hipDeviceSynchronize());
      pool_trim();
    }
    g_inited = false;
  });
}
int32_t cm_pool_trim(void) {
  return abi_guard_bound([&] {
    bind_thread_to_library_device();
    CM_HIP(hipStreamSynchronize(thread_main_stream()));
    pool_trim();
  });
}
int32_t cm_device_mem_info(uint64_t* free_bytes, uint64_t* total_bytes) {
  return abi_guard_bound([&] {
    CM_CHECK(free_bytes && total_bytes, "cm_device_mem_info: null output");
    bind_thread_to_library_device();
    size_t f = 0, t = 0;
    CM_HIP(hipMemGetInfo(&f, &t));
    *free_bytes = f;
    *total_bytes = t;
  });
}
int32_t cm_stream_create(cm_stream_t* out) {
  return abi_guard_bound([&] {
    hipStream_t st;
    CM_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    *out = (cm_stream_t)(uintptr_t)st;
  });
}
int32_t cm_stream_destroy(cm_stream_t s) {
  return abi_guard_bound([&] {
    if (!s) return;
    stage_forget_stream(as_stream(s));        // its copies out of this thread's upload ring finish first (pool.hip)
    CM_HIP(hipStreamDestroy(as_stream(s)));
  });
}
int32_t cm_set_cpu_affinity(int32_t mode) {
  return abi_guard_bound([&] {
    CM_CHECK(mode >= 0 && mode <= 2, "cm_set_cpu_affinity: mode must be 0 (never), 1 (scoped to the proving calls) or 2 (sticky)");
    set_cpu_affinity_mode(mode);
  });
}
int32_t cm_get_cpu_affinity(void) { return cpu_affinity_mode(); }
int32_t cm_set_framing(const char* spec) {
  return abi_guard_bound([&] {
    const std::string err = set_framing(spec);
    if (!err.empty()) throw CmError(1, err);
  });
}
int32_t cm_get_framing(char* buf, size_t buf_len) {
  std::string d;
  try { d = framing().describe(); }
  catch (const std::exception& e) { g_last_error = e.what(); return -1; }   // a malformed CM_FRAMING: nothing is in force
  if (!buf || !buf_len) return (int32_t)d.size();
  const size_t n = d.size() < buf_len - 1 ? d.size() : buf_len - 1;
  memcpy(buf, d.data(), n);
  buf[n] = 0;
  return (int32_t)n;
}
int32_t cm_stream_sync(cm_stream_t s) {
  return abi_guard_bound([&] { CM_HIP(hipStreamSynchronize(as_stream(s))); });
}

int32_t cm_col_alloc(uint64_t n_u32, cm_handle* out) {
  return abi_guard_bound([&] {
    void* p = nullptr;
    CM_HIP(hipMalloc(&p, (n_u32 ? n_u32 : 1) * 4));
    *out = (cm_handle)(uintptr_t)p;
  });
}
int32_t cm_col_free(cm_handle h) {
  return abi_guard_bound([&] { if (h) CM_HIP(hipFree(as_words(h))); });
}
int32_t cm_col_h2d(cm_handle h, const uint32_t* src, uint64_t n, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_HIP(hipMemcpyAsync(as_words(h), src, n * 4, hipMemcpyHostToDevice, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_col_d2h(cm_handle h, uint32_t* dst, uint64_t n, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_HIP(hipMemcpyAsync(dst, as_words(h), n * 4, hipMemcpyDeviceToHost, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
// Column<T>::{at, set, clone} of a Rust-side backend: element ranges and device-to-device copies
int32_t cm_col_read(cm_handle h, uint64_t offset_u32, uint32_t* dst, uint64_t n, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(h && (dst || !n), "cm_col_read: null column / destination");
    CM_HIP(hipMemcpyAsync(dst, as_words(h) + offset_u32, n * 4, hipMemcpyDeviceToHost, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_col_write(cm_handle h, uint64_t offset_u32, const uint32_t* src, uint64_t n, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(h && (src || !n), "cm_col_write: null column / source");
    CM_HIP(hipMemcpyAsync(as_words(h) + offset_u32, src, n * 4, hipMemcpyHostToDevice, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_col_copy(cm_handle dst, cm_handle src, uint64_t n, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(dst && src, "cm_col_copy: null column");
    CM_HIP(hipMemcpyAsync(as_words(dst), as_words(src), n * 4, hipMemcpyDeviceToDevice, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_bit_reverse(const cm_handle* cols, uint32_t n_cols, uint32_t log_n, cm_stream_t s) {
  return abi_guard_bound([&] {
    DevBuf d = upload(ptrs(cols, n_cols), as_stream(s));
    bit_reverse_columns(d.as<uint32_t*>(), n_cols, log_n, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}

int32_t cm_twiddles_precompute(uint32_t log_size, cm_handle* tw_out) {
  return abi_guard_bound([&] {
    Twiddles* t = twiddles_create(log_size, 0);
    CM_HIP(hipStreamSynchronize(0));
    *tw_out = (cm_handle)(uintptr_t)t;
  });
}
int32_t cm_twiddles_free(cm_handle tw) {
  return abi_guard_bound([&] { twiddles_destroy((Twiddles*)(uintptr_t)tw); });
}
int32_t cm_interpolate(const cm_handle* cols, uint32_t n_cols, uint32_t log_n, cm_handle tw, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(tw, "cm_interpolate: null twiddles");
    DevBuf d = upload(ptrs(cols, n_cols), as_stream(s));
    interpolate(d.as<uint32_t*>(), n_cols, log_n, *(Twiddles*)(uintptr_t)tw, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_evaluate(const cm_handle* coeffs, uint32_t n_cols, uint32_t log_n, uint32_t log_out, cm_handle tw,
                    const cm_handle* out, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(tw, "cm_evaluate: null twiddles");
    DevBuf ds = upload(ptrs(coeffs, n_cols), as_stream(s));
    DevBuf dd = upload(ptrs(out, n_cols), as_stream(s));
    evaluate(ds.as<const uint32_t*>(), dd.as<uint32_t*>(), n_cols, log_n, log_out, *(Twiddles*)(uintptr_t)tw, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_interpolate_extend(const cm_handle* evals, const cm_handle* coeffs, const cm_handle* lde, uint32_t n_cols, uint32_t log_n,
                              cm_handle tw, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(tw, "cm_interpolate_extend: null twiddles");
    DevBuf de = upload(ptrs(evals, n_cols), as_stream(s));
    DevBuf dc = upload(ptrs(coeffs, n_cols), as_stream(s));
    DevBuf dl = upload(ptrs(lde, n_cols), as_stream(s));
    interpolate_extend(de.as<const uint32_t*>(), dc.as<uint32_t*>(), dl.as<uint32_t*>(), n_cols, log_n, *(Twiddles*)(uintptr_t)tw, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_fft_plan(uint32_t log_n, uint32_t out[8][4], uint32_t* n_passes) {
  return abi_guard_bound([&] {
    CM_CHECK(out && n_passes, "cm_fft_plan: null output");
    CM_CHECK(log_n >= 1 && log_n <= 28, "cm_fft_plan: log size out of range (1..28)");
    static_assert(FFT_MAX_PASSES == 8, "cm_fft_plan's out[8][4]");
    FftPassShape p[FFT_MAX_PASSES];
    const uint32_t np = fft_plan(log_n, p);
    for (uint32_t i = 0; i < np; i++) { out[i][0] = p[i].lo; out[i][1] = p[i].hi; out[i][2] = p[i].tile_log; out[i][3] = p[i].M; }
    *n_passes = np;
  });
}
int32_t cm_fft_extend_fused(uint32_t log_n, uint32_t* fused) {
  return abi_guard_bound([&] {
    CM_CHECK(fused, "cm_fft_extend_fused: null output");
    CM_CHECK(log_n >= 1 && log_n <= 27, "cm_fft_extend_fused: log size out of range (1..27)");
    *fused = fft_extend_fused(log_n) ? 1u : 0u;
  });
}
int32_t cm_eval_at_point(const cm_handle* coeffs, uint32_t n_cols, uint32_t log_n, const uint32_t pt_xy[8],
                         uint32_t* out, cm_stream_t s) {
  return abi_guard_bound([&] {
    DevBuf ds = upload(ptrs(coeffs, n_cols), as_stream(s));
    DevBuf scratch(eval_at_point_scratch_words(n_cols, log_n) * 4);
    DevBuf dout((size_t)n_cols * 16);
    eval_at_point_batch(ds.as<const uint32_t*>(), n_cols, log_n, QM31::from_u32(pt_xy), QM31::from_u32(pt_xy + 4),
                        scratch.u32(), dout.u32(), as_stream(s));
    CM_HIP(hipMemcpyAsync(out, dout.p, (size_t)n_cols * 16, hipMemcpyDeviceToHost, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}

int32_t cm_merkle_commit_layer(uint32_t log_size, cm_handle prev_layer, const cm_handle* cols, uint32_t n_cols,
                               cm_handle out_hashes, cm_stream_t s) {
  return abi_guard_bound([&] {
    DevBuf dc = upload(ptrs(cols, n_cols), as_stream(s));
    merkle_layer(log_size, as_words(prev_layer), dc.as<const uint32_t*>(), n_cols, as_words(out_hashes), as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
int32_t cm_merkle_commit(const cm_handle* cols, const uint32_t* col_logs, uint32_t n_cols, uint8_t root[32],
                         cm_stream_t s) {
  return abi_guard_bound([&] {
    std::vector<const uint32_t*> c(n_cols);
    std::vector<uint32_t> logs(col_logs, col_logs + n_cols);
    for (uint32_t i = 0; i < n_cols; i++) c[i] = as_words(cols[i]);
    MerkleTree t;
    t.commit(c, logs, as_stream(s));
    t.root(root, as_stream(s));
  });
}
int32_t cm_merkle_commit_layers(const cm_handle* cols, const uint32_t* col_logs, uint32_t n_cols, uint8_t root[32], uint32_t* layers_out,
                                uint64_t cap_words, cm_stream_t s) {
  return abi_guard_bound([&] {
    CM_CHECK(root && layers_out, "cm_merkle_commit_layers: null output");
    std::vector<const uint32_t*> c(n_cols);
    std::vector<uint32_t> logs(col_logs, col_logs + n_cols);
    for (uint32_t i = 0; i < n_cols; i++) c[i] = as_words(cols[i]);
    MerkleTree t;
    t.commit(c, logs, as_stream(s));
    t.root(root, as_stream(s));   // (waits for the stream)
    const size_t max_log = t.layers.size() - 1;
    CM_CHECK(cap_words >= (((uint64_t)2 << max_log) - 1) * 8, "cm_merkle_commit_layers: output buffer too small");
    // the buffers the decommitment gathers from, as they are: largest layer first
    uint32_t* dst = layers_out;
    for (size_t l = max_log + 1; l-- > 0;) {
      const size_t bytes = (size_t)32 << l;
      CM_CHECK(t.layers[l].p && t.layers[l].bytes >= bytes, "cm_merkle_commit_layers: the commitment left a layer without a buffer");
      CM_HIP(hipMemcpy(dst, t.layers[l].p, bytes, hipMemcpyDeviceToHost));
      dst += (size_t)8 << l;
    }
  });
}
int32_t cm_merkle_plan(const uint32_t* col_logs, uint32_t n_cols, uint32_t out[][CM_MERKLE_PLAN_WORDS], uint32_t cap_launches,
                       uint32_t* n_launches) {
  return abi_guard_bound([&] {
    CM_CHECK(out && n_launches && (col_logs || !n_cols), "cm_merkle_plan: null argument");
    static_assert(CM_MERKLE_PLAN_WORDS == 9 + MERKLE_PLAN_MAX_LAYERS, "cm_merkle_plan's record");
    // MerkleTree::prepare's order: by size, descending (only the logs matter here)
    std::vector<uint32_t> logs(col_logs, col_logs + n_cols);
    for (uint32_t l : logs) CM_CHECK(l < 32, "merkle tree: column of 2^32 rows or more");
    std::stable_sort(logs.begin(), logs.end(), [](uint32_t a, uint32_t b) { return a > b; });
    MerkleLaunchPlan recs[MERKLE_PLAN_MAX_LAUNCHES];
    const uint32_t n = merkle_plan(logs.data(), logs.size(), recs);
    CM_CHECK(n <= cap_launches, "cm_merkle_plan: output buffer too small");
    for (uint32_t i = 0; i < n; i++) {
      const MerkleLaunchPlan& r = recs[i];
      uint32_t* w = out[i];
      memset(w, 0, sizeof(uint32_t) * CM_MERKLE_PLAN_WORDS);
      w[0] = r.kind; w[1] = r.hi; w[2] = r.lo; w[3] = r.has_prev; w[4] = r.narrow_prev; w[5] = r.narrow_nc; w[6] = r.npw;
      w[7] = r.wide_mask; w[8] = r.col_begin;
      for (uint32_t k = 0; k <= r.hi - r.lo; k++) w[9 + k] = r.ncols[k];
    }
    *n_launches = n;
  });
}
int32_t cm_merkle_layer_npw(uint32_t log_size, uint32_t has_prev, uint32_t n_cols, uint32_t* npw) {
  return abi_guard_bound([&] {
    CM_CHECK(npw, "cm_merkle_layer_npw: null output");
    CM_CHECK(log_size < 32, "cm_merkle_layer_npw: log size out of range");
    *npw = merkle_narrow_npw(log_size, has_prev != 0, n_cols);
  });
}
int32_t cm_grind(const uint8_t digest[32], uint32_t pow_bits, uint64_t* nonce_out, cm_stream_t s) {
  return abi_guard_bound([&] { *nonce_out = grind_gpu(digest, pow_bits, as_stream(s)); });
}

}  // extern "C"
