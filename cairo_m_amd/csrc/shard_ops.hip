// extern "C" op-level entries for the forms of the FRI and quotient kernels that only a whole proof reached (declared in
// include/cairom_hip.h): the row-range folds and fold + leaves of the sharded prover, the quotient launch on a row range, with the
// leaf hashes, and on coefficients that k_quotient_coeffs computed on the device, and the data-movement kernels of
// kernels_shard.hip.  Every entry checks its arguments before the first device call, calls the host wrapper the provers call,
// unchanged, and synchronises the stream.  In a whole proof the plan picks the ranges and the transcript the challenges; here the
// tests pick them.
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "fri_kernels.hpp"
#include "shard_kernels.hpp"
#include "abi.hpp"
#include <vector>
#include <string>
#include <cstring>

using namespace cm;

static_assert(CM_QUOT_PATH_ROWS2 == QUOT_ROWS2 && CM_QUOT_PATH_ROWS4 == QUOT_ROWS4 && CM_QUOT_PATH_ROWS2_LEAF == QUOT_ROWS2_LEAF &&
              CM_QUOT_PATH_ONE_ROW == QUOT_ONE_ROW && CM_QUOT_PATH_SLICES8 == QUOT_SLICES8 && CM_QUOT_PATH_SLICES64 == QUOT_SLICES64,
              "the header's path words are launch_quotients' own");

namespace {
bool canonical4(const uint32_t* w) { return w[0] < P && w[1] < P && w[2] < P && w[3] < P; }
}  // namespace

extern "C" {

int32_t cm_fri_fold_rows_op(const cm_handle out[4], const cm_handle src[4], const uint32_t alpha[4], uint32_t log_n, cm_handle tw,
                            uint32_t i0, uint32_t n_out, uint32_t flags, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(out && src && alpha, "cm_fri_fold_rows_op: null argument");
    CM_CHECK(tw, "cm_fri_fold_rows_op: null twiddles");
    for (int k = 0; k < 4; k++) CM_CHECK(out[k] && src[k], "cm_fri_fold_rows_op: null column handle");
    CM_CHECK((flags & ~(uint32_t)(CM_FOLD_CIRCLE | CM_FOLD_ACCUMULATE | CM_FOLD_ALPHA_ON_DEVICE)) == 0, "cm_fri_fold_rows_op: unknown flag");
    const bool circle = (flags & CM_FOLD_CIRCLE) != 0, accumulate = (flags & CM_FOLD_ACCUMULATE) != 0;
    CM_CHECK(circle || !accumulate, "cm_fri_fold_rows_op: only the circle fold accumulates");
    CM_CHECK(canonical4(alpha), "cm_fri_fold_rows_op: a challenge word is not below P");
    const Twiddles& T = *(Twiddles*)(uintptr_t)tw;
    // (the wrappers' own bounds, stated here so that the refusal carries this entry's name)
    CM_CHECK(log_n >= (circle ? 2u : 1u) && log_n + (circle ? 0u : 1u) <= T.R, "cm_fri_fold_rows_op: log_n outside what the twiddles cover");
    CM_CHECK(n_out >= 1, "cm_fri_fold_rows_op: n_out is 0");
    CM_CHECK((uint64_t)i0 + n_out <= ((uint64_t)1 << (log_n - 1)), "cm_fri_fold_rows_op: i0 + n_out beyond the 2^(log_n-1) outputs");

    hipStream_t st = as_stream(s);
    uint32_t* d[4]; const uint32_t* c[4];
    for (int k = 0; k < 4; k++) { d[k] = as_words(out[k]); c[k] = as_words(src[k]); }
    DevBuf d_a;
    // the challenge the kernel must NOT read is a different one, so that taking it from the wrong place shows
    QM31 a_arg = QM31::from_u32(alpha);
    if (flags & CM_FOLD_ALPHA_ON_DEVICE) {
      d_a = upload(std::vector<uint32_t>(alpha, alpha + 4), st);
      a_arg = QM31(M31(1), M31(2), M31(3), M31(4));
    }
    const uint32_t* d_alpha = (flags & CM_FOLD_ALPHA_ON_DEVICE) ? d_a.u32() : nullptr;
    if (circle) fold_circle_into_line_rows(d, c, log_n, T, a_arg, accumulate, i0, n_out, st, d_alpha);
    else fold_line_rows(d, c, log_n, T, a_arg, i0, n_out, st, d_alpha);
    CM_HIP(hipStreamSynchronize(st));
  });
}

int32_t cm_fri_fold_leaves_rows_op(const cm_handle* in, const cm_handle* circle, const uint32_t* alpha, const uint32_t* alpha_circle,
                                   uint32_t log_n, cm_handle tw, uint32_t row0, uint32_t n_rows, const cm_handle out[4],
                                   cm_handle leaf_hashes, uint32_t* fused_out, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(tw, "cm_fri_fold_leaves_rows_op: null twiddles");
    CM_CHECK(out && leaf_hashes && fused_out, "cm_fri_fold_leaves_rows_op: null argument");
    CM_CHECK(in || circle, "cm_fri_fold_leaves_rows_op: neither a line nor a circle source");
    CM_CHECK((in == nullptr) == (alpha == nullptr) && (circle == nullptr) == (alpha_circle == nullptr),
             "cm_fri_fold_leaves_rows_op: every source comes with its challenge");
    for (int k = 0; k < 4; k++) CM_CHECK(out[k] && (!in || in[k]) && (!circle || circle[k]), "cm_fri_fold_leaves_rows_op: null column handle");
    CM_CHECK((!alpha || canonical4(alpha)) && (!alpha_circle || canonical4(alpha_circle)), "cm_fri_fold_leaves_rows_op: a challenge word is not below P");
    const Twiddles& T = *(Twiddles*)(uintptr_t)tw;
    CM_CHECK(log_n >= 2 && log_n + (in ? 1u : 0u) <= T.R, "cm_fri_fold_leaves_rows_op: log_n outside what the twiddles cover");
    CM_CHECK(n_rows >= 1, "cm_fri_fold_leaves_rows_op: n_rows is 0");
    CM_CHECK((n_rows & (n_rows - 1)) == 0, "cm_fri_fold_leaves_rows_op: n_rows is not a power of two (the leaf layer of a slice is one tree layer)");
    CM_CHECK((uint64_t)row0 + n_rows <= ((uint64_t)1 << (log_n - 1)), "cm_fri_fold_leaves_rows_op: row0 + n_rows beyond the 2^(log_n-1) outputs");

    hipStream_t st = as_stream(s);
    uint32_t* d[4]; const uint32_t* c[4] = {nullptr, nullptr, nullptr, nullptr}; const uint32_t* q[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; k++) { d[k] = as_words(out[k]); if (in) c[k] = as_words(in[k]); if (circle) q[k] = as_words(circle[k]); }
    std::vector<uint32_t> a8(8, 0);
    if (alpha) memcpy(a8.data(), alpha, 16);
    if (alpha_circle) memcpy(a8.data() + 4, alpha_circle, 16);
    DevBuf d_a = upload(a8, st);
    const bool fused = in ? fold_line_leaf(d, c, circle ? q : nullptr, log_n, T, st, d_a.u32(), circle ? d_a.u32() + 4 : nullptr, as_words(leaf_hashes), row0, n_rows)
                          : fold_circle_leaf(d, q, log_n, T, st, d_a.u32() + 4, as_words(leaf_hashes), row0, n_rows);
    if (!fused) {
      // what the sharded prover does when the fused wrapper declines: the row-range folds (device challenges), then the leaf layer
      // of the slice's subtree
      bool blank = true;
      if (in) { fold_line_rows(d, c, log_n, T, QM31(), row0, n_rows, st, d_a.u32()); blank = false; }
      if (circle) fold_circle_into_line_rows(d, q, log_n, T, QM31(), !blank, row0, n_rows, st, d_a.u32() + 4);
      std::vector<const uint32_t*> cols(d, d + 4);
      DevBuf d_cols = upload(cols, st);
      uint32_t lg = 0;
      while ((1u << lg) < n_rows) lg++;
      merkle_layer(lg, nullptr, d_cols.as<const uint32_t*>(), 4, as_words(leaf_hashes), st);
    }
    CM_HIP(hipStreamSynchronize(st));
    *fused_out = fused ? 1u : 0u;
  });
}

int32_t cm_accumulate_quotients_rows_op(uint32_t log_size, const cm_handle* cols, uint32_t n_cols, const cm_sample_batches* b,
                                        const uint32_t random_coeff[4], const cm_handle out[4], cm_handle tw, uint32_t row0, uint32_t n_rows,
                                        cm_handle leaf_hashes, uint32_t device_coeffs, const uint32_t* sample_idx, uint32_t n_samples,
                                        uint32_t* path_out, uint32_t* coef_c_out, uint32_t* sums_out, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(tw, "cm_accumulate_quotients_rows_op: null twiddles");
    CM_CHECK(cols && b && random_coeff && out && path_out, "cm_accumulate_quotients_rows_op: null argument");
    CM_CHECK(b->points && b->batch_off && b->col_index && b->values, "cm_accumulate_quotients_rows_op: null argument");
    CM_CHECK(n_cols >= 1, "cm_accumulate_quotients_rows_op: n_cols is 0");
    CM_CHECK(n_cols <= (1u << 16), "cm_accumulate_quotients_rows_op: more than 65536 columns");
    CM_CHECK(b->n_batches >= 1, "cm_accumulate_quotients_rows_op: n_batches is 0");
    CM_CHECK(b->n_batches <= (1u << 16), "cm_accumulate_quotients_rows_op: more than 65536 batches");
    for (uint32_t i = 0; i < n_cols; i++) CM_CHECK(cols[i], "cm_accumulate_quotients_rows_op: null column handle");
    for (int k = 0; k < 4; k++) CM_CHECK(out[k], "cm_accumulate_quotients_rows_op: null column handle");
    CM_CHECK(canonical4(random_coeff), "cm_accumulate_quotients_rows_op: a coefficient word is not below P");
    CM_CHECK(b->batch_off[0] == 0, "cm_accumulate_quotients_rows_op: batch_off does not start at 0");
    for (uint32_t k = 0; k < b->n_batches; k++) {
      CM_CHECK(b->batch_off[k + 1] > b->batch_off[k], "cm_accumulate_quotients_rows_op: a batch with no entry");
      CM_CHECK(canonical4(b->points + 8 * k) && canonical4(b->points + 8 * k + 4), "cm_accumulate_quotients_rows_op: a point word is not below P");
    }
    const uint32_t n_entries = b->batch_off[b->n_batches];
    CM_CHECK(n_entries <= (1u << 24), "cm_accumulate_quotients_rows_op: more than 2^24 entries");
    for (uint32_t e = 0; e < n_entries; e++) CM_CHECK(b->col_index[e] < n_cols, "cm_accumulate_quotients_rows_op: column index out of range");
    if (device_coeffs) {
      CM_CHECK(sample_idx && coef_c_out && sums_out, "cm_accumulate_quotients_rows_op: device_coeffs without sample_idx / coef_c_out / sums_out");
      CM_CHECK(n_samples >= 1, "cm_accumulate_quotients_rows_op: n_samples is 0");
      CM_CHECK(n_samples <= (1u << 24), "cm_accumulate_quotients_rows_op: more than 2^24 samples");
      for (uint32_t e = 0; e < n_entries; e++) CM_CHECK(sample_idx[e] < n_samples, "cm_accumulate_quotients_rows_op: sample index out of range");
    }
    for (uint32_t v = 0; v < (device_coeffs ? n_samples : n_entries); v++)
      CM_CHECK(canonical4(b->values + 4 * (size_t)v), "cm_accumulate_quotients_rows_op: a sampled-value word is not below P");
    const Twiddles& T = *(Twiddles*)(uintptr_t)tw;
    CM_CHECK(log_size >= 1 && log_size <= T.R && log_size <= 30, "cm_accumulate_quotients_rows_op: log_size outside what the twiddles cover");
    CM_CHECK(n_rows >= 1 || row0 == 0, "cm_accumulate_quotients_rows_op: n_rows is 0 (the whole domain) with a row0");
    CM_CHECK((uint64_t)row0 + n_rows <= ((uint64_t)1 << log_size), "cm_accumulate_quotients_rows_op: row0 + n_rows beyond the 2^log_size rows");

    std::vector<const uint32_t*> c(n_cols), ep(n_entries);
    for (uint32_t i = 0; i < n_cols; i++) c[i] = as_words(cols[i]);
    for (uint32_t e = 0; e < n_entries; e++) ep[e] = c[b->col_index[e]];
    QuotientArgs a;
    a.log_size = log_size; a.n_batches = b->n_batches; a.row0 = row0; a.n_rows = n_rows;
    if (leaf_hashes) {
      a.entry_cols = ep.data();   // (the predicate only asks whether the launch has resolved entry columns)
      CM_CHECK(quotient_leaf_serves(a), "cm_accumulate_quotients_rows_op: leaf hashes asked for a launch the two-rows kernel does not serve");
    }

    hipStream_t st = as_stream(s);
    const QM31 rc = QM31::from_u32(random_coeff);
    std::vector<QuotientBatch> qb(b->n_batches);
    std::vector<uint32_t> coef_c((size_t)4 * n_entries, 0);
    for (uint32_t k = 0; k < b->n_batches; k++) {
      memset(&qb[k], 0, sizeof(QuotientBatch));
      qb[k].begin = b->batch_off[k]; qb[k].end = b->batch_off[k + 1];
      memcpy(qb[k].point, b->points + 8 * k, 32);
      if (device_coeffs) continue;
      // the host form of cm_accumulate_quotients
      const QM31 py = QM31::from_u32(b->points + 8 * k + 4), cdiff = conj_u(py) - py;
      QM31 alpha(M31(1)), sum_a, sum_b;
      for (uint32_t e = qb[k].begin; e < qb[k].end; e++) {
        const QM31 v = QM31::from_u32(b->values + 4 * (size_t)e);
        alpha = alpha * rc;
        const QM31 aa = conj_u(v) - v;
        sum_a += alpha * aa;
        sum_b += alpha * (v * cdiff - aa * py);
        (alpha * cdiff).to_u32(&coef_c[4 * (size_t)e]);
      }
      sum_a.to_u32(qb[k].sum_a);
      sum_b.to_u32(qb[k].sum_b);
      qpow(rc, qb[k].end - qb[k].begin).to_u32(qb[k].batch_coeff);
    }
    std::vector<uint32_t*> o(4);
    for (int k = 0; k < 4; k++) o[k] = as_words(out[k]);
    DevBuf dcols = upload(c, st), dci = upload(std::vector<uint32_t>(b->col_index, b->col_index + n_entries), st), dcc = upload(coef_c, st),
           dqb = upload(qb, st), dout = upload(o, st), dep = upload(ep, st);
    DevBuf d_si, d_samples, d_jobs;
    if (device_coeffs) {
      // one job per batch, pointing into the device copies, as QuotientPlan::bind lays them out for the provers
      d_si = upload(std::vector<uint32_t>(sample_idx, sample_idx + n_entries), st);
      d_samples = upload(std::vector<uint32_t>(b->values, b->values + 4 * (size_t)n_samples), st);
      std::vector<QuotientCoefJob> jobs(b->n_batches);
      for (uint32_t k = 0; k < b->n_batches; k++) jobs[k] = QuotientCoefJob{dqb.as<QuotientBatch>() + k, dcc.u32(), d_si.u32()};
      d_jobs = upload(jobs, st);
      quotient_coeffs(d_jobs.as<QuotientCoefJob>(), b->n_batches, d_samples.u32(), rc, st);
    }
    a.tw = view(T); a.cols = dcols.as<const uint32_t*>();
    a.col_index = dci.u32(); a.coef_c = dcc.u32(); a.batches = dqb.as<QuotientBatch>();
    a.out = dout.as<uint32_t*>();
    a.entry_cols = dep.as<const uint32_t*>();
    a.leaf_hashes = as_words(leaf_hashes);
    const QuotientPath path = launch_quotients(a, (double)n_cols, st);
    if (device_coeffs) {
      CM_HIP(hipMemcpyAsync(coef_c_out, dcc.p, (size_t)16 * n_entries, hipMemcpyDeviceToHost, st));
      CM_HIP(hipMemcpyAsync(qb.data(), dqb.p, qb.size() * sizeof(QuotientBatch), hipMemcpyDeviceToHost, st));
    }
    CM_HIP(hipStreamSynchronize(st));
    if (device_coeffs)
      for (uint32_t k = 0; k < b->n_batches; k++) {
        memcpy(sums_out + 12 * (size_t)k, qb[k].sum_a, 16);
        memcpy(sums_out + 12 * (size_t)k + 4, qb[k].sum_b, 16);
        memcpy(sums_out + 12 * (size_t)k + 8, qb[k].batch_coeff, 16);
      }
    *path_out = (uint32_t)path;
  });
}

int32_t cm_pack_parity_op(cm_handle src, cm_handle dst, uint32_t half_len, uint32_t parity, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(src && dst, "cm_pack_parity_op: null column handle");
    CM_CHECK(half_len >= 1, "cm_pack_parity_op: half_len is 0");
    CM_CHECK(half_len <= (1u << 30), "cm_pack_parity_op: half_len above 2^30");
    CM_CHECK(parity <= 1, "cm_pack_parity_op: parity is neither 0 nor 1");
    pack_parity(as_words(src), as_words(dst), half_len, parity, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}

int32_t cm_halo_build_op(cm_handle even_half, cm_handle odd_half, uint32_t even_src, uint32_t odd_src, uint32_t row0, uint32_t len,
                         uint32_t n, uint32_t trace_log, uint32_t log_ranks, cm_handle out, uint32_t* err_out, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(even_half && odd_half && out, "cm_halo_build_op: null column handle");
    CM_CHECK(err_out, "cm_halo_build_op: null argument");
    CM_CHECK(n >= 2 && n <= 30, "cm_halo_build_op: n outside 2..30");
    CM_CHECK(trace_log >= 1 && trace_log <= n, "cm_halo_build_op: trace_log outside 1..n");
    CM_CHECK(log_ranks >= 1 && log_ranks < n, "cm_halo_build_op: log_ranks outside 1..n-1 (a slice has two rows at least)");
    CM_CHECK(even_src < (1u << log_ranks) && odd_src < (1u << log_ranks), "cm_halo_build_op: a source rank outside the 2^log_ranks ranks");
    CM_CHECK(len >= 1, "cm_halo_build_op: len is 0");
    CM_CHECK((uint64_t)row0 + len <= ((uint64_t)1 << n), "cm_halo_build_op: row0 + len beyond the 2^n rows");
    hipStream_t st = as_stream(s);
    DevBuf d_err(4);
    CM_HIP(hipMemsetAsync(d_err.p, 0, 4, st));
    halo_build(as_words(even_half), as_words(odd_half), even_src, odd_src, row0, len, n, trace_log, log_ranks, as_words(out), d_err.u32(), st);
    CM_HIP(hipMemcpyAsync(err_out, d_err.p, 4, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
  });
}

int32_t cm_sum_copies_op(cm_handle in, uint32_t n_copies, uint64_t stride, uint64_t words, cm_handle out, uint32_t modular, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(in && out, "cm_sum_copies_op: null column handle");
    CM_CHECK(n_copies >= 1, "cm_sum_copies_op: n_copies is 0");
    CM_CHECK(n_copies <= 1024, "cm_sum_copies_op: more than 1024 copies");
    CM_CHECK(words >= 1, "cm_sum_copies_op: words is 0");
    CM_CHECK(words <= ((uint64_t)1 << 30), "cm_sum_copies_op: words above 2^30");
    CM_CHECK(stride >= words && stride <= ((uint64_t)1 << 30), "cm_sum_copies_op: stride below words (the copies overlap) or above 2^30");
    sum_copies(as_words(in), n_copies, stride, words, as_words(out), modular != 0, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}

int32_t cm_copy_segments_op(const cm_handle* src, const cm_handle* dst, const uint64_t* words, uint32_t n_segs, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(n_segs == 0 || (src && dst && words), "cm_copy_segments_op: null argument");
    CM_CHECK(n_segs <= 65535, "cm_copy_segments_op: more than 65535 segments (one block row each)");
    std::vector<CopySeg> segs(n_segs);
    for (uint32_t i = 0; i < n_segs; i++) {
      CM_CHECK(words[i] <= ((uint64_t)1 << 30), "cm_copy_segments_op: a segment above 2^30 words");
      CM_CHECK(words[i] == 0 || (src[i] && dst[i]), "cm_copy_segments_op: null column handle");
      segs[i] = CopySeg{as_words(src[i]), as_words(dst[i]), words[i]};
    }
    copy_segments(segs, as_stream(s));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
  });
}
}
