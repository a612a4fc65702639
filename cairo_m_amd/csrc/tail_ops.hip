// extern "C" entry points that run the device-side proof tail (tail_device.hpp) one kernel at a time, on inputs the caller
// chooses: the production kernels through the production host wrappers (tail_last_layer, tail_grind, tail_tables,
// tail_gather) and the production pinned buffers (tail_pinned_desc, tail_pinned_out, pinned_words).  In a whole proof the
// transcript picks the nonce and the query positions; here the tests pick them (declared in include/cairom_hip.h).
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "tail_device.hpp"
#include "abi.hpp"
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>

using namespace cm;

namespace {
static_assert(CM_TAIL_HDR_WORDS == TAIL_HDR_WORDS && CM_TAIL_SHIFTS == TAIL_MAX_SHIFTS && CM_TAIL_NO_NONCE == TAIL_NO_NONCE,
              "cairom_hip.h restates the tail's constants");
// device channel {digest[8], n_sent}
DevBuf upload_channel(const uint32_t digest[8], hipStream_t st) {
  std::vector<uint32_t> w(digest, digest + 8);
  w.push_back(0);
  return upload(w, st);
}
// DeviceTail::bound_items times the words per item: what the prover sizes its pinned witness buffer by
size_t piece_bound(uint32_t kind, uint32_t k, uint32_t width, uint32_t L0, uint32_t nq) {
  const size_t n = (size_t)std::min<uint64_t>(nq, (uint64_t)1 << (L0 - k));
  return (kind == TD_HASH_F ? 3 * n : n) * (kind == TD_ROWS_U ? width : kind == TD_COORDS_W ? 4u : 8u);
}
}  // namespace

extern "C" {

uint64_t cm_tail_tab_words(uint32_t nq_pad) { return tail_tab_words(nq_pad); }

int32_t cm_tail_grind_op(const uint32_t digest[8], uint32_t bits, uint64_t* nonce_out, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(digest && nonce_out, "cm_tail_grind_op: null argument");
    CM_CHECK(bits <= TAIL_MAX_POW_BITS, "cm_tail_grind_op: bits above TAIL_MAX_POW_BITS (26)");
    DevBuf d_chan = upload_channel(digest, as_stream(s));
    DevBuf d_nonce = upload(std::vector<unsigned long long>{~0ull}, as_stream(s));
    tail_grind(d_chan.u32(), bits, (unsigned long long*)d_nonce.p, as_stream(s));
    unsigned long long got = 0;
    CM_HIP(hipMemcpyAsync(&got, d_nonce.p, 8, hipMemcpyDeviceToHost, as_stream(s)));
    CM_HIP(hipStreamSynchronize(as_stream(s)));
    *nonce_out = got;
  });
}

int32_t cm_tail_tables_op(const uint32_t digest[8], uint64_t nonce, uint32_t n_queries, uint32_t nq_pad, uint32_t log_domain,
                          uint32_t qmask, const cm_tail_piece* pieces, uint32_t n_pieces, uint32_t n_small, cm_tail_tables_out* out,
                          cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(digest && out && (pieces || !n_pieces), "cm_tail_tables_op: null argument");
    CM_CHECK(out->struct_size == sizeof(cm_tail_tables_out), "cm_tail_tables_op: cm_tail_tables_out.struct_size does not match this library");
    CM_CHECK(out->hdr && out->positions && out->tab && (out->offsets || !n_pieces) && (out->words || !out->words_cap),
             "cm_tail_tables_op: null output buffer");
    CM_CHECK(n_queries >= 1 && n_queries <= TAIL_MAX_QUERIES, "cm_tail_tables_op: n_queries outside 1..1024");
    CM_CHECK(nq_pad >= n_queries && nq_pad <= TAIL_MAX_QUERIES && (nq_pad & (nq_pad - 1)) == 0,
             "cm_tail_tables_op: nq_pad must be a power of two in [n_queries, 1024]");
    CM_CHECK(log_domain < TAIL_MAX_SHIFTS, "cm_tail_tables_op: log_domain must be below 32");
    CM_CHECK(n_small <= n_pieces, "cm_tail_tables_op: n_small above the number of pieces");
    CM_CHECK(n_pieces <= (1u << 16), "cm_tail_tables_op: too many pieces");
    size_t n_col_ptrs = 0, bound = 0;
    for (uint32_t d = 0; d < n_pieces; d++) {
      const cm_tail_piece& p = pieces[d];
      CM_CHECK(p.kind <= TD_ROWS_U, "cm_tail_tables_op: unknown piece kind");
      CM_CHECK(p.k <= log_domain, "cm_tail_tables_op: a piece's shift k is above log_domain");
      CM_CHECK(d >= n_small || p.kind != TD_ROWS_U, "cm_tail_tables_op: a row piece in front of n_small");
      CM_CHECK(d < n_small || p.kind == TD_ROWS_U, "cm_tail_tables_op: a hash or coordinate piece behind n_small");
      CM_CHECK(p.kind != TD_HASH_F || p.k >= 1, "cm_tail_tables_op: an F piece needs k >= 1");
      CM_CHECK(p.kind != TD_ROWS_U || (p.width >= 1 && p.width <= (1u << 16)), "cm_tail_tables_op: a row piece's width outside 1..65536");
      CM_CHECK(p.cols, "cm_tail_tables_op: a piece without column handles");
      const uint32_t nh = p.kind == TD_ROWS_U ? p.width : p.kind == TD_COORDS_W ? 4u : 1u;
      for (uint32_t c = 0; c < nh; c++) CM_CHECK(p.cols[c], "cm_tail_tables_op: null column handle");
      if (p.kind == TD_ROWS_U) n_col_ptrs += p.width;
      bound += piece_bound(p.kind, p.k, p.width, log_domain, n_queries);
    }
    CM_CHECK(out->words_cap >= bound, "cm_tail_tables_op: words_cap below the bound of the pieces");
    CM_CHECK(bound < ((size_t)1 << 28), "cm_tail_tables_op: pieces too large");

    hipStream_t st = as_stream(s);
    // the device tables of column pointers of the row pieces (MerkleTree::dcols() in the prover), one upload
    std::vector<const uint32_t*> col_ptrs;
    col_ptrs.reserve(n_col_ptrs);
    for (uint32_t d = n_small; d < n_pieces; d++)
      for (uint32_t c = 0; c < pieces[d].width; c++) col_ptrs.push_back(as_words(pieces[d].cols[c]));
    DevBuf d_cols = upload(col_ptrs, st);
    // the descriptors, as DeviceTail::enqueue builds them
    std::vector<TailDesc> desc;
    desc.reserve(n_pieces);
    size_t col0 = 0;
    for (uint32_t d = 0; d < n_pieces; d++) {
      const cm_tail_piece& p = pieces[d];
      if (p.kind == TD_ROWS_U) {
        desc.push_back(TailDesc{{d_cols.as<const uint32_t*>() + col0, nullptr, nullptr, nullptr}, p.kind, p.k, p.width, 0});
        col0 += p.width;
      } else if (p.kind == TD_COORDS_W) {
        desc.push_back(TailDesc{{as_words(p.cols[0]), as_words(p.cols[1]), as_words(p.cols[2]), as_words(p.cols[3])}, p.kind, p.k, 4, 0});
      } else {
        desc.push_back(TailDesc{{as_words(p.cols[0]), nullptr, nullptr, nullptr}, p.kind, p.k, 8, 0});
      }
    }
    // pinned: descriptors in; {header | positions | witnesses} out
    TailDesc* h_desc = (TailDesc*)tail_pinned_desc(std::max<size_t>(desc.size(), 1) * sizeof(TailDesc));
    if (!desc.empty()) memcpy(h_desc, desc.data(), desc.size() * sizeof(TailDesc));
    uint32_t* ob = (uint32_t*)tail_pinned_out((TAIL_HDR_WORDS + (size_t)nq_pad + bound) * 4);
    uint32_t *hdr = ob, *h_pos = ob + TAIL_HDR_WORDS, *h_out = h_pos + nq_pad;
    memset(hdr, 0xFF, TAIL_HDR_WORDS * 4);
    memset(h_pos, 0, (size_t)nq_pad * 4);
    DevBuf d_desc(desc.size() * sizeof(TailDesc)), d_off(desc.size() * 4), d_tab(tail_tab_words(nq_pad) * 4);
    DevBuf d_chan = upload_channel(digest, st);
    DevBuf d_nonce = upload(std::vector<unsigned long long>{(unsigned long long)nonce}, st);
    CM_HIP(hipMemsetAsync(d_tab.p, 0, tail_tab_words(nq_pad) * 4, st));
    TailTablesArgs a;
    a.chan = d_chan.u32();
    a.nonce = (const unsigned long long*)d_nonce.p;
    a.n_queries = n_queries; a.log_domain = log_domain; a.qmask = qmask;
    a.n_desc = n_pieces;
    a.h_desc = h_desc; a.d_desc = d_desc.as<TailDesc>(); a.d_off = d_off.u32();
    a.tab = d_tab.u32(); a.nq_pad = nq_pad; a.hdr = hdr; a.h_positions = h_pos;
    tail_tables(a, st);
    tail_gather(d_desc.as<TailDesc>(), d_off.u32(), d_tab.u32(), nq_pad, n_small, n_pieces, n_queries, h_out, st);
    CM_HIP(hipMemcpyAsync(out->tab, d_tab.p, tail_tab_words(nq_pad) * 4, hipMemcpyDeviceToHost, st));
    if (n_pieces) CM_HIP(hipMemcpyAsync(out->offsets, d_off.p, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    memcpy(out->hdr, hdr, TAIL_HDR_WORDS * 4);
    memcpy(out->positions, h_pos, (size_t)nq_pad * 4);
    CM_CHECK(hdr[4] <= bound, "cm_tail_tables_op: the device's witness size is above the bound of the pieces");
    if (hdr[4]) memcpy(out->words, h_out, (size_t)hdr[4] * 4);
  });
}

int32_t cm_tail_last_op(const uint32_t digest[8], const cm_handle last[4], uint32_t log_n, uint32_t log_keep, const uint32_t* ar,
                        uint32_t n_ar_words, uint32_t digest_out[8], uint32_t* degree_flag, uint32_t* last_out, uint32_t* ar_out,
                        uint64_t* nonce_cell, cm_stream_t s) {
  return abi_guard([&] {
    CM_CHECK(digest && last && digest_out && degree_flag && last_out && nonce_cell && ((ar && ar_out) || !n_ar_words),
             "cm_tail_last_op: null argument");
    for (int c = 0; c < 4; c++) CM_CHECK(last[c], "cm_tail_last_op: null column handle");
    CM_CHECK(log_n <= 6, "cm_tail_last_op: log_n above 6 (TAIL_MAX_LAST = 64 values)");
    CM_CHECK(log_keep <= log_n, "cm_tail_last_op: log_keep above log_n");
    CM_CHECK(n_ar_words <= PIN_LAST_LAYER - PIN_ALPHAS, "cm_tail_last_op: more than 384 challenge / root words");
    static_assert((4u << 6) <= PIN_LAST_LAYER_END - PIN_LAST_LAYER, "the last layer's pinned slot");
    hipStream_t st = as_stream(s);
    const uint32_t n = 1u << log_n;
    DevBuf d_chan = upload_channel(digest, st);
    DevBuf d_ar = upload(std::vector<uint32_t>(ar, ar + n_ar_words), st);
    DevBuf d_nonce = upload(std::vector<unsigned long long>{0ull}, st);   // (not ~0: the kernel has to arm it)
    uint32_t* hdr = (uint32_t*)tail_pinned_out(TAIL_HDR_WORDS * 4);
    memset(hdr, 0xFF, TAIL_HDR_WORDS * 4);
    TailLastArgs a;
    memset(&a, 0, sizeof(a));
    a.d_ar = d_ar.u32();
    a.n_ar_words = n_ar_words;
    for (int c = 0; c < 4; c++) a.last[c] = as_words(last[c]);
    a.log_n = log_n;
    a.log_keep = log_keep;
    tail_last_twiddles(log_n, &a.ninv, a.xinv);
    a.chan = d_chan.u32();
    a.h_ar = pinned_words() + PIN_ALPHAS;
    a.h_last = pinned_words() + PIN_LAST_LAYER;
    a.hdr = hdr;
    a.nonce = (unsigned long long*)d_nonce.p;
    memset(a.h_ar, 0xFF, (size_t)n_ar_words * 4);
    memset(a.h_last, 0xFF, (size_t)4 * n * 4);
    tail_last_layer(a, st);
    uint32_t chan[9];
    unsigned long long cell = 0;
    CM_HIP(hipMemcpyAsync(chan, d_chan.p, sizeof(chan), hipMemcpyDeviceToHost, st));
    CM_HIP(hipMemcpyAsync(&cell, d_nonce.p, 8, hipMemcpyDeviceToHost, st));
    CM_HIP(hipStreamSynchronize(st));
    CM_CHECK(hdr[TAIL_HDR_LAST_DONE] == 1u, "cm_tail_last_op: the kernel did not set its done word");
    memcpy(digest_out, chan, 32);
    *degree_flag = hdr[6];
    memcpy(last_out, a.h_last, (size_t)4 * n * 4);
    if (n_ar_words) memcpy(ar_out, a.h_ar, (size_t)n_ar_words * 4);
    *nonce_cell = cell;
  });
}

}  // extern "C"
