// Program identity (cm_program_id_entries, cm_proof_program_id, cm_program_ids, cm_proofs_program_ids, cm_run_statement_of): which
// program a proof is about, as one 31-bit word, and what a chain of proofs states — program, registers, roots, inputs, outputs.
//
// The id is Proof::program_id() of the reference (crates/prover/src/lib.rs:75-97): the Poseidon2 root of the partial memory tree
// (adapter/merkle.rs:183-295) that holds only the proof's public program cells.  Those cells are the dense range
// [first, first + n), so the tree is the range fold of mem_range.hpp with no record: a cell becomes its node of depth 28
// (range_cell_node), a child outside the interval at depth d is default[d], and once the interval is one node the same step chains
// it to depth 0.  Clocks do not enter.  The reference unwraps every entry and the root: an absent entry or an empty program is a
// panic there and a refusal (status 1) here.  A present all-zero cell hashes to default[28] and so leaves no trace in the id: that
// is the tree's own property (link.hip counts such cells as `zero only`), not a fault of this code.
//
// Host: cm_program_id_entries / cm_proof_program_id fold in host code, about 4 n + 28 hashes, no device call.
// Device, a batch of programs in one call: the host walks every item once — present flags and addresses are checked there, where
// the message can name the entry, and the value words are gathered behind a table (offset, count, first address, flag per item) —
// ONE upload, two launches whatever the batch holds, ONE download of (id, flag) pairs:
//   k_pid_cells  one lane per cell of the whole batch: its four words range-checked, three Poseidon2 calls -> the node of depth 28.
//                A word that is not below P raises its item's flag word with a plain store (the lane bisects the offsets only then).
//   k_pid_tree   one workgroup of 1024 lanes per item.  While the interval is wider than 1024 nodes the lanes stride over it from
//                one global buffer into the other; the barrier between depths orders the two (they swap roles, so neither is
//                const __restrict__).  After that the level lives in LDS as in k_range_tail, and once the interval is one node
//                lane 0 alone is left hashing the remaining depths.  Lane 0 stores the id and copies the flag beside it.
// Every output word is written by exactly one lane, there is no atomic, and each kernel has one call site of the permutation.
#include "../../include/cairom_hip.h"
#include "program_id.hpp"
#include "mem_open.hpp"
#include "handles.hpp"
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace cm {
namespace {

constexpr uint32_t PID_BLOCK = 256;
// the uploaded table: four runs of n_items words in front of the values (16 n bytes: the values stay 16-byte aligned)
enum : uint32_t { PT_OFF = 0, PT_COUNT = 1, PT_FIRST = 2, PT_FLAG = 3, PT_RUNS = 4 };

static_assert(sizeof(cm_run_statement) == 56, "cm_run_statement: fourteen words, as the header states");
static_assert(PID_TAIL == 1024, "k_pid_tree: one lane per node of an LDS level, one workgroup");

// ---- kernels -----------------------------------------------------------------------------------------------------------
// tab[PT_OFF * n_items + i] = the first cell of item i among `total`; an item the host refused has no cells
__global__ void __launch_bounds__(PID_BLOCK)
k_pid_cells(const uint32_t* __restrict__ tab, uint32_t n_items, uint32_t total, const uint4* __restrict__ values, uint32_t* __restrict__ nodes,
            uint32_t* __restrict__ flag) {
  const uint32_t t = blockIdx.x * PID_BLOCK + threadIdx.x;
  if (t >= total) return;
  const uint4 q = values[t];
  const uint32_t v[4] = {q.x, q.y, q.z, q.w};
  if (pid_value_bad(v)) {
    // the item of cell t: the last one whose offset is not above t (items without cells share the offset of the next one with cells)
    uint32_t lo = 0, hi = n_items;
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (tab[PT_OFF * n_items + mid] <= t) lo = mid + 1; else hi = mid;
    }
    flag[lo - 1] = 1u;   // (lo >= 1: the first offset is 0)
  }
  nodes[t] = range_cell_node(v);
}

// item i = blockIdx.x: a[off .. off + count) holds its nodes of depth 28; b[off + i .. off + i + count / 2 + 1) is its second buffer.
// out[2 i] = the id, out[2 i + 1] = the flag (1 for an item without cells).
__global__ void __launch_bounds__(PID_TAIL)
k_pid_tree(const uint32_t* __restrict__ tab, uint32_t n_items, uint32_t* a, uint32_t* b, TreeDefaults dflt, uint32_t* __restrict__ out) {
  __shared__ uint32_t level[2][PID_TAIL];
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const uint32_t off = tab[PT_OFF * n_items + i], count = tab[PT_COUNT * n_items + i], first = tab[PT_FIRST * n_items + i];
  if (count == 0) {   // (the whole workgroup leaves: no barrier is skipped by a part of it)
    if (t == 0) { out[2 * i] = 0u; out[2 * i + 1] = 1u; }
    return;
  }
  uint32_t lo = first, hi = first + count - 1, cur = 0;
  uint32_t* in = a + off;
  uint32_t* spare = b + off + i;
#pragma unroll 1
  for (uint32_t k = 0; k < RANGE_SLOTS; k++) {
    const uint32_t plo = lo >> 1, n_out = pid_width(plo, hi >> 1), d = dflt.h[pid_child_depth(k)];
    const bool wide = pid_width(lo, hi) > PID_TAIL;
    uint32_t* const o = wide ? spare : level[cur];
#pragma unroll 1
    for (uint32_t j = t; j < n_out; j += PID_TAIL) {
      uint32_t l, r;
      pid_children(in, lo, hi, d, j + plo, l, r);
      o[j] = host::poseidon2_hash(l, r);
    }
    __syncthreads();
    if (wide) spare = in; else cur ^= 1u;
    in = o; lo = plo; hi >>= 1;
  }
  if (t == 0) { out[2 * i] = in[0]; out[2 * i + 1] = tab[PT_FLAG * n_items + i]; }
}

// ---- what makes a list of entries a program -----------------------------------------------------------------------------------
// "" or what is wrong with e[7 n]; words: also range-check the value words (the device path leaves those to k_pid_cells)
std::string entries_error(const uint32_t* e, uint64_t n, bool words) {
  if (!e) return "null entries";
  if (n == 0) return "no entries: a program of no cells has no id";
  if (n > PID_MAX_ENTRIES) return "more than 2^24 entries (" + std::to_string(n) + ")";
  if (!e[0]) return "entry 0 (address " + std::to_string(e[1]) + ") is absent";
  const uint32_t first = e[1];
  if (range_header_bad(first, (uint32_t)n))
    return "the range [" + std::to_string(first) + ", " + std::to_string((uint64_t)first + n) + ") ends beyond the address space of 2^28 cells";
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t* const r = e + PID_ENTRY_WORDS * i;
    if (!r[0]) return "entry " + std::to_string(i) + " (address " + std::to_string(first + i) + ") is absent";
    if (r[1] != first + i) return "entry " + std::to_string(i) + " has address " + std::to_string(r[1]) + ", not " + std::to_string(first + i);
    if (!words) continue;
    for (uint32_t j = 0; j < 4; j++)
      if (r[2 + j] >= P) return "value word " + std::to_string(j) + " of entry " + std::to_string(i) + " (address " + std::to_string(r[1]) + ") is not below P";
  }
  return "";
}

// the fold in host code; the entries are good (the caller checked)
uint32_t fold_host(const uint32_t* e, uint32_t n) {
  const std::vector<uint32_t>& dh = host::poseidon2_default_hashes();
  std::vector<uint32_t> a(n), b(n / 2 + 1);
  for (uint32_t i = 0; i < n; i++) a[i] = range_cell_node(e + PID_ENTRY_WORDS * (size_t)i + 2);
  uint32_t lo = e[1], hi = e[1] + n - 1;
  for (uint32_t k = 0; k < RANGE_SLOTS; k++) {
    const uint32_t plo = lo >> 1, n_out = pid_width(plo, hi >> 1), d = dh[pid_child_depth(k)];
#pragma unroll 1
    for (uint32_t j = 0; j < n_out; j++) {
      uint32_t l, r;
      pid_children(a.data(), lo, hi, d, j + plo, l, r);
      b[j] = host::poseidon2_hash(l, r);
    }
    a.swap(b);
    lo = plo; hi >>= 1;
  }
  return a[0];
}

struct Item { const uint32_t* e; uint64_t n; std::string refused; };

// ids[i], status[i] for every item; the lowest bad item's message in `first_bad` ("" when every item is good)
void ids_device(std::vector<Item>& items, uint32_t* ids, int32_t* status, std::string& first_bad, hipStream_t st) {
  const uint32_t n = (uint32_t)items.size();
  uint64_t total = 0;
  for (Item& it : items) {
    if (it.refused.empty()) it.refused = entries_error(it.e, it.n, false);
    if (it.refused.empty()) total += it.n;
    CM_CHECK(total <= PID_MAX_BATCH_CELLS, "program ids: more than 2^26 cells in one call: split the batch");
  }
  std::vector<uint32_t> up((size_t)PT_RUNS * n + 4 * total, 0u);
  uint32_t* const vals = up.data() + (size_t)PT_RUNS * n;
  uint32_t off = 0;
  for (uint32_t i = 0; i < n; i++) {
    const Item& it = items[i];
    const bool good = it.refused.empty();
    up[PT_OFF * n + i] = off;
    up[PT_COUNT * n + i] = good ? (uint32_t)it.n : 0u;
    up[PT_FIRST * n + i] = good ? it.e[1] : 0u;
    if (!good) continue;
    for (uint64_t c = 0; c < it.n; c++) memcpy(vals + 4 * ((size_t)off + c), it.e + PID_ENTRY_WORDS * c + 2, 16);
    off += (uint32_t)it.n;
  }
  const TreeDefaults dflt = tree_defaults();
  DevBuf d_up(up.size() * 4), d_a((total + 1) * 4), d_b((total + n) * 4), d_out((size_t)n * 8);
  stage_upload(d_up.p, up.data(), up.size() * 4, st);
  const uint32_t* const tab = d_up.u32();
  if (total)
    hipLaunchKernelGGL(k_pid_cells, blocks_for(total, PID_BLOCK), dim3(PID_BLOCK), 0, st, tab, n, (uint32_t)total,
                       (const uint4*)(d_up.u32() + (size_t)PT_RUNS * n), d_a.u32(), d_up.u32() + (size_t)PT_FLAG * n);
  hipLaunchKernelGGL(k_pid_tree, dim3(n), dim3(PID_TAIL), 0, st, tab, n, d_a.u32(), d_b.u32(), dflt, d_out.u32());
  CM_HIP(hipGetLastError());
  const uint32_t* const land = (const uint32_t*)stage_download_async(d_out.p, (size_t)n * 8, st);
  CM_HIP(hipStreamSynchronize(st));   // the buffers go back to the pool behind this wait
  for (uint32_t i = 0; i < n; i++) {
    Item& it = items[i];
    if (it.refused.empty() && land[2 * i + 1]) {
      it.refused = entries_error(it.e, it.n, true);
      if (it.refused.empty()) it.refused = "a value word is not below P";
    }
    status[i] = it.refused.empty() ? 0 : 1;
    ids[i] = it.refused.empty() ? land[2 * i] : 0u;
    if (!it.refused.empty() && first_bad.empty()) first_bad = "item " + std::to_string(i) + ": " + it.refused;
  }
}

// a proof's entries of one kind, as cm_proof_public_entries lays them out
std::vector<uint32_t> proof_entries(const cm_proof* p, uint32_t which) {
  if (!p || !p->d || which > 2) throw CmError(1, "program id: the proof's public entries cannot be read");
  const PublicData& d = p->d->public_data;
  const std::vector<PublicEntry>& v = which == 0 ? d.program : which == 1 ? d.input : d.output;
  static_assert(sizeof(PublicEntry) == 4 * PID_ENTRY_WORDS, "PID_ENTRY_WORDS words per public entry");
  const uint32_t* w = (const uint32_t*)v.data();
  return std::vector<uint32_t>(w, w + PID_ENTRY_WORDS * v.size());
}

std::string hex8(uint32_t x) {
  char buf[16];
  snprintf(buf, sizeof(buf), "0x%08x", x);
  return buf;
}

}  // namespace
}  // namespace cm

// ================================================================= C ABI
namespace {
int32_t batch_result(const std::string& first_bad) {
  if (first_bad.empty()) return 0;
  cm_set_last_error(first_bad.c_str());
  return 1;
}
}  // namespace

extern "C" {
// host code: no device call on this path
int32_t cm_program_id_entries(const uint32_t* entries, uint64_t n, uint32_t* id) {
  return cm::abi_guard([&] {
    CM_CHECK(entries && id, "cm_program_id_entries: null argument");
    const std::string bad = cm::entries_error(entries, n, true);
    CM_CHECK(bad.empty(), "cm_program_id_entries: " + bad);
    *id = cm::fold_host(entries, (uint32_t)n);
  });
}
int32_t cm_proof_program_id(const cm_proof* p, uint32_t* id) {
  return cm::abi_guard([&] {
    CM_CHECK(p && id, "cm_proof_program_id: null argument");
    const std::vector<uint32_t> e = cm::proof_entries(p, 0);
    const std::string bad = cm::entries_error(e.data(), e.size() / cm::PID_ENTRY_WORDS, true);
    CM_CHECK(bad.empty(), "cm_proof_program_id: " + bad);
    *id = cm::fold_host(e.data(), (uint32_t)(e.size() / cm::PID_ENTRY_WORDS));
  });
}
int32_t cm_program_ids(const uint32_t* const* entries, const uint64_t* n_entries, uint32_t n, uint32_t* ids, int32_t* status, cm_stream_t s) {
  std::string first_bad;
  const int32_t rc = cm::abi_guard([&] {
    cm::open_require_device("cm_program_ids");
    CM_CHECK(n >= 1 && entries && n_entries && ids && status, "cm_program_ids: no items / null argument");
    CM_CHECK(n <= cm::PID_MAX_ITEMS, "cm_program_ids: more than 2^20 items in one call: split the batch");
    std::vector<cm::Item> items(n);
    for (uint32_t i = 0; i < n; i++) items[i] = cm::Item{entries[i], n_entries[i], ""};
    cm::bind_thread_to_library_device();
    cm::ids_device(items, ids, status, first_bad, cm::stream_or_own(s));
  });
  return rc ? rc : batch_result(first_bad);
}
int32_t cm_proofs_program_ids(const cm_proof* const* proofs, uint32_t n, uint32_t* ids, int32_t* status, cm_stream_t s) {
  std::string first_bad;
  const int32_t rc = cm::abi_guard([&] {
    cm::open_require_device("cm_proofs_program_ids");
    CM_CHECK(n >= 1 && proofs && ids && status, "cm_proofs_program_ids: no proofs / null argument");
    CM_CHECK(n <= cm::PID_MAX_ITEMS, "cm_proofs_program_ids: more than 2^20 proofs in one call: split the batch");
    std::vector<std::vector<uint32_t>> own(n);
    std::vector<cm::Item> items(n);
    for (uint32_t i = 0; i < n; i++) {
      if (!proofs[i]) { items[i] = cm::Item{nullptr, 0, "null proof"}; continue; }
      own[i] = cm::proof_entries(proofs[i], 0);
      items[i] = cm::Item{own[i].data(), own[i].size() / cm::PID_ENTRY_WORDS, ""};
    }
    cm::bind_thread_to_library_device();
    cm::ids_device(items, ids, status, first_bad, cm::stream_or_own(s));
  });
  return rc ? rc : batch_result(first_bad);
}

// What a chain of proofs states.  The chain check comes first and speaks for itself; then the program has to be one program.
int32_t cm_run_statement_of(const cm_proof* const* proofs, uint32_t n, const cm_pcs_config* expected, const uint32_t* expected_program_id,
                            uint32_t device, cm_run_statement* out) {
  {
    const int32_t rc = cm::abi_guard([&] {
      CM_CHECK(out, "cm_run_statement_of: null output");
      CM_CHECK(out->struct_size >= sizeof(cm_run_statement),
               "cm_run_statement_of: struct_size does not cover cm_run_statement (set it to sizeof(cm_run_statement))");
      CM_CHECK(device <= 1, "cm_run_statement_of: `device` is not 0 (host code) or 1 (the GPU)");
    });
    if (rc) return rc;
  }
  const int32_t chain = device ? cm_verify_run_device(proofs, n, expected) : cm_verify_run(proofs, n, expected);
  if (chain) return chain;   // (status and message are the chain check's own)
  return cm::abi_guard([&] {
    const std::vector<uint32_t> prog = cm::proof_entries(proofs[0], 0);
    const uint64_t m = prog.size() / cm::PID_ENTRY_WORDS;
    for (uint32_t i = 1; i < n; i++) {
      const std::vector<uint32_t> other = cm::proof_entries(proofs[i], 0);
      const uint64_t k = other.size() / cm::PID_ENTRY_WORDS;
      if (k != m)
        throw cm::CmError(11, "run: segment " + std::to_string(i) + " has " + std::to_string(k) + " program entries, segment 0 has " + std::to_string(m));
      for (uint64_t c = 0; c < m; c++) {
        const uint32_t* const x = prog.data() + cm::PID_ENTRY_WORDS * c;
        const uint32_t* const y = other.data() + cm::PID_ENTRY_WORDS * c;
        if (memcmp(x, y, 6 * 4) != 0)   // present, address, value[4]: the clock is not compared
          throw cm::CmError(11, "run: segment " + std::to_string(i) + " program differs from segment 0 at address " + std::to_string(x[0] ? x[1] : y[1]));
      }
    }
    uint32_t id = 0;
    if (device) {
      std::vector<cm::Item> items(1, cm::Item{prog.data(), m, ""});
      int32_t status = 0;
      std::string first_bad;
      cm::bind_thread_to_library_device();
      cm::ids_device(items, &id, &status, first_bad, cm::thread_main_stream());
      CM_CHECK(status == 0, "run: program id: " + items[0].refused);
    } else {
      const std::string bad = cm::entries_error(prog.data(), m, true);
      CM_CHECK(bad.empty(), "run: program id: " + bad);
      id = cm::fold_host(prog.data(), (uint32_t)m);
    }
    if (expected_program_id && *expected_program_id != id)
      throw cm::CmError(11, "run: program_id " + cm::hex8(id) + " != expected " + cm::hex8(*expected_program_id));
    cm_public_data head, tail;
    head.struct_size = tail.struct_size = sizeof(cm_public_data);
    CM_CHECK(cm_proof_public_data(proofs[0], &head) == 0 && cm_proof_public_data(proofs[n - 1], &tail) == 0,
             "cm_run_statement_of: the proofs' public data cannot be read");
    cm_run_statement o;
    memset(&o, 0, sizeof(o));
    o.struct_size = sizeof(o);
    o.n_segments = n;
    o.program_id = id;
    o.program_start = prog[1];
    o.n_program = (uint32_t)m;
    o.initial_pc = head.initial_pc; o.initial_fp = head.initial_fp; o.final_pc = tail.final_pc; o.final_fp = tail.final_fp;
    o.initial_root = head.initial_root; o.final_root = tail.final_root;
    o.n_input = head.n_input; o.n_output = tail.n_output;
    memcpy(out, &o, sizeof(o));
  });
}
}  // extern "C"
