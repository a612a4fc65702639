// The adapter's tail for a run (cm_run, header revision 10): included by adapter_device.hip behind its kernels.
//
// A run keeps the program's memory on the device between segments — `lo` = the locals, dense from address 0; `hi` = the heap, index
// h = the cell at MAX_ADDRESS - h — so segment k + 1 starts from segment k's image plus segment k's log instead of a fresh upload
// of all of memory.  From the image and the touched-cell list of step 5 (k_cells: ascending address, first / last entry, last
// clock) the kernels below build, on the calling thread's stream:
//   * both boundary-memory row arrays: locals, then the touched cells in the gap between the two regions (placed by an exclusive
//     scan of "in gap" over the cell list), then the heap in ascending address.  Every image cell first gets its untouched row
//     (k_run_rows_image), the touched cells then overwrite theirs (k_run_rows_touched, later on the same stream): the order comes
//     from addresses and the scan, never from atomics;
//   * the leaves of both partial Merkle trees (k_run_leaves) for the device-pointer tree builder;
//   * the public entries of the three ranges (k_run_public), copied to pinned memory: the only download that is not O(1);
//   * the advance: last-entry values scattered into the image (k_run_advance) behind everything that reads the old one.
// Host round trips of one segment: the adapter's two (totals / flags, counts) and ONE here (gap count, flags, both tree sizes and
// roots, public entries), then one wait without data behind the copy of the tree nodes into right-sized blocks (device trees) or
// behind their upload (a memory below CM_ADAPTER_DEVICE_TREE_MIN rows hashes its trees on the host from the downloaded rows).  No NULL-stream copy, no device-wide wait, no host container keyed by address.
namespace cm {

struct Run {
  DevBuf lo, hi;                    // the image: 16 bytes per cell (pool blocks of the thread that made or last grew them)
  uint32_t n_lo = 0, n_hi = 0;      // cells in each region
  uint64_t cap_lo = 0, cap_hi = 0;  // cells allocated
  uint32_t ranges[6] = {0, 0, 0, 0, 0, 0};
  hipEvent_t ev = nullptr;          // behind the last work enqueued on the image
  // the image's own partial Merkle tree (node list, exact size) for cm_run_open_memory: built on first use, dropped — not
  // rebuilt — when the image advances; empty otherwise, so a run that never opens a cell pays nothing for it
  DevBuf img_tree;
  uint64_t n_img_tree = 0;
  uint32_t img_root = 0;
  std::mutex mu;                    // one call at a time
  void mark(hipStream_t st) { CM_HIP(hipEventRecord(ev, st)); }
  void wait_on(hipStream_t st) { CM_HIP(hipStreamWaitEvent(st, ev, 0)); }
  ~Run() { if (ev) { (void)hipEventSynchronize(ev); (void)hipEventDestroy(ev); } }
};

struct RunTailIn {
  const cm_runner_segment& seg;
  uint32_t n_steps, n_mem, n_cells, n_acc, n_cu;
  uint64_t (&counts)[CM_N_OPCODE_COMPONENTS];
  DevBuf (&bundles)[CM_N_OPCODE_COMPONENTS];
  DevBuf &d_acc, &d_cu, &d_mem, &d_cells;
  uint64_t n_memory_end, n_heap_end;
};

DeviceInput* make_device_input_resident(const cm_prover_input& meta, DevBuf (&bundles)[CM_N_OPCODE_COMPONENTS], DevBuf& data_accesses, DevBuf& clock_updates,
                                        DevBuf& init_mem, DevBuf& fin_mem, DevBuf& init_tree, DevBuf& fin_tree, const PublicEntry* entries);  // prover.hip

namespace {

struct RunDims { uint32_t n_lo, n_hi, hi_base; };   // hi_base = MAX_ADDRESS + 1 - n_hi: the lowest heap address
struct Ranges6 { uint32_t r[6]; };                  // program, input, output: [start, end)
// device words of one tail: [0] touched cells in the gap, [1] flags (1: an address beyond MAX_ADDRESS, 2: a non-zero cell outside
// both regions at the segment's end), [2..3] / [4..5] TreeState of the initial / final tree
enum : uint32_t { RS_GAP = 0, RS_ERR = 1, RS_TREE0 = 2, RS_TREE1 = 4, RS_WORDS = 8 };

__device__ __forceinline__ bool in_range(const Ranges6& g, int k, uint32_t a) { return a >= g.r[2 * k] && a < g.r[2 * k + 1]; }
// update_multiplicities (adapter/memory.rs:427-461), one cell: program, input, then output
__device__ __forceinline__ void public_mults(const Ranges6& g, uint32_t a, uint32_t& im, uint32_t& fm) {
  if (in_range(g, 0, a)) { im = 0; if (fm == 0) fm = host::M31_NEG1; }
  if (in_range(g, 1, a)) { im = 0; if (fm == 0) fm = host::M31_NEG1; }
  if (in_range(g, 2, a)) { fm = 0; im = 1; }
}
__device__ __forceinline__ void put_row(cm_memory_cell* rows, uint32_t row, uint32_t addr, uint4 v, uint32_t clock, uint32_t mult) {
  static_assert(sizeof(cm_memory_cell) == 28, "boundary-memory rows are seven words");
  uint32_t* o = reinterpret_cast<uint32_t*>(rows + row);
  o[0] = addr; o[1] = v.x; o[2] = v.y; o[3] = v.z; o[4] = v.w; o[5] = clock; o[6] = mult;
}
__device__ __forceinline__ uint4 log_value(const uint32_t* __restrict__ mem, uint32_t e) {
  const uint32_t* w = mem + 5 * (size_t)e + 1;
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// per touched cell: 1 when it lies between the two regions (its row is placed by the scan of these flags)
__global__ void k_run_gap_flags(const CellRec* __restrict__ cells, uint32_t n_cells, RunDims d, uint32_t* __restrict__ flag, uint32_t* __restrict__ state) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const uint32_t a = cells[i].addr;
  if (a > host::MAX_ADDRESS) atomicOr(state + RS_ERR, 1u);
  flag[i] = (a >= d.n_lo && a < d.hi_base) ? 1u : 0u;
}
__global__ void k_run_totals(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ rank, uint32_t n_cells, RunDims d, uint32_t* __restrict__ state) {
  if (threadIdx.x || blockIdx.x) return;
  const uint32_t n_gap = rank[n_cells - 1] + flag[n_cells - 1];
  const uint32_t leaves = 4u * (d.n_lo + n_gap + d.n_hi);
  state[RS_GAP] = n_gap;
  state[RS_TREE0] = leaves; state[RS_TREE0 + 1] = 0;
  state[RS_TREE1] = leaves; state[RS_TREE1 + 1] = 0;
}
// one thread per image cell (one 16-byte load each, coalesced): its row as if the segment had not touched it
__global__ void k_run_rows_image(const uint4* __restrict__ lo, const uint4* __restrict__ hi, RunDims d, Ranges6 g, const uint32_t* __restrict__ state,
                                 cm_memory_cell* __restrict__ init_rows, cm_memory_cell* __restrict__ fin_rows) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.n_lo + d.n_hi) return;
  uint32_t addr, row;
  uint4 v;
  if (t < d.n_lo) { addr = t; row = t; v = lo[t]; }
  else {
    const uint32_t j = t - d.n_lo;             // ascending address = descending heap index
    addr = d.hi_base + j; row = d.n_lo + state[RS_GAP] + j; v = hi[host::MAX_ADDRESS - addr];
  }
  uint32_t im = 0, fm = 0;
  public_mults(g, addr, im, fm);
  put_row(init_rows, row, addr, v, 0u, im);
  put_row(fin_rows, row, addr, v, 0u, fm);
}
// one thread per touched cell, behind k_run_rows_image: initial row = the image's value (or the first logged value of a cell
// outside it), final row = the last logged value and clock.  end = the regions when the segment ends: a touched cell outside
// them is a read of an untouched cell and has to be zero.
__global__ void k_run_rows_touched(const CellRec* __restrict__ cells, const uint32_t* __restrict__ rank, uint32_t n_cells, const uint32_t* __restrict__ mem,
                                   const uint4* __restrict__ lo, const uint4* __restrict__ hi, RunDims d, RunDims end, Ranges6 g,
                                   uint32_t* __restrict__ state, cm_memory_cell* __restrict__ init_rows, cm_memory_cell* __restrict__ fin_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const CellRec c = cells[i];
  if (c.addr > host::MAX_ADDRESS) return;      // (flagged by k_run_gap_flags)
  uint32_t row;
  uint4 iv;
  if (c.addr < d.n_lo) { row = c.addr; iv = lo[c.addr]; }
  else if (c.addr >= d.hi_base) { row = d.n_lo + state[RS_GAP] + (c.addr - d.hi_base); iv = hi[host::MAX_ADDRESS - c.addr]; }
  else { row = d.n_lo + rank[i]; iv = log_value(mem, c.first_entry); }
  const uint4 fv = log_value(mem, c.last_entry);
  if (c.addr >= end.n_lo && c.addr < end.hi_base && (fv.x | fv.y | fv.z | fv.w)) atomicOr(state + RS_ERR, 2u);
  uint32_t im = 1, fm = host::M31_NEG1;
  public_mults(g, c.addr, im, fm);
  put_row(init_rows, row, c.addr, iv, 0u, im);
  put_row(fin_rows, row, c.addr, fv, c.last_clock, fm);
}
// four (index, value, multiplicity) leaves per row and tree; multiplicity 2 inside the public ranges (program and input for the
// initial tree, output for the final one)
__global__ void k_run_leaves(const cm_memory_cell* __restrict__ init_rows, const cm_memory_cell* __restrict__ fin_rows, RunDims d, Ranges6 g,
                             const uint32_t* __restrict__ state, uint32_t cap_rows, uint32_t* __restrict__ i_idx, uint32_t* __restrict__ i_val,
                             uint32_t* __restrict__ i_mult, uint32_t* __restrict__ f_idx, uint32_t* __restrict__ f_val, uint32_t* __restrict__ f_mult) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= cap_rows || r >= d.n_lo + state[RS_GAP] + d.n_hi) return;
  const uint32_t* a = reinterpret_cast<const uint32_t*>(init_rows + r);
  const uint32_t* b = reinterpret_cast<const uint32_t*>(fin_rows + r);
  const uint32_t addr = a[0];
  const uint32_t mi = (in_range(g, 0, addr) || in_range(g, 1, addr)) ? 2u : 1u, mf = in_range(g, 2, addr) ? 2u : 1u;
  reinterpret_cast<uint4*>(i_idx)[r] = make_uint4(addr << 2, (addr << 2) + 1, (addr << 2) + 2, (addr << 2) + 3);
  reinterpret_cast<uint4*>(f_idx)[r] = make_uint4(addr << 2, (addr << 2) + 1, (addr << 2) + 2, (addr << 2) + 3);
  reinterpret_cast<uint4*>(i_val)[r] = make_uint4(a[1], a[2], a[3], a[4]);
  reinterpret_cast<uint4*>(f_val)[r] = make_uint4(b[1], b[2], b[3], b[4]);
  reinterpret_cast<uint4*>(i_mult)[r] = make_uint4(mi, mi, mi, mi);
  reinterpret_cast<uint4*>(f_mult)[r] = make_uint4(mf, mf, mf, mf);
}
// entry j of the three ranges laid end to end -> PublicEntry (present, address, value, clock): program and input from the initial
// rows, output from the final ones.  A cell between the regions is looked up in the touched-cell list by bisection.
__global__ void k_run_public(Ranges6 g, uint32_t n_total, const CellRec* __restrict__ cells, const uint32_t* __restrict__ rank, uint32_t n_cells,
                             RunDims d, const uint32_t* __restrict__ state, const cm_memory_cell* __restrict__ init_rows,
                             const cm_memory_cell* __restrict__ fin_rows, PublicEntry* __restrict__ out) {
  uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_total) return;
  PublicEntry e;
  e.present = 0; e.addr = 0; e.value[0] = e.value[1] = e.value[2] = e.value[3] = 0; e.clock = 0;
  int k = 0;
  uint32_t off = j;
  for (; k < 3; k++) {
    const uint32_t len = g.r[2 * k + 1] > g.r[2 * k] ? g.r[2 * k + 1] - g.r[2 * k] : 0u;
    if (off < len) break;
    off -= len;
  }
  const uint32_t a = g.r[2 * k] + off;
  uint32_t row = 0xffffffffu;
  if (a < d.n_lo) row = a;
  else if (a >= d.hi_base && a <= host::MAX_ADDRESS) row = d.n_lo + state[RS_GAP] + (a - d.hi_base);
  else {
    uint32_t lo = 0, hi = n_cells;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (cells[mid].addr < a) lo = mid + 1; else hi = mid; }
    if (lo < n_cells && cells[lo].addr == a) row = d.n_lo + rank[lo];
  }
  if (row != 0xffffffffu) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>((k == 2 ? fin_rows : init_rows) + row);
    e.present = 1; e.addr = a; e.value[0] = w[1]; e.value[1] = w[2]; e.value[2] = w[3]; e.value[3] = w[4]; e.clock = w[5];
  }
  out[j] = e;
}
// the advance: every touched cell inside the regions at the segment's end takes its last logged value
__global__ void k_run_advance(const CellRec* __restrict__ cells, uint32_t n_cells, const uint32_t* __restrict__ mem, RunDims end,
                              uint4* __restrict__ lo, uint4* __restrict__ hi) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_cells) return;
  const CellRec c = cells[i];
  const uint4 v = log_value(mem, c.last_entry);
  if (c.addr < end.n_lo) lo[c.addr] = v;
  else if (c.addr >= end.hi_base && c.addr <= host::MAX_ADDRESS) hi[host::MAX_ADDRESS - c.addr] = v;
}

// build_partial_merkle_tree over sorted leaf arrays (no map): the host form of the level-by-level device builder, for small memories
uint32_t partial_merkle_tree_sorted_host(std::vector<uint32_t> idx, std::vector<uint32_t> val, std::vector<uint32_t> mult, std::vector<cm_merkle_node>& nodes) {
  const std::vector<uint32_t>& dflt = host::poseidon2_default_hashes();
  std::vector<uint32_t> nidx, nval, nmult;
  for (uint32_t depth = air::TREE_HEIGHT; depth >= 1; depth--) {
    nidx.clear(); nval.clear(); nmult.clear();
    for (size_t i = 0; i < idx.size();) {
      const uint32_t index = idx[i];
      uint32_t lv = dflt[depth], lm = 0, rv = dflt[depth], rm = 0;
      size_t used = 1;
      if ((index & 1u) == 0) {
        lv = val[i]; lm = mult[i];
        if (i + 1 < idx.size() && idx[i + 1] == index + 1) { rv = val[i + 1]; rm = mult[i + 1]; used = 2; }
      } else { rv = val[i]; rm = mult[i]; }
      const uint32_t ph = host::poseidon2_hash(lv, rv);
      nodes.push_back(cm_merkle_node{index & ~1u, depth, lv, rv, ph, lm, rm, 1u});
      nidx.push_back(index >> 1); nval.push_back(ph); nmult.push_back(1u);
      i += used;
    }
    idx.swap(nidx); val.swap(nval); mult.swap(nmult);
  }
  return val.empty() ? 0u : val[0];
}

// a region that has to hold n_end cells: capacity doubling, the cells it grows over are zero
void run_grow(DevBuf& buf, uint64_t& cap, uint32_t n_now, uint32_t n_end, hipStream_t st) {
  if (n_end > cap) {
    const uint64_t ncap = std::max<uint64_t>(n_end, std::min<uint64_t>(2 * cap, (uint64_t)host::MAX_ADDRESS + 1));
    DevBuf nb((size_t)ncap * 16);
    if (n_now) CM_HIP(hipMemcpyAsync(nb.p, buf.p, (size_t)n_now * 16, hipMemcpyDeviceToDevice, st));
    buf = std::move(nb);   // (the old block goes back to this thread's pool: reuse is ordered behind the copy on `st`)
    cap = ncap;
  }
  if (n_end > n_now) CM_HIP(hipMemsetAsync((uint8_t*)buf.p + (size_t)n_now * 16, 0, (size_t)(n_end - n_now) * 16, st));
}

DeviceInput* run_tail(Run& run, RunTailIn& t, hipStream_t st) {
  const uint64_t SPACE = (uint64_t)host::MAX_ADDRESS + 1;
  const RunDims d{run.n_lo, run.n_hi, (uint32_t)(SPACE - run.n_hi)};
  const RunDims end{(uint32_t)t.n_memory_end, (uint32_t)t.n_heap_end, (uint32_t)(SPACE - t.n_heap_end)};
  Ranges6 g;
  for (int i = 0; i < 2; i++) { g.r[i] = t.seg.program_range[i]; g.r[2 + i] = t.seg.input_range[i]; g.r[4 + i] = t.seg.output_range[i]; }
  uint64_t n_pub = 0;
  for (int k = 0; k < 3; k++) n_pub += g.r[2 * k + 1] > g.r[2 * k] ? g.r[2 * k + 1] - g.r[2 * k] : 0u;
  CM_CHECK(n_pub <= 3 * SPACE, "run: public ranges larger than the address space");
  const uint32_t n_cells = t.n_cells;
  // the gap holds at most every touched cell, and at most its own width
  const uint64_t cap_rows64 = (uint64_t)d.n_lo + std::min<uint64_t>(n_cells, (uint64_t)d.hi_base - d.n_lo) + d.n_hi;
  CM_CHECK(cap_rows64 < (1ull << 30), "run: boundary memory too large");
  const uint32_t cap_rows = (uint32_t)cap_rows64;
  const CellRec* cells = t.d_cells.as<CellRec>();
  const uint4* lo = run.lo.as<uint4>();
  const uint4* hi = run.hi.as<uint4>();
  // ---- rows ----
  DevBuf d_state(RS_WORDS * 4), d_flag((size_t)n_cells * 4 + 4), d_rank((size_t)n_cells * 4 + 4);
  DevBuf init_rows((size_t)cap_rows * sizeof(cm_memory_cell) + 4), fin_rows((size_t)cap_rows * sizeof(cm_memory_cell) + 4);
  CM_HIP(hipMemsetAsync(d_state.p, 0, RS_WORDS * 4, st));
  hipLaunchKernelGGL(k_run_gap_flags, grid1(n_cells), dim3(256), 0, st, cells, n_cells, d, d_flag.u32(), d_state.u32());
  with_temp([&](void* tmp, size_t& b) { CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp, b, d_flag.u32(), d_rank.u32(), (int)n_cells, st)); });
  hipLaunchKernelGGL(k_run_totals, dim3(1), dim3(64), 0, st, d_flag.u32(), d_rank.u32(), n_cells, d, d_state.u32());
  if (d.n_lo + d.n_hi)
    hipLaunchKernelGGL(k_run_rows_image, grid1(d.n_lo + d.n_hi), dim3(256), 0, st, lo, hi, d, g, d_state.u32(), init_rows.as<cm_memory_cell>(),
                       fin_rows.as<cm_memory_cell>());
  hipLaunchKernelGGL(k_run_rows_touched, grid1(n_cells), dim3(256), 0, st, cells, d_rank.u32(), n_cells, t.d_mem.u32(), lo, hi, d, end, g,
                     d_state.u32(), init_rows.as<cm_memory_cell>(), fin_rows.as<cm_memory_cell>());
  // ---- public entries -> pinned memory ----
  DevBuf d_pub((size_t)n_pub * sizeof(PublicEntry) + 4);
  if (n_pub)
    hipLaunchKernelGGL(k_run_public, grid1((uint32_t)n_pub), dim3(256), 0, st, g, (uint32_t)n_pub, cells, d_rank.u32(), n_cells, d, d_state.u32(),
                       init_rows.as<cm_memory_cell>(), fin_rows.as<cm_memory_cell>(), d_pub.as<PublicEntry>());
  // ---- trees: on the device, or (small memories) on the host from the downloaded rows ----
  size_t tree_min = 2048;
  if (const char* e = getenv("CM_ADAPTER_DEVICE_TREE_MIN")) tree_min = (size_t)strtoull(e, nullptr, 10);
  const bool device_trees = cap_rows >= tree_min;
  uint32_t* const pin = pinned_words() + PIN_LAST_LAYER + 64;   // [0..7] the state words, [8..10] / [12..14] tree size + root
  TreeJob job[2];
  DevBuf tree[2];
  const size_t rows_bytes = (size_t)cap_rows * sizeof(cm_memory_cell), pub_bytes = (size_t)n_pub * sizeof(PublicEntry);
  const size_t pub_off = device_trees ? 0 : ((2 * rows_bytes + 15) & ~(size_t)15);
  uint8_t* land = (uint8_t*)stage_landing(pub_off + pub_bytes + 16, st);
  if (device_trees) {
    for (int h = 0; h < 2; h++) for (int k = 0; k < 3; k++) job[h].a[k].alloc((size_t)cap_rows * 16);
    hipLaunchKernelGGL(k_run_leaves, grid1(cap_rows), dim3(256), 0, st, init_rows.as<cm_memory_cell>(), fin_rows.as<cm_memory_cell>(), d, g, d_state.u32(),
                       cap_rows, job[0].a[0].u32(), job[0].a[1].u32(), job[0].a[2].u32(), job[1].a[0].u32(), job[1].a[1].u32(), job[1].a[2].u32());
    for (int h = 0; h < 2; h++) {
      job[h].state.alloc(sizeof(TreeState));
      CM_HIP(hipMemcpyAsync(job[h].state.p, d_state.u32() + (h ? RS_TREE1 : RS_TREE0), sizeof(TreeState), hipMemcpyDeviceToDevice, st));
      partial_merkle_tree_enqueue(job[h], 4 * cap_rows, tree[h], pin + 8 + 4 * h, st);
    }
  } else {
    CM_HIP(hipMemcpyAsync(land, init_rows.p, rows_bytes, hipMemcpyDeviceToHost, st));
    CM_HIP(hipMemcpyAsync(land + rows_bytes, fin_rows.p, rows_bytes, hipMemcpyDeviceToHost, st));
  }
  if (pub_bytes) CM_HIP(hipMemcpyAsync(land + pub_off, d_pub.p, pub_bytes, hipMemcpyDeviceToHost, st));
  CM_HIP(hipMemcpyAsync(pin, d_state.p, RS_WORDS * 4, hipMemcpyDeviceToHost, st));
  CM_HIP(hipGetLastError());
  CM_HIP(hipStreamSynchronize(st));   // the tail's one round trip
  const uint32_t n_gap = pin[RS_GAP], err = pin[RS_ERR];
  CM_CHECK(!(err & 1u), "run: the memory log names an address beyond MAX_ADDRESS");
  CM_CHECK(!(err & 2u), "run: a touched cell outside both regions at the segment's end is not zero (are the end lengths the runner's?)");
  const uint64_t n_rows = (uint64_t)d.n_lo + n_gap + d.n_hi;
  cm_prover_input meta;
  memset(&meta, 0, sizeof(meta));
  uint64_t n_tree[2] = {0, 0};
  uint32_t root[2] = {0, 0};
  if (device_trees) {
    for (int h = 0; h < 2; h++) {
      CM_CHECK(pin[8 + 4 * h] == 1, "partial merkle tree: did not converge to one root");
      n_tree[h] = pin[8 + 4 * h + 1]; root[h] = pin[8 + 4 * h + 2];
      // the builder's block is sized for the worst case (30 nodes per leaf); a dense memory has ~1.3: the input keeps a copy of
      // the right size, the large block goes back to this thread's pool for the next segment
      DevBuf exact(n_tree[h] * sizeof(cm_merkle_node) + 4);
      if (n_tree[h]) CM_HIP(hipMemcpyAsync(exact.p, tree[h].p, n_tree[h] * sizeof(cm_merkle_node), hipMemcpyDeviceToDevice, st));
      tree[h] = std::move(exact);
    }
    CM_HIP(hipStreamSynchronize(st));   // (a wait without data: the proof runs on another thread's streams)
  } else {
    for (int h = 0; h < 2; h++) {
      const uint32_t* rows = reinterpret_cast<const uint32_t*>(land + h * rows_bytes);
      std::vector<uint32_t> li, lv, lm;
      for (uint64_t r = 0; r < n_rows; r++) {
        const uint32_t a = rows[7 * r];
        const bool pub = h == 0 ? ((a >= g.r[0] && a < g.r[1]) || (a >= g.r[2] && a < g.r[3])) : (a >= g.r[4] && a < g.r[5]);
        for (uint32_t i = 0; i < 4; i++) { li.push_back((a << 2) + i); lv.push_back(rows[7 * r + 1 + i]); lm.push_back(pub ? 2u : 1u); }
      }
      std::vector<cm_merkle_node> nodes;
      root[h] = partial_merkle_tree_sorted_host(std::move(li), std::move(lv), std::move(lm), nodes);
      n_tree[h] = nodes.size();
      if (nodes.empty()) tree[h].alloc(4);
      else tree[h] = upload(nodes, st);   // through the pinned staging ring: `nodes` may die before the copy runs
    }
    CM_HIP(hipStreamSynchronize(st));   // the proof runs on another thread's streams
  }
  // ---- assemble the device-resident ProverInput ----
  meta.initial_pc = t.seg.trace[0]; meta.initial_fp = t.seg.trace[1];
  meta.final_pc = t.seg.trace[2 * (size_t)t.n_steps]; meta.final_fp = t.seg.trace[2 * (size_t)t.n_steps + 1];
  for (int c = 0; c < CM_N_OPCODE_COMPONENTS; c++) meta.n_bundles[c] = t.counts[c];
  meta.n_data_accesses = t.n_acc; meta.n_clock_updates = t.n_cu;
  meta.n_initial_memory = n_rows; meta.n_final_memory = n_rows;
  meta.n_initial_tree = n_tree[0]; meta.n_final_tree = n_tree[1];
  meta.initial_root = root[0]; meta.final_root = root[1];
  for (int i = 0; i < 2; i++) { meta.program_range[i] = g.r[i]; meta.input_range[i] = g.r[2 + i]; meta.output_range[i] = g.r[4 + i]; }
  // room for the image at the segment's end first (an allocation may fail; the image itself does not change: the cells a region
  // grows over are beyond its current length), then the input (a public entry may be refused); nothing after that can fail
  run_grow(run.lo, run.cap_lo, run.n_lo, end.n_lo, st);
  run_grow(run.hi, run.cap_hi, run.n_hi, end.n_hi, st);
  run.mark(st);   // a region may sit in a new block now: whoever comes next waits for its copy even if the call fails below
  DeviceInput* din = make_device_input_resident(meta, t.bundles, t.d_acc, t.d_cu, init_rows, fin_rows, tree[0], tree[1],
                                                reinterpret_cast<const PublicEntry*>(land + pub_off));
  // ---- the advance, behind everything that read the old image ----
  run.img_tree.release(); run.n_img_tree = 0;   // (its readers were waited for inside cm_run_open_memory)
  run.n_lo = end.n_lo; run.n_hi = end.n_hi;
  hipLaunchKernelGGL(k_run_advance, grid1(n_cells), dim3(256), 0, st, cells, n_cells, t.d_mem.u32(), end, run.lo.as<uint4>(), run.hi.as<uint4>());
  run.mark(st);
  return din;
}

}  // namespace

// ---- the run object (C ABI: cm_run_begin / cm_run_memory / cm_run_free in prover.hip) ----
Run* run_begin(const uint32_t* initial_memory, uint64_t n_initial_memory, const uint32_t* initial_heap, uint64_t n_initial_heap, const uint32_t ranges[6]) {
  bind_thread_to_library_device();
  hipStream_t st = thread_main_stream();
  const uint64_t SPACE = (uint64_t)host::MAX_ADDRESS + 1;
  CM_CHECK(ranges, "cm_run_begin: null ranges");
  CM_CHECK((initial_memory || !n_initial_memory) && (initial_heap || !n_initial_heap), "cm_run_begin: null memory");
  CM_CHECK(n_initial_memory <= SPACE && n_initial_heap <= SPACE && n_initial_memory + n_initial_heap <= SPACE, "cm_run_begin: locals and heap overlap");
  std::unique_ptr<Run> r(new Run());
  CM_HIP(hipEventCreateWithFlags(&r->ev, hipEventDisableTiming));
  for (int i = 0; i < 6; i++) r->ranges[i] = ranges[i];
  r->n_lo = (uint32_t)n_initial_memory; r->n_hi = (uint32_t)n_initial_heap;
  r->cap_lo = std::max<uint64_t>(n_initial_memory, 64); r->cap_hi = std::max<uint64_t>(n_initial_heap, 64);
  r->lo.alloc((size_t)r->cap_lo * 16); r->hi.alloc((size_t)r->cap_hi * 16);
  if (n_initial_memory) CM_HIP(hipMemcpyAsync(r->lo.p, initial_memory, (size_t)n_initial_memory * 16, hipMemcpyHostToDevice, st));
  if (n_initial_heap) CM_HIP(hipMemcpyAsync(r->hi.p, initial_heap, (size_t)n_initial_heap * 16, hipMemcpyHostToDevice, st));
  CM_HIP(hipStreamSynchronize(st));   // the caller's arrays are free again
  r->mark(st);
  return r.release();
}
void run_memory(Run& r, uint32_t* locals, uint64_t cap_l, uint64_t* n_l, uint32_t* heap, uint64_t cap_h, uint64_t* n_h) {
  bind_thread_to_library_device();
  hipStream_t st = thread_main_stream();
  if (n_l) *n_l = r.n_lo;
  if (n_h) *n_h = r.n_hi;
  r.wait_on(st);
  const bool want_l = locals && r.n_lo, want_h = heap && r.n_hi;
  CM_CHECK((!locals || cap_l >= r.n_lo) && (!heap || cap_h >= r.n_hi), "cm_run_memory: an output array is too small (the lengths are reported)");
  // straight into the caller's arrays (no pinned copy of the image is kept); waited for before the call returns
  if (want_l) CM_HIP(hipMemcpyAsync(locals, r.lo.p, (size_t)r.n_lo * 16, hipMemcpyDeviceToHost, st));
  if (want_h) CM_HIP(hipMemcpyAsync(heap, r.hi.p, (size_t)r.n_hi * 16, hipMemcpyDeviceToHost, st));
  CM_HIP(hipStreamSynchronize(st));
}
// The tree over the four leaves of each of `cells` cells, which `fill(idx, val, mult)` enqueues on st in ascending index order:
// the device tree builder, one round trip for the tree's size and root, one wait behind its copy into a right-sized block (the
// builder's is sized for 30 nodes per leaf: see run_tail).  For the image tree of a run and for cm_mem_image_create.
void leaves_tree_build(uint64_t cells, const std::function<void(uint32_t*, uint32_t*, uint32_t*)>& fill, DevBuf& nodes_out, uint64_t& n_nodes_out,
                       uint32_t& root_out, hipStream_t st) {
  CM_CHECK(cells > 0 && cells <= (uint64_t)host::MAX_ADDRESS + 1, "image tree: no cells, or more than the address space");
  const uint32_t cap = (uint32_t)(4 * cells);
  TreeJob j;
  for (int k = 0; k < 3; k++) j.a[k].alloc((size_t)cap * 4);
  j.state.alloc(sizeof(TreeState));
  const TreeState s0{cap, 0};
  stage_upload(j.state.p, &s0, sizeof(s0), st);
  fill(j.a[0].u32(), j.a[1].u32(), j.a[2].u32());
  DevBuf nodes;
  uint32_t* const pin3 = pinned_words() + PIN_LAST_LAYER + 56;
  partial_merkle_tree_enqueue(j, cap, nodes, pin3, st);
  CM_HIP(hipStreamSynchronize(st));
  CM_CHECK(pin3[0] == 1, "partial merkle tree: did not converge to one root");
  const uint64_t n_nodes = pin3[1];
  const uint32_t root = pin3[2];
  DevBuf exact(n_nodes * sizeof(cm_merkle_node) + 4);
  CM_HIP(hipMemcpyAsync(exact.p, nodes.p, n_nodes * sizeof(cm_merkle_node), hipMemcpyDeviceToDevice, st));
  CM_HIP(hipStreamSynchronize(st));
  nodes_out = std::move(exact); n_nodes_out = n_nodes; root_out = root;
}
// Openings under the root of the image as it is now (mem_open.hip): the leaves of every image cell (k_image_leaves) through the
// device tree builder on first use — one round trip for the tree's size and root, one wait behind its copy into a right-sized
// block — then one round trip per call for the records.
static void run_image_tree(Run& r, const char* who, hipStream_t st) {
  const uint64_t cells = (uint64_t)r.n_lo + r.n_hi;
  CM_CHECK(cells > 0, std::string(who) + ": the image is empty: there is no tree to open");
  if (!r.img_tree.p) {
    r.wait_on(st);   // the last advance may have been enqueued from another thread's stream
    leaves_tree_build(cells, [&](uint32_t* idx, uint32_t* val, uint32_t* mult) { image_leaves_enqueue(r.lo.u32(), r.n_lo, r.hi.u32(), r.n_hi, idx, val, mult, st); },
                      r.img_tree, r.n_img_tree, r.img_root, st);
  }
}
void run_open_memory(Run& r, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, uint32_t* root) {
  bind_thread_to_library_device();
  hipStream_t st = thread_main_stream();
  run_image_tree(r, "cm_run_open_memory", st);
  *root = r.img_root;
  open_paths(r.img_tree.as<cm_merkle_node>(), r.n_img_tree, addresses, n, out, st);
}
// The same cached tree, opened over a range (mem_range.hip): one round trip per call once the tree exists.
void run_open_memory_range(Run& r, uint32_t start, uint32_t n_cells, uint32_t* values, cm_mem_range_opening* out, uint32_t* root) {
  bind_thread_to_library_device();
  hipStream_t st = thread_main_stream();
  run_image_tree(r, "cm_run_open_memory_range", st);
  open_range(r.img_tree.as<cm_merkle_node>(), r.n_img_tree, start, n_cells, values, out, st);
  *root = r.img_root;
}
// The same cached tree, opened over a set of cells (mem_set.hip).  The set is good and n_siblings is its plan's (the caller checked).
void run_open_memory_set(Run& r, const uint32_t* addresses, uint32_t n, uint32_t* values, uint32_t* siblings, uint32_t n_siblings, uint32_t* root) {
  bind_thread_to_library_device();
  hipStream_t st = thread_main_stream();
  run_image_tree(r, "cm_run_open_memory_set", st);
  open_set(r.img_tree.as<cm_merkle_node>(), r.n_img_tree, addresses, n, values, siblings, n_siblings, st);
  *root = r.img_root;
}
// an upper bound of the boundary-memory rows of the next segment, for the memory budget: the image and every logged access
uint64_t run_rows_bound(const Run& r, uint64_t n_memory_trace) {
  const uint64_t gap = (uint64_t)host::MAX_ADDRESS + 1 - r.n_lo - r.n_hi;
  return (uint64_t)r.n_lo + r.n_hi + std::min(n_memory_trace, gap);
}
// the input errors of the advance that need no device data: before any GPU work
void run_check_ends(const Run& r, uint64_t n_memory_end, uint64_t n_heap_end) {
  const uint64_t SPACE = (uint64_t)host::MAX_ADDRESS + 1;
  CM_CHECK(n_memory_end >= r.n_lo && n_heap_end >= r.n_hi, "run: a region's end length is below its current length");
  CM_CHECK(n_memory_end <= SPACE && n_heap_end <= SPACE && n_memory_end + n_heap_end <= SPACE, "run: locals and heap overlap at the segment's end");
}
uint64_t run_image_bytes(const Run& r) { return pool_round(r.lo.bytes) + pool_round(r.hi.bytes); }
std::mutex& run_mutex(Run& r) { return r.mu; }
void run_free(Run* r) {
  if (!r) return;
  bind_thread_to_library_device();
  delete r;
}

}  // namespace cm
