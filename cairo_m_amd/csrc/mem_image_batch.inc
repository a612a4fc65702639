// Batched image updates (cm_mem_images_apply), the tail of mem_image.hip: many followed memories, one update each, through ONE
// ladder of launches whose length is that of the part with the most per-level steps — a small update is bound by its chain of
// dependent launches (DESIGN §3.2), and independent images can share that chain as the records of the batched verifier do
// (mem_batch.hip).  The lanes run the single update's own bodies (img_cell_records, img_parent, img_rank_lane, img_merge_lane)
// on the batch's layout (mem_batch.hpp: batch_plan, BatchView, batch_part, k_batch_heads, parts_flags_and_scan).
//
// Host: the call's argument checks, then per part the single call's checks 1 .. 3, which read nothing the device holds; a part that
// fails one has its verdict there and is left out.  Device, the same launches whatever the number of parts:
//   one upload of one block: per part the result words and a table entry (ImgPart), the lvl rows, the prefixes of the dirty records
//                    and of the merge lanes, then the addresses, new values and old values, concatenated;
//   k_imgs_check     k_img_check on the concatenation: a lane bisects lvl[0] for its part and looks its cell half up in THAT part's
//                    image; the lowest differing cell per part by atomicMin (a minimum: no order decides it);
//   k_imgs_cells     one lane per cell: the three records into the part's dirty slice, the node of depth 28;
//   the flag pass, ONE scan and the head scatter of the batched verifier;
//   k_imgs_level     one lane per parent of ALL parts' S_{k+1} while ANY part's S_k is wider than SET_TAIL: set_parent_from inside
//                    the part's slice, a child outside S_k from that part's own tree, the dirty record into that part's slice;
//   k_imgs_tail      one workgroup per part: the remaining depths in LDS, the part's root;
//   k_imgs_rank      one lane per dirty record of all parts (and one sentinel per part, so that the per-part totals fall out of
//                    ONE exclusive scan over the concatenated insert flags);
//   k_imgs_merge     one lane per old and per dirty record of all parts into each part's NEW list, taken from the pool before the
//                    first launch and sized as the single call sizes its own;
//   k_imgs_offsets   one block per part: the new depth offsets, into the result words and into the part's new handle words;
//   one download of the result words, one wait.  The host then decides part by part: refuse and drop the new list, or swap.
// Every word is written by exactly one lane.  Temporaries: the single update's per cell, plus 36 + 44 + 29 + 3 words per part.

namespace cm {
namespace {

static_assert(sizeof(cm_mem_image_update) == 8 + 6 * sizeof(void*) && sizeof(cm_mem_image_result) == 256, "sizes as the header states them");

// a part as its lanes see it: the image's list and offsets, where the new list and the new handle words go
struct ImgPart {
  const uint32_t* nodes;
  const uint32_t* off;
  uint4* out;          // cap records
  uint32_t* words;     // IMG_DEV_WORDS
  uint32_t n_old, cap, has_old, reserved0;
  ImgSlices sl;        // inside the part's slice of the dirty records
};
static_assert(sizeof(ImgPart) % 16 == 0, "a table of these keeps the arrays behind it on a 16-byte boundary");

// dpre[b] = the dirty records of the parts before b plus b (one sentinel slot behind every part's records: rank, ins, scan and the
// records themselves share that index); mpre[b] = the merge lanes (old and dirty records) of the parts before b
struct ImgBatch {
  const ImgPart* part;
  uint32_t* res;            // IMG_DEV_WORDS per part: IW_MISMATCH, IW_ROOT, IW_OFF ..
  const uint32_t* dpre;
  const uint32_t* mpre;
  uint4* dirty;
  uint32_t B;
  __device__ __forceinline__ uint4* dirty_of(uint32_t b) const { return dirty + 2 * (size_t)dpre[b]; }
};

// ---- kernels -----------------------------------------------------------------------------------------------------------
// off = lvl[0]: the cells' prefix; a, old_values and cur are the concatenation's
__global__ void __launch_bounds__(SET_BLOCK)
k_imgs_check(ImgBatch ib, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a, uint32_t n, const uint32_t* __restrict__ old_values,
             uint32_t* __restrict__ cur) {
  const uint32_t u = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (u >= 2u * n) return;
  const uint32_t b = compose_part_of(off, ib.B, u >> 1);
  const ImgPart& pt = ib.part[b];
  set_gather_half(pt.nodes, pt.off, a, u, cur);
  if (pt.has_old && (old_values[2 * (size_t)u] != cur[2 * (size_t)u] || old_values[2 * (size_t)u + 1] != cur[2 * (size_t)u + 1]))
    atomicMin(ib.res + IMG_DEV_WORDS * (size_t)b + IW_MISMATCH, (u >> 1) - off[b]);
}

__global__ void __launch_bounds__(SET_BLOCK)
k_imgs_cells(ImgBatch ib, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a, const uint4* __restrict__ new_values, uint32_t n,
             uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (t >= n) return;
  const uint32_t b = compose_part_of(off, ib.B, t), at = off[b];
  out[t] = img_cell_records(a[t], new_values[t], t - at, off[b + 1] - at, ib.dirty_of(b));
}

// in = every part's S_k at its slice, out = every part's S_{k+1} (n_out nodes in all), as k_batch_level
__global__ void __launch_bounds__(SET_BLOCK)
k_imgs_level(BatchView v, ImgBatch ib, TreeDefaults dflt, const uint32_t* __restrict__ in, uint32_t k, uint32_t n_out, uint32_t* __restrict__ out) {
  const uint32_t g = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (g >= n_out) return;
  const uint32_t* const row = v.level(k + 1);
  const uint32_t p = compose_part_of(row, v.B, g), r = g - row[p];
  const BatchPart bp = batch_part(v, p);
  const ImgPart& pt = ib.part[p];
  // (r < |S_{k+1}| of the part <= its cells: inside its slice of the node buffers and of its depth's dirty records)
  out[bp.at + r] = img_parent(set_parent_from(bp.s, k, r, bp.q0), in + bp.at, k, ImgTree{pt.nodes, pt.off, ib.dirty_of(p)}, dflt, pt.sl.o[2 + k] + r);
}

// part blockIdx.x: its S_k0 (at most SET_TAIL nodes: the host plan's k_tail) up to the top, which is its root
__global__ void __launch_bounds__(SET_TAIL)
k_imgs_tail(BatchView v, ImgBatch ib, TreeDefaults dflt, const uint32_t* __restrict__ in, uint32_t k0) {
  __shared__ uint32_t level[2][SET_TAIL];
  __shared__ uint32_t w[SET_STEPS];
  const uint32_t t = threadIdx.x, p = blockIdx.x;
  const BatchPart bp = batch_part(v, p);
  const ImgPart& pt = ib.part[p];
  const ImgTree tr{pt.nodes, pt.off, ib.dirty_of(p)};
  if (t < SET_STEPS) {
    const uint32_t* const row = v.level(t);
    const uint32_t width = row[p + 1] - row[p];
    w[t] = width < SET_TAIL ? width : SET_TAIL;   // (the plan's are at most SET_TAIL from k0 on)
  }
  __syncthreads();
  if (t < w[k0]) level[0][t] = in[bp.at + t];
  __syncthreads();
  uint32_t cur = 0;
#pragma unroll 1
  for (uint32_t k = k0; k < SET_DEPTHS; k++) {
    if (t < w[k + 1]) level[cur ^ 1][t] = img_parent(set_parent_from(bp.s, k, t, bp.q0), level[cur], k, tr, dflt, pt.sl.o[2 + k] + t);
    __syncthreads();
    cur ^= 1;
  }
  if (t == 0) ib.res[IMG_DEV_WORDS * (size_t)p + IW_ROOT] = level[cur][0];
}

// lane g = dpre[b] + j: dirty record j of part b, or (j = the part's count) its sentinel; n_lanes = dpre[B]
__global__ void __launch_bounds__(SET_BLOCK)
k_imgs_rank(ImgBatch ib, uint32_t n_lanes, uint32_t* __restrict__ rank, uint32_t* __restrict__ ins) {
  const uint32_t g = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (g >= n_lanes) return;
  const uint32_t b = compose_part_of(ib.dpre, ib.B, g), at = ib.dpre[b];
  const ImgPart& pt = ib.part[b];
  img_rank_lane(pt.nodes, pt.off, reinterpret_cast<const uint32_t*>(ib.dirty_of(b)), pt.sl, g - at, rank + at, ins + at);
}

// lane g = mpre[b] + t: old record t of part b, or its dirty record t - n_old; n_lanes = mpre[B]
__global__ void __launch_bounds__(SET_BLOCK)
k_imgs_merge(ImgBatch ib, uint32_t n_lanes, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ scan) {
  const uint32_t g = blockIdx.x * SET_BLOCK + threadIdx.x;
  if (g >= n_lanes) return;
  const uint32_t b = compose_part_of(ib.mpre, ib.B, g), at = ib.dpre[b];
  const ImgPart& pt = ib.part[b];
  img_merge_lane(reinterpret_cast<const uint4*>(pt.nodes), pt.n_old, ib.dirty_of(b), pt.sl, rank + at, scan + at, scan[at], pt.cap, pt.out, g - ib.mpre[b]);
}

// part blockIdx.x: its handle words — what the fold left in the result words, then the depth offsets of the merged list
__global__ void __launch_bounds__(64)
k_imgs_offsets(ImgBatch ib, const uint32_t* __restrict__ scan) {
  const uint32_t t = threadIdx.x, b = blockIdx.x;
  if (t >= IMG_DEV_WORDS) return;
  const ImgPart& pt = ib.part[b];
  uint32_t* const res = ib.res + IMG_DEV_WORDS * (size_t)b;
  const uint32_t* const sc = scan + ib.dpre[b];
  uint32_t word = 0;
  if (t < IW_OFF) word = res[t];
  else if (t - IW_OFF <= IMG_SLICES) word = pt.off[t - IW_OFF] + (sc[pt.sl.o[t - IW_OFF]] - sc[0]);
  if (t >= IW_OFF) res[t] = word;
  pt.words[t] = word;
}

// ---- the device path -------------------------------------------------------------------------------------------------------
inline size_t img_round4(size_t x) { return (x + 3) & ~(size_t)3; }

// one part that passed the host's checks, in the plan's order
struct ImgJob {
  uint32_t i = 0;                       // the caller's index
  cm_mem_image* img = nullptr;
  const cm_mem_image_update* u = nullptr;
  DeviceUpdate up;
  uint32_t mismatch = NO_CELL, cur4[4] = {0, 0, 0, 0}, root = 0;
};

// Enqueues the updates of all jobs and makes the call's one round trip (one more per part whose old values differ, for the value
// the message names).  Nothing is swapped here.
void device_update_many(std::vector<ImgJob>& jobs, const BatchPlan& bp, hipStream_t st) {
  const uint32_t B = bp.B, N = bp.N;
  CM_CHECK(B == jobs.size() && B > 0, "memory image: the plan does not hold every part");
  constexpr size_t PW = sizeof(ImgPart) / 4;
  std::vector<uint32_t> dpre(B + 1, 0u), mpre(B + 1, 0u);
  std::vector<ImgPart> table(B);
  bool any_old = false;
  uint64_t lanes = 0;
  for (uint32_t b = 0; b < B; b++) {
    ImgJob& j = jobs[b];
    ImgPart& pt = table[b];
    memset(&pt, 0, sizeof(pt));
    const uint32_t n = j.u->n;
    pt.sl.o[0] = 0; pt.sl.o[1] = 2 * n; pt.sl.o[2] = 3 * n;
    for (uint32_t k = 0; k < SET_DEPTHS; k++) pt.sl.o[3 + k] = pt.sl.o[2 + k] + (bp.level(k + 1)[b + 1] - bp.level(k + 1)[b]);
    pt.sl.o[IMG_SLICES + 1] = pt.sl.o[IMG_SLICES];
    const uint32_t n_dirty = pt.sl.o[IMG_SLICES];
    CM_CHECK(j.img->n_nodes + n_dirty < (1ull << 32), "memory image: the tree is too large");
    pt.n_old = (uint32_t)j.img->n_nodes;
    pt.cap = pt.n_old + n_dirty;
    pt.has_old = j.u->old_values ? 1u : 0u;
    any_old = any_old || pt.has_old;
    dpre[b + 1] = dpre[b] + n_dirty + 1;
    lanes += (uint64_t)pt.n_old + n_dirty;
    CM_CHECK(lanes < (1ull << 32), "cm_mem_images_apply: the images and their updates hold 2^32 records or more together: apply in groups");
    mpre[b + 1] = (uint32_t)lanes;
  }
  const uint32_t D = dpre[B];
  // the new lists and handle words, from the pool before the first launch
  for (uint32_t b = 0; b < B; b++) {
    jobs[b].up.words.alloc(IMG_DEV_WORDS * 4);
    jobs[b].up.nodes.alloc((size_t)table[b].cap * 32);
    table[b].nodes = jobs[b].img->d_nodes.u32();
    table[b].off = jobs[b].img->d_off();
    table[b].out = jobs[b].up.nodes.as<uint4>();
    table[b].words = jobs[b].up.words.u32();
  }
  // the block, every array on a 16-byte boundary: res[36 B] | table[44 B] | lvl[29 (B + 1)] | woff[B + 1] (zeros: no words) |
  // dpre[B + 1] | mpre[B + 1] | addresses[N] | new values[4 N] | old values[4 N] (when any part has them)
  const size_t at_tab = img_round4((size_t)IMG_DEV_WORDS * B), at_lvl = at_tab + PW * B, at_woff = at_lvl + img_round4((size_t)SET_STEPS * (B + 1)),
               at_dpre = at_woff + img_round4(B + 1), at_mpre = at_dpre + img_round4(B + 1), at_addr = at_mpre + img_round4(B + 1),
               at_new = at_addr + img_round4(N), at_old = at_new + 4 * (size_t)N, total = at_old + (any_old ? 4 * (size_t)N : 0);
  std::vector<uint32_t> block(total, 0u);
  memcpy(block.data() + at_tab, table.data(), sizeof(ImgPart) * B);
  memcpy(block.data() + at_lvl, bp.lvl.data(), bp.lvl.size() * 4);
  memcpy(block.data() + at_dpre, dpre.data(), dpre.size() * 4);
  memcpy(block.data() + at_mpre, mpre.data(), mpre.size() * 4);
  const uint32_t* const off = bp.level(0);
  for (uint32_t b = 0; b < B; b++) {
    const cm_mem_image_update& u = *jobs[b].u;
    block[(size_t)IMG_DEV_WORDS * b + IW_MISMATCH] = NO_CELL;
    memcpy(block.data() + at_addr + off[b], u.addresses, (size_t)u.n * 4);
    memcpy(block.data() + at_new + 4 * (size_t)off[b], u.new_values, (size_t)u.n * 16);
    if (u.old_values) memcpy(block.data() + at_old + 4 * (size_t)off[b], u.old_values, (size_t)u.n * 16);
  }
  DevBuf d_block(total * 4), d_heads(bp.n_heads * 4), d_cur((size_t)N * 16), d_a((size_t)N * 4), d_b((size_t)N * 4), d_dirty((size_t)D * 32),
      d_rank((size_t)D * 4), d_ins((size_t)D * 4), d_scan((size_t)D * 4), flag, scan, tmp, tmp_ins;
  const StreamWait wait{st};   // nothing goes back to the pool while the stream still runs, on the error paths too
  stage_upload(d_block.p, block.data(), total * 4, st);
  uint32_t* const d_res = d_block.u32();
  const uint32_t* const d_lvl = d_block.u32() + at_lvl;
  const uint32_t* const d_addr = d_block.u32() + at_addr;
  const ImgBatch ib{reinterpret_cast<const ImgPart*>(d_block.u32() + at_tab), d_res, d_block.u32() + at_dpre, d_block.u32() + at_mpre, d_dirty.as<uint4>(), B};
  const TreeDefaults dflt = tree_defaults();
  {
    const KProfScope kp("k_imgs_check", 0, st);
    hipLaunchKernelGGL(k_imgs_check, blocks_for(2ull * N, SET_BLOCK), dim3(SET_BLOCK), 0, st, ib, d_lvl, d_addr, N,
                       (const uint32_t*)(any_old ? d_block.u32() + at_old : nullptr), d_cur.u32());
  }
  uint32_t* in = d_a.u32();
  uint32_t* out = d_b.u32();
  {
    const KProfScope kp("k_imgs_cells", 0, st);
    hipLaunchKernelGGL(k_imgs_cells, blocks_for(N, SET_BLOCK), dim3(SET_BLOCK), 0, st, ib, d_lvl, d_addr, (const uint4*)(d_block.u32() + at_new), N, in);
  }
  parts_flags_and_scan(d_addr, d_lvl, B, N, flag, scan, tmp, st);
  const BatchView v{d_lvl, d_block.u32() + at_woff, nullptr, d_addr, flag.as<unsigned long long>(), scan.as<unsigned long long>(), d_heads.u32(), nullptr, B,
                    (uint32_t)bp.n_heads};
  hipLaunchKernelGGL(k_batch_heads, blocks_for((uint64_t)SET_DEPTHS * N, SET_BLOCK), dim3(SET_BLOCK), 0, st, v, N, d_heads.u32());
  for (uint32_t k = 0; k < bp.k_tail; k++) {
    const uint32_t n_out = bp.steps[k + 1].n_nodes;
    const KProfScope kp("k_imgs_level", 0, st);
    hipLaunchKernelGGL(k_imgs_level, blocks_for(n_out, SET_BLOCK), dim3(SET_BLOCK), 0, st, v, ib, dflt, (const uint32_t*)in, k, n_out, out);
    std::swap(in, out);
  }
  {
    const KProfScope kp("k_imgs_tail", 0, st);
    hipLaunchKernelGGL(k_imgs_tail, dim3(B), dim3(SET_TAIL), 0, st, v, ib, dflt, (const uint32_t*)in, bp.k_tail);
  }
  // the merge into the new lists; every handle keeps its old one until its part has passed every check
  {
    const KProfScope kp("k_imgs_rank", 0, st);
    hipLaunchKernelGGL(k_imgs_rank, blocks_for(D, SET_BLOCK), dim3(SET_BLOCK), 0, st, ib, D, d_rank.u32(), d_ins.u32());
  }
  size_t bytes = 0;
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_ins.u32(), d_scan.u32(), (int)D, st));
  tmp_ins.alloc(bytes ? bytes : 4);
  CM_HIP(hipcub::DeviceScan::ExclusiveSum(tmp_ins.p, bytes, d_ins.u32(), d_scan.u32(), (int)D, st));
  {
    const KProfScope kp("k_imgs_merge", 0, st);
    hipLaunchKernelGGL(k_imgs_merge, blocks_for(mpre[B], SET_BLOCK), dim3(SET_BLOCK), 0, st, ib, mpre[B], (const uint32_t*)d_rank.u32(), (const uint32_t*)d_scan.u32());
  }
  {
    const KProfScope kp("k_imgs_offsets", 0, st);
    hipLaunchKernelGGL(k_imgs_offsets, dim3(B), dim3(64), 0, st, ib, (const uint32_t*)d_scan.u32());
  }
  CM_HIP(hipGetLastError());
  std::vector<uint32_t> land((size_t)IMG_DEV_WORDS * B);
  download(land.data(), d_res, land.size() * 4, st);
  for (uint32_t b = 0; b < B; b++) {
    ImgJob& j = jobs[b];
    const uint32_t* const mine = land.data() + (size_t)IMG_DEV_WORDS * b;
    j.mismatch = mine[IW_MISMATCH];
    j.root = mine[IW_ROOT];
    memcpy(j.up.off, mine + IW_OFF, (IMG_SLICES + 1) * 4);
    if (j.mismatch != NO_CELL) {
      CM_CHECK(j.mismatch < j.u->n, "memory image: the device names a cell outside the update");
      download(j.cur4, d_cur.u32() + 4 * ((size_t)off[b] + j.mismatch), 16, st);
    }
    CM_CHECK(j.up.off[IMG_SLICES] >= table[b].n_old && j.up.off[IMG_SLICES] <= table[b].cap,
             "memory image: the device counts more records than the merge can make");
  }
}

void set_result(cm_mem_image_result& r, const CmError& e) {
  r.status = e.code ? e.code : 1;
  snprintf(r.message, sizeof(r.message), "%s", e.what());
}

}  // namespace
}  // namespace cm

extern "C" int32_t cm_mem_images_apply(const cm_mem_image_update* parts, uint32_t n_parts, cm_mem_image_result* results) {
  using namespace cm;
  return abi_guard([&] {
    // the call's own refusals: before any address is read and before the device is asked for
    const std::string head = "cm_mem_images_apply: ";
    CM_CHECK(parts && results, head + "null argument");
    CM_CHECK(n_parts >= 1 && n_parts <= BATCH_MAX_PARTS, head + "no parts, or more than 2^16 parts in one call: apply in groups");
    uint64_t cells = 0;
    std::vector<std::pair<cm_mem_image*, uint32_t>> by_handle(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) {
      const std::string part = head + "part " + std::to_string(i);
      CM_CHECK(parts[i].struct_size >= sizeof(cm_mem_image_update), part + ": struct_size does not cover cm_mem_image_update (set it to sizeof(cm_mem_image_update))");
      CM_CHECK(parts[i].img, part + ": null image");
      cells += parts[i].n;
      by_handle[i] = {parts[i].img, i};
    }
    CM_CHECK(cells <= SET_MAX_CELLS, head + "the parts hold " + std::to_string(cells) + " cells, more than 2^20 in one call: apply in groups");
    // one global order of the handles, by address: the locks are taken in it, and two parts of one image stand side by side
    std::sort(by_handle.begin(), by_handle.end(), [](const auto& x, const auto& y) {
      return x.first != y.first ? std::less<cm_mem_image*>()(x.first, y.first) : x.second < y.second;
    });
    for (uint32_t i = 1; i < n_parts; i++)
      CM_CHECK(by_handle[i].first != by_handle[i - 1].first,
               head + "parts " + std::to_string(by_handle[i - 1].second) + " and " + std::to_string(by_handle[i].second) +
                   " name one image: updates of one image depend on each other and do not belong in one fold (apply them one after the other)");
    for (uint32_t i = 0; i < n_parts; i++) memset(&results[i], 0, sizeof(results[i]));
    // check 1 of every part, in the single call's words: a part's own verdict, and such a part never reaches a kernel
    std::vector<uint32_t> alive;
    for (uint32_t i = 0; i < n_parts; i++) {
      const cm_mem_image_update& p = parts[i];
      try {
        CM_CHECK(p.img->device, head + "device images only: a host image takes its updates through cm_mem_image_apply");
        CM_CHECK(p.addresses && p.new_values, "cm_mem_image_apply: null argument");
        check_update_addresses("cm_mem_image_apply", p.addresses, p.n);
        alive.push_back(i);
      } catch (const CmError& e) { set_result(results[i], e); }
    }
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(n_parts);
    for (const auto& h : by_handle) locks.emplace_back(h.first->mu);
    for (uint32_t i = 0; i < n_parts; i++) results[i].root = parts[i].img->root;
    try { open_require_device("cm_mem_images_apply"); }
    catch (const CmError& e) {
      for (uint32_t i : alive) set_result(results[i], e);
      throw;
    }
    // checks 2 and 3: the host holds what they read
    std::vector<ImgJob> jobs;
    std::vector<const uint32_t*> addrs;
    std::vector<uint32_t> counts;
    for (uint32_t i : alive) {
      const cm_mem_image_update& p = parts[i];
      try {
        check_new_words(p.addresses, p.n, p.new_values);
        check_root_before(*p.img, p.root_before);
      } catch (const CmError& e) { set_result(results[i], e); continue; }
      jobs.emplace_back();
      jobs.back().i = i; jobs.back().img = p.img; jobs.back().u = &p;
      addrs.push_back(p.addresses);
      counts.push_back(p.n);
    }
    if (!jobs.empty()) {
      bind_thread_to_library_device();
      BatchPlan bp;
      batch_plan(addrs.data(), counts.data(), nullptr, (uint32_t)jobs.size(), bp);
      device_update_many(jobs, bp, thread_main_stream());
      // checks 4 and 6, part by part; the image changes only behind the last of them
      for (ImgJob& j : jobs) {
        const cm_mem_image_update& p = *j.u;
        try {
          if (j.mismatch != NO_CELL) old_differs(p.addresses, p.old_values, j.mismatch, j.cur4);
          check_root_after(p.root_after, j.root);
        } catch (const CmError& e) { set_result(results[j.i], e); continue; }
        cm_mem_image& img = *j.img;
        img.d_nodes = std::move(j.up.nodes);
        img.d_words = std::move(j.up.words);
        memcpy(img.off, j.up.off, sizeof(img.off));
        img.n_nodes = img.off[IMG_SLICES];
        img.root = j.root;
        results[j.i].root = j.root;
      }
    }
    for (uint32_t i = 0; i < n_parts; i++)
      if (results[i].status) throw CmError(results[i].status, "part " + std::to_string(i) + ": " + results[i].message);
  });
}
