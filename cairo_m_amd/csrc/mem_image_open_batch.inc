// Batched set openings (cm_mem_images_open_memory_sets), behind the batched update at the tail of mem_image.hip: many sets under
// many followed memories — or many sets under ONE, the common case of many clients under one root — through one chain of launches
// and one round trip.  A small set opening is bound by its launches and its two copies, not by hashing or gathering (DESIGN §3.2),
// and independent openings share that chain as the parts of the batched verifier and of the batched update do.  The lanes run the
// single opener's own bodies (set_gather_word, set_gather_half of mem_set.hpp) on the batch layout of mem_batch.hpp.
//
// Host: the call's argument checks, then per part the single call's checks (open_set_check, require_device_image), which read
// nothing the device holds; a part that fails one has its verdict there and is left out.  Device, the same launches whatever the
// number of parts:
//   one upload of one block: per part a table entry (SetPart), the cells' prefix off[], the words' prefix woff[], the default
//                    hashes, the addresses, concatenated;
//   the flag pass over the 28 N pairs, part-major, and ONE scan (parts_flags_and_scan);
//   k_sets_gather    28 N + 2 N lanes.  A pair lane bisects off[] for its part and, with the needs flag, takes the sibling word from
//                    THAT part's node list to the part's slice of the words, at the scan's low word minus the scan at the part's
//                    first pair; the last pair lane of a part stores the part's count.  A lane behind them stores one half of a
//                    cell's value from its part's depth-30 slice.  Every word is written by exactly one lane: no atomic, the same
//                    bytes every time.
//   one download of one block — the counts, the values, the words — in trips of TREE_LAND_BYTES through the pinned landing buffer.
//                    The counts lead the first trip and are ALL compared with the host plan before a byte reaches a caller's array.
// Each image keeps its depth offsets in its handle words (d_off), so no part pays open_depth_offsets_enqueue.  Temporaries: flags
// and scan (448 bytes per cell), the output block (4 + 16 n + 4 n_siblings bytes per part) and 40 bytes per part of tables.  No LDS, no scratch.

namespace cm {
namespace {

static_assert(sizeof(cm_mem_set_request) == 16 + 4 * sizeof(void*) && sizeof(cm_mem_set_result) == 256, "sizes as the header states them");

// a part as its lanes see it: the image's list and offsets, where its values and its words go in the output block
struct SetPart {
  const uint32_t* nodes;
  const uint32_t* off;
  uint32_t* values;    // 4 n
  uint32_t* words;     // woff[p + 1] - woff[p]
};
static_assert(sizeof(SetPart) % 16 == 0, "a table of these keeps the arrays behind it on a 16-byte boundary");

// off, woff: B + 1 each; a: the N addresses of all parts; flag, scan: the 28 N pairs, part-major (depth-major inside a part).
// The default hashes come with the uploaded block: a lane indexes them by its own depth, and as a by-value argument they would
// be copied to 128 bytes of scratch per lane.
__global__ void __launch_bounds__(SET_BLOCK)
k_sets_gather(const SetPart* __restrict__ part, const uint32_t* __restrict__ off, const uint32_t* __restrict__ woff, uint32_t n_parts,
              const uint32_t* __restrict__ a, uint32_t n, const unsigned long long* __restrict__ flag, const unsigned long long* __restrict__ scan,
              const TreeDefaults* __restrict__ dflt, uint32_t* __restrict__ count) {
  const uint32_t t = blockIdx.x * SET_BLOCK + threadIdx.x, n_pairs = SET_DEPTHS * n;
  if (t >= n_pairs) {
    const uint32_t u = t - n_pairs;
    if (u >= 2u * n) return;
    const uint32_t p = compose_part_of(off, n_parts, u >> 1), at = off[p];
    const SetPart& pt = part[p];
    set_gather_half(pt.nodes, pt.off, a + at, u - 2u * at, pt.values);
    return;
  }
  const uint32_t p = compose_part_of(off, n_parts, t / SET_DEPTHS), at = off[p], np = off[p + 1] - at, tl = t - SET_DEPTHS * at;
  const uint32_t needs = (uint32_t)flag[t] & 1u, pos = (uint32_t)scan[t] - (uint32_t)scan[(size_t)SET_DEPTHS * at];
  if (tl == SET_DEPTHS * np - 1) count[p] = pos + needs;
  if (!needs || pos >= woff[p + 1] - woff[p]) return;   // (the host compares count[p] with its plan before it reads a word)
  const SetPart& pt = part[p];
  pt.words[pos] = set_gather_word(pt.nodes, pt.off, a + at, np, tl, *dflt);
}

// one part that passed the host's checks, in the batch's order
struct SetJob {
  uint32_t i = 0;   // the caller's index
  const cm_mem_set_request* q = nullptr;
};

// Enqueues the gather of all jobs, makes the call's round trip and lands every job's values and words in its caller's arrays:
// nothing before every count has been compared.  results[job.i].n_siblings is the host plan's (open_set_check).
void open_sets_device(const std::vector<SetJob>& jobs, const cm_mem_set_result* results, hipStream_t st) {
  const uint32_t B = (uint32_t)jobs.size();
  CM_CHECK(B > 0 && B <= BATCH_MAX_PARTS, "memory sets: no part reached the device path");
  std::vector<uint32_t> off(B + 1, 0u), woff(B + 1, 0u);
  for (uint32_t b = 0; b < B; b++) {
    const uint32_t n = jobs[b].q->n, need = results[jobs[b].i].n_siblings;
    CM_CHECK(n > 0 && need <= SET_DEPTHS * n, "memory sets: a bad set reached the device path");
    off[b + 1] = off[b] + n;
    woff[b + 1] = woff[b] + need;
  }
  const uint32_t N = off[B], W = woff[B];
  CM_CHECK(N <= SET_MAX_CELLS, "memory sets: more than 2^20 cells reached the device path");
  constexpr size_t PW = sizeof(SetPart) / 4;
  // the output block: count[B] | values[4 N] | words[W]; the upload: table[8 B] | off[B + 1] | woff[B + 1] | the default hashes |
  // addresses[N], every array on a 16-byte boundary
  const size_t o_vals = img_round4(B), o_words = o_vals + 4 * (size_t)N, out_words = o_words + W, out_bytes = out_words * 4;
  const size_t at_off = PW * B, at_woff = at_off + img_round4(B + 1), at_dflt = at_woff + img_round4(B + 1),
               at_addr = at_dflt + img_round4(sizeof(TreeDefaults) / 4), total = at_addr + N;
  DevBuf d_block(total * 4), d_out(out_bytes), flag, scan, tmp;
  const StreamWait wait{st};   // nothing goes back to the pool while the stream still runs, on the error paths too
  std::vector<uint32_t> block(total, 0u);
  std::vector<SetPart> table(B);
  for (uint32_t b = 0; b < B; b++) {
    const cm_mem_image& img = *jobs[b].q->img;
    table[b] = SetPart{img.d_nodes.u32(), img.d_off(), d_out.u32() + o_vals + 4 * (size_t)off[b], d_out.u32() + o_words + woff[b]};
    memcpy(block.data() + at_addr + off[b], jobs[b].q->addresses, (size_t)jobs[b].q->n * 4);
  }
  memcpy(block.data(), table.data(), sizeof(SetPart) * B);
  memcpy(block.data() + at_off, off.data(), off.size() * 4);
  memcpy(block.data() + at_woff, woff.data(), woff.size() * 4);
  const TreeDefaults dflt = tree_defaults();
  memcpy(block.data() + at_dflt, &dflt, sizeof(dflt));
  stage_upload(d_block.p, block.data(), total * 4, st);
  const uint32_t* const d_off = d_block.u32() + at_off;
  const uint32_t* const d_addr = d_block.u32() + at_addr;
  parts_flags_and_scan(d_addr, d_off, B, N, flag, scan, tmp, st);
  {
    const KProfScope kp("k_sets_gather", 0, st);
    hipLaunchKernelGGL(k_sets_gather, blocks_for((uint64_t)(SET_DEPTHS + 2) * N, SET_BLOCK), dim3(SET_BLOCK), 0, st,
                       reinterpret_cast<const SetPart*>(d_block.u32()), d_off, (const uint32_t*)(d_block.u32() + at_woff), B, d_addr, N,
                       (const unsigned long long*)flag.as<unsigned long long>(), (const unsigned long long*)scan.as<unsigned long long>(),
                       reinterpret_cast<const TreeDefaults*>(d_block.u32() + at_dflt), d_out.u32());
  }
  CM_HIP(hipGetLastError());
  // the pieces of the block in its own order: every part's values, then every part's words
  struct Piece { size_t at, bytes; uint8_t* to; };
  std::vector<Piece> pieces;
  pieces.reserve(2 * (size_t)B);
  for (uint32_t b = 0; b < B; b++) pieces.push_back({(o_vals + 4 * (size_t)off[b]) * 4, (size_t)jobs[b].q->n * 16, (uint8_t*)jobs[b].q->values});
  for (uint32_t b = 0; b < B; b++) pieces.push_back({(o_words + woff[b]) * 4, (size_t)(woff[b + 1] - woff[b]) * 4, (uint8_t*)jobs[b].q->siblings});
  static_assert((size_t)BATCH_MAX_PARTS * 4 <= TREE_LAND_BYTES, "every part's count comes back in the first trip");
  size_t next = 0;
  for (size_t done = 0; done < out_bytes;) {
    const size_t m = std::min(out_bytes - done, TREE_LAND_BYTES);
    const uint8_t* const land = (const uint8_t*)stage_download_async(d_out.as<uint8_t>() + done, m, st);
    CM_HIP(hipStreamSynchronize(st));   // (also keeps the temporaries alive until the kernels have run)
    if (!done)   // nothing reaches a caller's array before every part's count has been compared
      for (uint32_t b = 0; b < B; b++) {
        const uint32_t got = ((const uint32_t*)land)[b], need = woff[b + 1] - woff[b];
        CM_CHECK(got == need, "memory sets: part " + std::to_string(jobs[b].i) + ": the device counts " + std::to_string(got) +
                                  " sibling words where the host plan has " + std::to_string(need));
      }
    // bytes [done, done + m) of the block: what they hold of the pieces from `next` on
    for (; next < pieces.size(); next++) {
      const Piece& pc = pieces[next];
      const size_t lo = std::max(pc.at, done), hi = std::min(pc.at + pc.bytes, done + m);
      if (lo < hi) memcpy(pc.to + (lo - pc.at), land + (lo - done), hi - lo);
      if (pc.at + pc.bytes > done + m) break;   // the rest of it comes with the next trip
    }
    done += m;
  }
}

void set_result(cm_mem_set_result& r, const CmError& e) {
  r.status = e.code ? e.code : 1;
  snprintf(r.message, sizeof(r.message), "%s", e.what());
}

}  // namespace
}  // namespace cm

extern "C" int32_t cm_mem_images_open_memory_sets(const cm_mem_set_request* parts, uint32_t n_parts, cm_mem_set_result* results) {
  using namespace cm;
  return abi_guard([&] {
    // the call's own refusals: before any address is read and before the device is asked for
    const std::string head = "cm_mem_images_open_memory_sets: ";
    CM_CHECK(parts && results, head + "null argument");
    CM_CHECK(n_parts >= 1 && n_parts <= BATCH_MAX_PARTS, head + "no parts, or more than 2^16 parts in one call: open in groups");
    uint64_t cells = 0;
    std::vector<cm_mem_image*> imgs(n_parts);
    for (uint32_t i = 0; i < n_parts; i++) {
      const std::string part = head + "part " + std::to_string(i);
      CM_CHECK(parts[i].struct_size >= sizeof(cm_mem_set_request), part + ": struct_size does not cover cm_mem_set_request (set it to sizeof(cm_mem_set_request))");
      CM_CHECK(parts[i].img, part + ": null image");
      cells += parts[i].n;
      imgs[i] = parts[i].img;
    }
    CM_CHECK(cells <= SET_MAX_CELLS, head + "the parts hold " + std::to_string(cells) + " cells, more than 2^20 in one call: open in groups");
    for (uint32_t i = 0; i < n_parts; i++) memset(&results[i], 0, sizeof(results[i]));
    // the single call's argument checks, in its words: a part's own verdict, and such a part never reaches a kernel
    std::vector<uint8_t> good(n_parts, 0);
    for (uint32_t i = 0; i < n_parts; i++) {
      const cm_mem_set_request& p = parts[i];
      try {
        open_set_check("cm_mem_image_open_memory_set", p.addresses, p.n, p.values, p.siblings, p.cap_siblings, &results[i].n_siblings);
        good[i] = 1;
      } catch (const CmError& e) { set_result(results[i], e); }
    }
    // openings only read: one image may stand behind many parts.  Each distinct handle's mutex once, in the one global order of
    // the handles, by address, and held until the download has landed
    std::sort(imgs.begin(), imgs.end(), std::less<cm_mem_image*>());
    imgs.erase(std::unique(imgs.begin(), imgs.end()), imgs.end());
    std::vector<std::unique_lock<std::mutex>> locks;
    locks.reserve(imgs.size());
    for (cm_mem_image* h : imgs) locks.emplace_back(h->mu);
    std::vector<SetJob> jobs;
    for (uint32_t i = 0; i < n_parts; i++) {
      results[i].root = parts[i].img->root;
      if (!good[i]) continue;
      try { require_device_image(*parts[i].img, "cm_mem_image_open_memory_set"); }
      catch (const CmError& e) { set_result(results[i], e); continue; }
      jobs.push_back(SetJob{i, &parts[i]});
    }
    try {
      open_require_device("cm_mem_images_open_memory_sets");
      if (!jobs.empty()) {
        bind_thread_to_library_device();
        open_sets_device(jobs, results, thread_main_stream());
      }
    } catch (const CmError& e) {
      for (const SetJob& j : jobs) set_result(results[j.i], e);
      throw;
    }
    for (uint32_t i = 0; i < n_parts; i++)
      if (results[i].status) throw CmError(results[i].status, "part " + std::to_string(i) + ": " + results[i].message);
  });
}
