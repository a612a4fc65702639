// What the memory-tree family shares (mem_open, mem_range, mem_set, mem_transition, mem_compose, mem_image, program_id, link): the
// default hashes as a kernel argument, the launch and stream helpers and the chunked download (the guard of their C ABI: abi.hpp).
// None of it is part of the library's exported symbols.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "host_adapter.hpp"
#include "abi.hpp"
#include <algorithm>
#include <cstring>
#include <vector>

namespace cm {

constexpr size_t TREE_LAND_BYTES = (size_t)8 << 20;   // per trip through the pinned landing buffer

struct TreeDefaults { uint32_t h[air::TREE_HEIGHT + 1]; };   // h[d] = the hash of an empty subtree whose top is at depth d
CM_INTERNAL inline TreeDefaults tree_defaults() {
  TreeDefaults dflt;
  const std::vector<uint32_t>& dh = host::poseidon2_default_hashes();
  for (uint32_t d = 0; d <= air::TREE_HEIGHT; d++) dflt.h[d] = dh[d];
  return dflt;
}

CM_INTERNAL inline dim3 blocks_for(uint64_t n, uint32_t block) { return dim3((uint32_t)((n + block - 1) / block)); }

// nothing of a call goes back to the pool while the stream still runs, on the error paths too (declared behind the buffers)
struct CM_INTERNAL StreamWait {
  hipStream_t st;
  ~StreamWait() { (void)hipStreamSynchronize(st); }
};

// `bytes` of device memory at `src` into `dst` through the pinned landing buffer, at most TREE_LAND_BYTES a trip; waits for st
CM_INTERNAL inline void download(void* dst, const void* src, size_t bytes, hipStream_t st) {
  for (size_t done = 0; done < bytes;) {
    const size_t m = std::min(bytes - done, TREE_LAND_BYTES);
    const void* land = stage_download_async((const uint8_t*)src + done, m, st);
    CM_HIP(hipStreamSynchronize(st));
    memcpy((uint8_t*)dst + done, land, m);
    done += m;
  }
}

}  // namespace cm
