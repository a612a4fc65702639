// Memory openings (mem_open.hip): what the run adapter (adapter_run.inc) needs of them.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"

namespace cm {

// the leaves (4a + i, value_i, 1) of an image — lo dense from address 0, hi[i] = the cell at MAX_ADDRESS - i — in ascending index
// order, 4 * (n_lo + n_hi) of them, for partial_merkle_tree_enqueue's device-pointer form.  Enqueued; waits for nothing.
void image_leaves_enqueue(const uint32_t* lo, uint32_t n_lo, const uint32_t* hi, uint32_t n_hi, uint32_t* idx, uint32_t* val, uint32_t* mult,
                          hipStream_t st);
// nodes_out (exact size), n_nodes_out and root_out = the tree over 4 * cells leaves that `fill(idx, val, mult)` enqueues on st in
// ascending index order, through the device tree builder (adapter_run.inc); two waits on `st`
void leaves_tree_build(uint64_t cells, const std::function<void(uint32_t*, uint32_t*, uint32_t*)>& fill, DevBuf& nodes_out, uint64_t& n_nodes_out,
                       uint32_t& root_out, hipStream_t st);
// out[i] = the opening of addresses[i] under the tree whose node list (depth 30..1, ascending index inside a depth) is `nodes`:
// one upload, two launches, one download on `st`, which is waited for.  The addresses are below 2^28 (the caller checked).
void open_paths(const cm_merkle_node* nodes, uint64_t n_nodes, const uint32_t* addresses, uint64_t n, cm_mem_opening* out, hipStream_t st);
// off[j], j = 0 .. 30 (device) = the number of records of `nodes` deeper than 30 - j: the records of depth d are
// [off[30 - d], off[31 - d]) (k_open_depth_offsets, for the range openings of mem_range.hip).  Enqueued; waits for nothing.
void open_depth_offsets_enqueue(const cm_merkle_node* nodes, uint64_t n_nodes, uint32_t* off, hipStream_t st);
// status 1 unless (addresses, out) can take n openings and every address is below 2^28; status 3 without a device
void open_require_device(const char* who);
void open_check_addresses(const char* who, const uint32_t* addresses, uint64_t n, const cm_mem_opening* out);

}  // namespace cm
