// Memory transitions (mem_transition.hip): a set of cells with their values under two roots and ONE list of sibling words — the
// record of a set opening (mem_set.hpp) of the same addresses.  Valid when the set fold of (addresses, old values, words) is the
// root before and the fold of (addresses, new values, words) the root after: the two memories agree in every cell outside the set.
#pragma once
#include "../../include/cairom_hip.h"
#include "mem_set.hpp"
#include "segment_input.hpp"
#include "handles.hpp"   // cm_mem_transition: what cm_input_open_transition hands out

namespace cm {

// The transition of `d` from its initial to its final tree over `addresses` (strictly ascending, below 2^28, 0 < n <= 2^20), or,
// when addresses is nullptr, over the segment's write set, which then never leaves the device between the diff and the opening.
// On the calling thread's stream and pool, which it waits for.  The caller owns the result.
cm_mem_transition* open_transition(const DeviceInput& d, const uint32_t* addresses, uint64_t n);

}  // namespace cm
