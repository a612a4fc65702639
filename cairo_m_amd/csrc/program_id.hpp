// Program identity (program_id.hip): the pieces the host fold and the kernels share.  A program's id (Proof::program_id,
// crates/prover/src/lib.rs:75-97) is the root of the partial memory tree that holds only its public program cells: the dense range
// [first, first + n) whose every outside sibling is the default hash of its depth — the range fold of mem_range.hpp with no record.
// Host code except where CM_HD says otherwise.
#pragma once
#include "../../include/cairom_hip.h"
#include "mem_range.hpp"
#include "mem_tree.hpp"

namespace cm {

constexpr uint32_t PID_ENTRY_WORDS = 7;            // present, address, value[4], clock (cm_proof_public_entries)
constexpr uint32_t PID_MAX_ENTRIES = 1u << 24;     // one program
constexpr uint64_t PID_MAX_BATCH_CELLS = 1ull << 26;   // one batch call: 1 GB of values
constexpr uint32_t PID_MAX_ITEMS = 1u << 20;
constexpr uint32_t PID_TAIL = 1024;                // an interval of at most this many nodes lives in LDS (one lane per node)

// ---- the interval arithmetic: one fold for the host call and k_pid_tree ---------------------------------------------------------
// step k = 0 .. 27 hashes the nodes [lo, hi] of depth 28 - k into [lo >> 1, hi >> 1] of depth 27 - k; once lo == hi the same step
// is the chain to depth 0
CM_HD uint32_t pid_width(uint32_t lo, uint32_t hi) { return hi - lo + 1; }
CM_HD uint32_t pid_child_depth(uint32_t k) { return RANGE_SLOTS - k; }
// the children of parent p, lo >> 1 <= p <= hi >> 1, where in[i] = node lo + i: a child outside the interval is dflt_child, the
// default hash of the children's depth
CM_HD void pid_children(const uint32_t* in, uint32_t lo, uint32_t hi, uint32_t dflt_child, uint32_t p, uint32_t& l, uint32_t& r) {
  range_children(in, lo, hi, dflt_child, dflt_child, p, l, r);
}
CM_HD bool pid_value_bad(const uint32_t* v) { return v[0] >= P || v[1] >= P || v[2] >= P || v[3] >= P; }

}  // namespace cm
