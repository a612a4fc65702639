// Batched verification on the GPU (cm_verify_many, cm_verify_run_device): the host plans, the device hashes and folds.
//
// Per proof the host runs verify_prelude (verifier_common.hpp: everything cm_verify_proof does in front of the queries) and then
// walks the query phase SYMBOLICALLY: which witness word a Merkle node consumes and which pair slot a FRI witness value fills
// depends on the query positions alone, never on a hash or a field value, so every structural verdict (WitnessTooShort,
// TooManyQueriedValues, ...EvaluationsInvalid, ...) is final after planning and only three kinds of check are left for the device:
// a tree's root, and the last FRI layer's evaluations.  Every check of a proof, in the host verifier's order, is one SLOT; a slot
// the device decides owns one flag word.  Planning stops at the first slot that fails on the host (nothing behind it is sent), and
// the verdict is the lowest failed slot.
//
// One upload: the BLOB, flat uint32 words, offsets absolute and below 2^31.  A reference with bit 31 set points into the device
// SCRATCH buffer instead (values the kernels produce: answers, FRI pairs, folded evaluations).
//   proof words    per proof: queried values of the 4 trees, hash / column witnesses of every decommitment, FRI witnesses, roots,
//                  the last layer's polynomial
//   sample tables  per (proof, size group): [n_batches, random_coeff[4]] then per batch [point x[4], y[4], n_entries, entries_off];
//                  an entry is [tree << 28 | column within the tree's part of the row, sampled value[4]]
//   answer jobs    per (proof, size group, query row), 8 words: [table_off, row base in the queried values of tree 0..3, log,
//                  position, out (scratch)]
//   FRI program    per proof, VF_* words: the size groups of the first layer ([log, n_pairs, slots_off, pairs_out, folded_out, 0],
//                  a slot is [start, source of value 0, source of value 1]) and the inner layers ([log, n_pairs, slots_off,
//                  pairs_out, alpha[4], n_add, first group to add, n_evals, 0])
//   tree jobs      per (proof, tree), 8 words: [n_levels, levels_off, root_off, flag, 0...]; a level is [n_nodes, nodes_off, columns
//                  absorbed per node, has children]; a node is [left, right, values]: a child is an index into the level below or
//                  (bit 31) the blob offset of a hash witness, values point at queried values, column witness or (bit 31) scratch
//   reduce jobs    per proof: [first flag, n_flags]
// One download: per proof the lowest raised flag, or 0xffffffff (cm_verify_many_detail: the flag words in front of them as well).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "proof.hpp"

namespace cm {

struct VerifyOutcome {
  int32_t check = 0;     // CM_VERIFY_* of the failed check, 0 = accepted
  std::string message;   // the host verifier's string, "" = accepted
};
// one slot of a proof's plan as the batch left it (cm_verify_many_detail)
struct VerifySlotDetail {
  int32_t check = 0;       // CM_VERIFY_* id
  std::string message;     // what the host verifier says when this check fails
  bool on_device = false;  // decided by a kernel (owns a flag word); false: failed while planning
  bool raised = false;     // the flag word was set (or the slot failed while planning)
};
// out[i] = the verdict on proofs[i]; throws CmError for everything that is not a verdict (no device: code 3).
// detail (optional): every proof's slots in the host verifier's order, read from the flag words of the same launches.
// flags: 0 or CM_VERIFY_ARITH_ON_DEVICE (the LogUp sum and the OODS check as the first two slots: verify_prelude.hpp).
void verify_many_device(const ProofData* const* proofs, uint32_t n, const cm_pcs_config& cfg, std::vector<VerifyOutcome>& out, hipStream_t st,
                        std::vector<std::vector<VerifySlotDetail>>* detail = nullptr, uint32_t flags = 0);
// the calling thread's last verify_many_device: plan, upload, kernels, download (ms)
void verify_many_timing(double ms[4]);
// Host code, no GPU: the shapes of the plan verify_many_device would launch for each proof ALONE (read back from the tables the
// planner built, so they are what the kernels would walk).  out[i].struct_size is kept.
void verify_plan_stats(const ProofData* const* proofs, uint32_t n, const cm_pcs_config& cfg, cm_verify_stats* out);

constexpr uint32_t VERIFY_MAX_LEVEL_NODES = 1024;   // two levels of a tree in 64 KB of LDS
constexpr size_t verify_merkle_lds_bytes(uint32_t cap) { return 2 * (size_t)cap * 32; }   // k_verify_merkle: 2 levels x cap nodes x 8 words

}  // namespace cm
