// The two pure-arithmetic checks of verify_prelude on the GPU (cm_verify_many_ex with CM_VERIFY_ARITH_ON_DEVICE; kernels and
// op-level entries: verify_prelude.hip).  Both are exact field arithmetic, so the device gives the host's words bit for bit.
//
// Job formats (flat uint32 words next to the tables of verify_device.hpp; offsets into the blob unless marked scratch):
//   sum jobs   per chunk of at most VP_SUM_THREADS entries of ONE public list, 8 words:
//              [entries_off, n_entries, emit (1: program / input, 0: output), root, rel_off, out (scratch, 4 words), 0, 0]
//              an entry is the 7 words of PublicEntry: present, addr, value[4], clock; rel_off: air::RelationsRaw
//   oods jobs  per (proof, component), component-major across the batch, 12 words (every group's kernel walks the whole list):
//              [component, n_base, tr_off, it_off, pp_off, rel_off, coeff_off, shift_off, log_size, oods_x_off, out (scratch), 0]
//              log_size 0: the numerator alone (cm_point_eval_op); otherwise it is divided by canonic_vanishing(log_size, oods).
//              component VP_NONE: padding (the batch pads every component's jobs to a multiple of 64, so a wave holds one component).
//              coeff: the component's slice of the host's table of random_coeff powers (verify_prelude builds the same table).
//   fin jobs   per proof, 16 words:
//              [do_logup, parts (scratch), n_parts, head_off (7 words), rel_off, claimed_off, n_claimed, logup_flag, sum_out (scratch),
//               do_oods, quotients (scratch), n_quotients, composition_off (4 QM31), oods_flag, 0, 0]
//              sum_out receives initial_logup_sum (the claimed sums not added); a flag of VP_NONE is not written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <vector>
#include "field.hpp"
#include "point_eval.hpp"
#include "proof.hpp"

namespace cm {

constexpr uint32_t VP_SUM_THREADS = 256;   // entries per workgroup of k_verify_public_sum (CM_PUBLIC_SUM_ENTRIES)
constexpr uint32_t VP_SUM_JOB_WORDS = 8, VP_OODS_JOB_WORDS = 12, VP_FIN_JOB_WORDS = 16;
constexpr uint32_t VP_NONE = 0xffffffffu;
constexpr uint32_t VP_REL_WORDS = (uint32_t)(sizeof(air::RelationsRaw) / 4);
enum : uint32_t { VPF_DO_LOGUP = 0, VPF_PARTS, VPF_N_PARTS, VPF_HEAD, VPF_REL, VPF_CLAIMED, VPF_N_CLAIMED, VPF_LOGUP_FLAG, VPF_SUM_OUT,
                  VPF_DO_OODS, VPF_QUOT, VPF_N_QUOT, VPF_COMPOSITION, VPF_OODS_FLAG };

void launch_verify_public_sum(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st);
void launch_verify_oods(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st);   // every group's kernel
// k_verify_oods is one kernel per component group (verify_prelude_oods.inc says why), each in its own translation unit: the felt
// opcodes, the u32 opcodes but the three widest, those three (both U32StoreDiv and U32StoreMulFpFp), and the rest with the builtins
constexpr int VP_OODS_GROUPS = 4;
constexpr int verify_oods_group(int cid) {
  return cid <= air::C_U32_STORE_IMM ? 0
         : (cid == air::C_U32_STORE_DIV_FP_IMM || cid == air::C_U32_STORE_DIV_FP_FP || cid == air::C_U32_STORE_MUL_FP_FP) ? 2
         : cid <= air::C_U32_STORE_SUB_FP_FP ? 1 : 3;
}
template <int G>
void launch_verify_oods_group(const uint32_t* blob, uint32_t* scr, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st);
void launch_verify_prelude_fin(const uint32_t* blob, uint32_t* scr, uint32_t* flags, const uint32_t* jobs, uint32_t n_jobs, hipStream_t st);

inline void relations_words(const HostRelations& rel, uint32_t* w) {   // air::RelationsRaw
  for (int r = 0; r < air::N_RELATIONS; r++) rel.z[r].to_u32(w + 4 * r);
  for (int r = 0; r < air::N_RELATIONS; r++)
    for (int i = 0; i < air::MAX_REL_SIZE; i++) rel.alpha_pow[r][i].to_u32(w + 4 * air::N_RELATIONS + 4 * (r * air::MAX_REL_SIZE + i));
}

// The public data of one proof as sum jobs and the LogUp half of its fin job.  S: put(const uint32_t*, size_t), scratch(size_t).
template <class S>
inline void plan_public_sum(S& s, const PublicData& d, uint32_t rel_off, std::vector<uint32_t>& sum_jobs, uint32_t* fin) {
  static_assert(sizeof(PublicEntry) == 28, "PublicEntry is seven words");
  const uint32_t head[7] = {d.initial_pc, d.initial_fp, d.final_pc, d.final_fp, d.clock, d.initial_root, d.final_root};
  const std::vector<PublicEntry>* lists[3] = {&d.program, &d.input, &d.output};
  size_t n_parts = 0;
  for (auto* l : lists) n_parts += (l->size() + VP_SUM_THREADS - 1) / VP_SUM_THREADS;
  const uint32_t parts = s.scratch(4 * n_parts);
  uint32_t part = 0;
  for (int k = 0; k < 3; k++) {
    const std::vector<PublicEntry>& l = *lists[k];
    const uint32_t off = s.put(reinterpret_cast<const uint32_t*>(l.data()), 7 * l.size());
    for (size_t c0 = 0; c0 < l.size(); c0 += VP_SUM_THREADS, part++) {
      const uint32_t job[VP_SUM_JOB_WORDS] = {off + 7 * (uint32_t)c0, (uint32_t)std::min<size_t>(VP_SUM_THREADS, l.size() - c0), k < 2 ? 1u : 0u,
                                              k < 2 ? d.initial_root : d.final_root, rel_off, parts + 4 * part, 0, 0};
      sum_jobs.insert(sum_jobs.end(), job, job + VP_SUM_JOB_WORDS);
    }
  }
  fin[VPF_DO_LOGUP] = 1;
  fin[VPF_PARTS] = parts;
  fin[VPF_N_PARTS] = (uint32_t)n_parts;
  fin[VPF_HEAD] = s.put(head, 7);
  fin[VPF_REL] = rel_off;
  fin[VPF_SUM_OUT] = s.scratch(4);
}

}  // namespace cm
