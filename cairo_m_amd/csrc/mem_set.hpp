// Set openings (mem_set.hip): the one rule that says which nodes of a set need a sibling word, the plan of a set's verification
// and the host fold.  The addresses a[0] < a[1] < ... < a[n-1] < 2^28 are strictly ascending; S_k = the ascending list of distinct
// a[i] >> k = the nodes of depth 28 - k on some path.  A node x of S_k needs a sibling exactly when x ^ 1 is not in S_k; the
// record's words come depth by depth, k = 0 first, by ascending node inside a depth, each node(28 - k, x ^ 1).  Host code except
// where CM_HD says otherwise.
#pragma once
#include "../../include/cairom_hip.h"
#include "engine.hpp"
#include "host_adapter.hpp"
#include "mem_range.hpp"
#include "mem_tree.hpp"
#include <string>
#include <vector>

namespace cm {

constexpr uint32_t SET_MAX_CELLS = 1u << 20;   // one call: at most 28 * 2^20 sibling words, 448 B of scan temporaries per cell
constexpr uint32_t SET_DEPTHS = 28;            // k = 0 .. 27
constexpr uint32_t SET_STEPS = 1 + SET_DEPTHS; // the cells, then one step per depth 27 .. 0
// The single-workgroup tail takes a level of at most this many nodes.  128, as RANGE_TAIL: of the sets the tests pin,
// range(777, 5777, 3) (1667 cells, every one with a sibling word and a parent of its own, then 1667, 1250, 625, 313, 157 nodes) and
// the 1500 random cells of the dense block (1500, 1268, 956, 594, 314, 157) run six per-level launches and enter the tail at 79
// nodes, range(1000, 1257) runs two (257, 129) and enters at 65, the three-run set runs one (141) and enters at 72: all above half
// the tail's width.  The per-level steps of the stride-3 set hold parents with only a left or only a right child (depth 28) and
// with both (from depth 27 on), and so do the tail's steps of the three-run set.  A single cell or the two ends of the address
// space enter the tail at width 1 or 2.
constexpr uint32_t SET_TAIL = 128;
enum : uint32_t { SET_K_CELLS = 0, SET_K_LEVEL = 1, SET_K_TAIL = 2 };
enum : uint32_t { SET_HEAD = 1u, SET_NEEDS = 2u };

static_assert(sizeof(cm_mem_set_step) == 16, "plain words, size as the header states it");

// ---- the one rule, host and device ------------------------------------------------------------------------------------------
// Address lane i at shift k: SET_HEAD when the lane is the first of its node x = a[i] >> k of S_k (i == 0, or a[i - 1] >> k
// differs), plus SET_NEEDS when that node needs a sibling word: for an odd x the lane before decides (it lies in x - 1 or further
// left), for an even x the lane `next` = the first lane behind i that lies in another node (n when there is none).  0 for a lane
// that is no head.  The addresses are strictly ascending and below 2^28 (the caller checked).
CM_HD uint32_t set_lane_given_next(const uint32_t* a, uint32_t n, uint32_t i, uint32_t k, uint32_t next) {
  const uint32_t x = a[i] >> k;
  if (i && (a[i - 1] >> k) == x) return 0;
  if (x & 1u) return SET_HEAD | ((i && (a[i - 1] >> k) == x - 1) ? 0u : SET_NEEDS);
  return SET_HEAD | ((next < n && (a[next] >> k) == x + 1) ? 0u : SET_NEEDS);
}
// `next` by bisection of the addresses behind i for (x + 1) << k: what a lane that knows only its own index does (the kernels);
// the host plan walks the heads in order and knows the next one.  Distinct addresses put at most 2^k lanes into a node, so `next`
// is at most i + 2^k.  For any array the bisection reads inside a[0 .. n).
CM_HD uint32_t set_lane(const uint32_t* a, uint32_t n, uint32_t i, uint32_t k) {
  const uint32_t bound = ((a[i] >> k) + 1) << k;   // (at most 2^28)
  const bool asks = !((a[i] >> k) & 1u) && !(i && (a[i - 1] >> k) == (a[i] >> k));   // (only an even head asks)
  uint32_t lo = i + 1, hi = !asks ? lo : (k < 20 && n - i > (1u << k)) ? i + (1u << k) : n;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] < bound) lo = mid + 1; else hi = mid;
  }
  return set_lane_given_next(a, n, i, k, lo);
}
// the first i >= 1 with a[i] <= a[i - 1], or the first i with a[i] >= 2^28 where that comes sooner; n when the addresses are good
inline uint64_t set_first_bad_address(const uint32_t* a, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (a[i] >= RANGE_SPACE || (i && a[i] <= a[i - 1])) return i;
  return n;
}

// ---- the plan: one record per hashing step, consumed by the device verifier and handed out by cm_mem_set_plan ---------------
// steps[0]: the cells -> the n nodes of depth 28.  steps[k + 1]: S_k -> the |S_{k+1}| nodes of depth 27 - k, reading count[k]
// sibling words; the per-level kernel while S_k is wider than SET_TAIL, the tail from there on (consecutive tail steps are one
// launch).  Returns n_siblings.  A lane that is no head at shift k is none at k + 1, so the walk keeps only the heads, and the
// head behind a head is the first lane of the next node: the rule without its bisection, linear in the nodes of all depths.
inline uint32_t mem_set_plan(const uint32_t* a, uint32_t n, cm_mem_set_step steps[SET_STEPS]) {
  std::vector<uint32_t> heads(n), next;
  for (uint32_t i = 0; i < n; i++) heads[i] = i;
  steps[0] = cm_mem_set_step{28, n, 0, SET_K_CELLS};
  uint32_t total = 0;
  for (uint32_t k = 0; k < SET_DEPTHS; k++) {
    uint32_t needs = 0;
    next.clear();
    for (size_t j = 0; j < heads.size(); j++) {
      const uint32_t i = heads[j];
      if (set_lane_given_next(a, n, i, k, j + 1 < heads.size() ? heads[j + 1] : n) & SET_NEEDS) needs++;
      if (i == 0 || (a[i - 1] >> (k + 1)) != (a[i] >> (k + 1))) next.push_back(i);   // (SET_HEAD at shift k + 1; shift 28: lane 0 alone)
    }
    steps[k + 1] = cm_mem_set_step{27 - k, (uint32_t)next.size(), needs, heads.size() > SET_TAIL ? SET_K_LEVEL : SET_K_TAIL};
    total += needs;
    heads.swap(next);
  }
  return total;
}

// ---- what the kernels of the set openings and of the transitions (mem_transition.hip) share, device only ---------------------
constexpr uint32_t SET_BLOCK = 256;
struct SetWidths { uint32_t w[SET_STEPS]; };                  // w[k] = |S_k|, k = 0 .. 28 (the plan's)
// the sibling word of lane t = k * n + i, which has the needs flag: the other half of the pair x & ~1, x = a[i] >> k (the left half
// when x is odd), from depth 28 - k's slice of the node list, or that depth's default hash
__device__ __forceinline__ uint32_t set_gather_word(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a,
                                                    uint32_t n, uint32_t t, const TreeDefaults& dflt) {
  const uint32_t k = t / n, depth = SET_DEPTHS - k, x = a[t % n] >> k;
  const uint32_t* const nd = range_find(nodes, off, depth, x & ~1u);
  return nd ? ((x & 1u) ? nd[2] : nd[3]) : dflt.h[depth];
}
// half u & 1 of the value of cell a[u / 2] into values[2 u], values[2 u + 1]: the pair 4a + 2 * (u & 1) of depth 30, zeros when missing
__device__ __forceinline__ void set_gather_half(const uint32_t* __restrict__ nodes, const uint32_t* __restrict__ off, const uint32_t* __restrict__ a,
                                                uint32_t u, uint32_t* __restrict__ values) {
  const uint32_t* const nd = range_find(nodes, off, air::TREE_HEIGHT, 4u * a[u >> 1] + 2u * (u & 1u));
  values[2 * (size_t)u] = nd ? nd[2] : 0u;
  values[2 * (size_t)u + 1] = nd ? nd[3] : 0u;
}
// what the hashing lanes read: the addresses, the flags and their scan, the head lanes, the record
struct SetView {
  const uint32_t* a;
  const unsigned long long* flag;
  const unsigned long long* scan;
  const uint32_t* heads;
  const uint32_t* words;
  uint32_t n, n_words;
};
// Parent r of S_{k+1}: its first child is node c of S_k.  paired: an even node whose successor in S_k is x + 1, the children are
// nodes c and c + 1.  Else the other child is the sibling word w, on the left when the node is odd; w = P when the record has no
// such word.  x = that first child's index at its depth, a[i] >> k, for a fold that files what it hashes (the image); one that
// does not read it pays nothing for it.  Index arithmetic only: the same for every plane of values folded over the addresses.
// A batch (mem_batch.hip) scans the pairs of many sets at once: the view is then one set's slice of the flags and of the scan with
// `heads` the whole batch's list, and q0 = the low word of the scan at the slice's start, which the word positions are taken from.
struct SetParent { uint32_t c, w, x; bool paired, odd; };
__device__ __forceinline__ SetParent set_parent_from(const SetView& s, uint32_t k, uint32_t r, uint32_t q0) {
  // the parent's head lane is the head lane of its first child: a lane that starts a node at shift k + 1 starts one at shift k
  const uint32_t i = k + 1 < SET_DEPTHS ? s.heads[(uint32_t)(s.scan[(size_t)(k + 1) * s.n] >> 32) + r] : 0u;
  const size_t t = (size_t)k * s.n + i;
  SetParent p;
  p.c = (uint32_t)(s.scan[t] >> 32) - (uint32_t)(s.scan[(size_t)k * s.n] >> 32);
  p.paired = !((uint32_t)s.flag[t] & 1u);
  p.x = s.a[i] >> k;
  p.w = 0u;
  p.odd = false;
  if (p.paired) return p;
  const uint32_t q = (uint32_t)s.scan[t] - q0;
  p.w = q < s.n_words ? s.words[q] : P;
  p.odd = p.x & 1u;
  return p;
}
__device__ __forceinline__ SetParent set_parent(const SetView& s, uint32_t k, uint32_t r) { return set_parent_from(s, k, r, 0u); }

// ---- the host pieces both verifiers and both openers run (mem_set.hip) ---------------------------------------------------------
// flag[t] and scan[t] of the 28 n pairs, enqueued on st (the scan's temporary lives in `tmp` until the stream has run)
void set_flags_and_scan(const uint32_t* d_addr, uint32_t n, DevBuf& flag, DevBuf& scan, DevBuf& tmp, hipStream_t st);
// heads[rank] = the head lane of every node of S_0 .. S_27, depth-major (k_set_heads), n_heads of them
void set_heads_enqueue(const DevBuf& flag, const DevBuf& scan, uint32_t n, uint32_t n_heads, uint32_t* heads, hipStream_t st);
// out[t] = the node of depth 28 of cell t, its four value words range-checked into *bad (k_fold_cells<1> of set_fold.hpp, also the
// first step of the range verifier)
CM_INTERNAL void set_cells_enqueue(const uint32_t* values, uint32_t n, uint32_t* out, uint32_t* bad, hipStream_t st);
// what is wrong with address `bad` = set_first_bad_address(a, n) < n
std::string set_address_complaint(const uint32_t* a, uint64_t bad);
// the host fold: 0 and *root_out, or 11 and the message "<noun> of <n> cells: ...", a bad value named "<value_word> <j> of cell <a>"
// (1: a NULL argument or n > 2^20, behind `who`)
int32_t set_root_host(const char* who, const uint32_t* a, uint64_t n64, const uint32_t* values, const uint32_t* words, uint32_t n_words, uint32_t* root_out,
                      const char* noun = "memory set", const char* value_word = "value word");

// ---- what the run adapter (adapter_run.inc) and the C ABI need --------------------------------------------------------------
// values[4 * n] and siblings[n_siblings] = the opening of the set under the tree whose node list is `nodes`: four launches, one
// scan and one round trip on `st` (one more per further 8 MB).  The addresses are good and n_siblings is the plan's (the caller
// checked); a device count that differs is an error and nothing is written.
void open_set(const cm_merkle_node* nodes, uint64_t n_nodes, const uint32_t* addresses, uint32_t n, uint32_t* values, uint32_t* siblings,
              uint32_t n_siblings, hipStream_t st);
// status 1 unless every pointer is set, 0 < n <= 2^20, the addresses are strictly ascending and below 2^28 and cap_siblings holds
// the record; *n_siblings = the needed count as soon as the addresses are good
void open_set_check(const char* who, const uint32_t* addresses, uint64_t n, const uint32_t* values, const uint32_t* siblings, uint32_t cap_siblings,
                    uint32_t* n_siblings);

}  // namespace cm
