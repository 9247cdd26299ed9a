// Planner of the grouped verifier (cpx_batch_verify_grouped, include/cpx.h) — host code without a HIP call: how a batch of B proofs is cut
// into groups, which proofs the second stage rechecks given the groups' results and the proofs' flag words, what every proof's verdict
// is, and how much of each scratch buffer either stage needs.  One definition for both verifier paths — Engine::located_check (engine.cpp)
// runs the two stages for the host-driven and the device-resident one — and tests/host_emul/locate_plan_emul.cpp, which compiles it for the
// CPU (tests/test_verify_grouped_cpu.py).  check_plan.hpp turns the offsets below into the task lists of either stage and of the fused
// check, whose grouping is this plan for kLocateGroupsMax groups; who fills the scalars is the paths' business (the host's staging in
// verify_core, k_vs_scalars and k_vs_crs_sum_groups on the device).
//
// Stage 1: NT group tasks through Engine::launch_check — group g is ONE bucket MSM over the points of its proofs (up to G * NPT points,
// the fused check's task) and ONE fixed-base task over the CRS scalars summed over its proofs.  Stage 2: the S suspect proofs through
// launch_check again, one task each, slot s of the stage for the s-th suspect in batch order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "../../include/cpx.h"   // verdict codes

namespace cpx {

constexpr long kLocateGroupsMax = 256;       // largest value of option locate_groups_max (and the grouping of cpx_batch_verify_fused)
constexpr uint32_t kLocateFlagDecode = 1u;   // flag word of a proof (VerifyDev::flags, host::VerifyState): a point or scalar did not decode
constexpr uint32_t kLocateFlagStruct = 2u;   // ... vec_T[0] is the identity (curdleproofs.rs:218)

struct LocatePlan {
  size_t B = 0, G = 1, NT = 0;   // proofs, proofs per group (the last group may be short), groups
  size_t group_first(size_t g) const { return g * G; }
  size_t group_count(size_t g) const { return g * G >= B ? 0 : (B - g * G < G ? B - g * G : G); }
  size_t group_of(size_t p) const { return p / G; }
  // One proof per group: stage 1 IS the per-proof check, a failing group is its proof's verdict and there is no second stage.
  bool per_proof() const { return G == 1; }

  // ---- stage 1: NT tasks.  Task g reads the points, scalars and gather entries [g G NPT, + group_count(g) NPT) of the batch ----
  size_t s1_max_n(size_t NPT) const { return G * NPT; }                              // points of the largest task
  size_t s1_points(size_t NPT) const { return B * NPT; }                             // all tasks together
  size_t s1_task_off(size_t g, size_t NPT) const { return g * G * NPT; }             // first point of task g = its conv_off
  size_t s1_task_n(size_t g, size_t NPT) const { return group_count(g) * NPT; }
  size_t s1_crs_scalars(size_t n) const { return NT * n; }                           // the summed CRS scalars, row g at g n
  size_t s1_out_first(size_t g, size_t fix_parts) const { return g * fix_parts; }    // first partial slot of the group's fixed-base task
  // ---- stage 2: S tasks of NPT points, dense ----
  static size_t s2_conv_off(size_t s, size_t NPT) { return s * NPT; }
  static size_t s2_out_first(size_t s, size_t fix_parts) { return s * fix_parts; }
  // ---- scratch of Engine::launch_check for `tasks` tasks of at most `max_n` points, `slices` waves per window ----
  static size_t conv_entries(size_t tasks, size_t max_n) { return 2 * tasks * max_n; }   // P and -phi(P) per point (TAff)
  static size_t digit_words(size_t tasks, size_t max_n) { return 9 * tasks * max_n; }
  static size_t bucket_parts(size_t tasks, size_t slices) { return tasks * 32 * slices; }
  static size_t fix_part_slots(size_t tasks, size_t fix_parts) { return tasks * fix_parts; }
  static size_t result_bytes(size_t tasks) { return tasks * 48; }                        // compressed sums
};

// groups_max = option locate_groups_max (1 .. kLocateGroupsMax; out-of-range values are clamped)
inline LocatePlan locate_plan(size_t B, long groups_max) {
  LocatePlan pl;
  const size_t gm = groups_max < 1 ? 1 : groups_max > kLocateGroupsMax ? (size_t)kLocateGroupsMax : (size_t)groups_max;
  pl.B = B;
  pl.G = B ? (B + gm - 1) / gm : 1;
  pl.NT = (B + pl.G - 1) / pl.G;
  return pl;
}

// The proofs stage 2 rechecks, in batch order: the flag-free proofs of the groups whose sum is not the identity (group_ok[g] == 0).  A
// flagged proof is never rechecked: its verdict is its flag.  An undecodable proof contributes nothing to its group; a structurally
// rejected one keeps its scalars and so sends its group here.
inline void locate_stage2(const LocatePlan& pl, const uint8_t* group_ok, const uint32_t* flags, std::vector<uint32_t>& list) {
  list.clear();
  if (pl.per_proof()) return;
  for (size_t g = 0; g < pl.NT; g++) {
    if (group_ok[g]) continue;
    for (size_t p = pl.group_first(g), e = p + pl.group_count(g); p < e; p++)
      if (!flags[p]) list.push_back((uint32_t)p);
  }
}

// The verdict of every proof.  list / recheck_ok: the stage-2 list and its results (recheck_ok[s] != 0: suspect s sums to the identity);
// both unused when the list is empty.
inline void locate_verdicts(const LocatePlan& pl, const uint8_t* group_ok, const uint32_t* flags, const std::vector<uint32_t>& list, const uint8_t* recheck_ok,
                            int* verdict) {
  for (size_t p = 0; p < pl.B; p++)
    verdict[p] = (flags[p] & kLocateFlagDecode) ? CPX_ERR_DESERIALIZE : (flags[p] & kLocateFlagStruct) ? CPX_ERR_VERIFY : group_ok[pl.group_of(p)] ? CPX_OK : CPX_ERR_VERIFY;
  // (a flag-free proof of a failing group stands as rejected until its own check says otherwise: with one proof per group that is final)
  for (size_t s = 0; s < list.size(); s++)
    if (recheck_ok[s]) verdict[list[s]] = CPX_OK;
}

}  // namespace cpx
