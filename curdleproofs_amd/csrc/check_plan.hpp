// Layout and task lists of the verifier's accumulated check — host code without a HIP call (kernels.h is included for the task types
// only).  The check is one fixed-base MSM over the CRS scalars plus one bucket MSM over the per-proof points R | S | T | U | slots, in
// three modes (per proof: cpx_batch_verify; fused: cpx_batch_verify_fused; grouped in two stages: cpx_batch_verify_grouped,
// locate_plan.hpp) and on two paths (host-driven: engine.cpp verify_core; device-resident: engine_device.cpp).  Where a proof's scalars
// sit, what its gather list is and what every mode's MsmTask / FixTask look like is written here once; the paths differ in the three
// base addresses they hand in and in who fills the scalars (the host's staging, or k_vs_scalars and k_vs_crs_sum_groups).
// tests/host_emul/check_plan_emul.cpp compiles it for the CPU (tests/test_check_plan_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "kernels.h"
#include "layout.hpp"
#include "locate_plan.hpp"

namespace cpx {

// The ONE scalar layout, over three base addresses (device buffers, or the host's staging copy of them).
template <class F>
struct CheckScalars {
  F* pts = nullptr;    // per-proof point scalars: NPT per proof, in the order of the proof's points
  F* crs = nullptr;    // per-proof CRS scalars: n per proof
  F* sums = nullptr;   // CRS scalars summed over a range of proofs: n per row (one row per group; the fused check: row 0 over all proofs)
  size_t NPT = 0, n = 0;
  F* of_proof(size_t p) const { return pts + p * NPT; }
  F* crs_of(size_t p) const { return crs + p * n; }
  F* sum_row(size_t g) const { return sums + g * n; }
};

struct CheckPlan {
  size_t B = 0, n = 0;             // proofs, CRS scalars per proof
  size_t NI = 0, NM = 0, NPT = 0;  // instance points (R | S | T | U), misc points (slot s is misc point s: layout.hpp), both
  const Aff* points = nullptr;     // row 0 of the per-proof points; a row's first NPT entries are the check's points, in scalar order
  size_t pp_stride = 0;            // entries per row
  const uint32_t* row_idx = nullptr;   // device: 0 .. NPT - 1, the gather list relative to a proof's row (per-proof tasks)
  const uint32_t* gidx = nullptr;      // device: the global gather list (gather(); every other task)
  CheckScalars<const Fr> at;           // device addresses of the scalars

  CheckPlan() = default;
  CheckPlan(size_t B_, size_t ell, size_t L, size_t n_) : B(B_), n(n_), NI(4 * ell), NM((size_t)SL_A + (size_t)ProofLayout(L).n_points()), NPT(NI + NM) {}
  // the device addresses: the per-proof points, the two gather lists (null where a mode has no use for one) and the scalars' three bases
  void place(const Aff* points_, size_t pp_stride_, const uint32_t* row_idx_, const uint32_t* gidx_, const Fr* pts, const Fr* crs, const Fr* sums) {
    points = points_, pp_stride = pp_stride_, row_idx = row_idx_, gidx = gidx_;
    at = CheckScalars<const Fr>{pts, crs, sums, NPT, n};
  }
  size_t n_points() const { return B * NPT; }   // of the whole batch = entries of the gather list and of `at.pts`

  // the global gather list: point i of proof p, relative to `points` (gather_proof: proof p's NPT entries of it)
  void gather_proof(size_t p, uint32_t* out) const {
    for (size_t i = 0; i < NPT; i++) out[p * NPT + i] = (uint32_t)(p * pp_stride + i);
  }
  void gather(uint32_t* out) const {
    for (size_t p = 0; p < B; p++) gather_proof(p, out);
  }

  // ---- per proof: B tasks (launch_check) ----
  void proof_tasks(size_t fix_parts, MsmTask* mt, FixTask* ft) const {
    for (size_t p = 0; p < B; p++) {
      mt[p] = MsmTask{points + p * pp_stride, row_idx, at.of_proof(p), (uint32_t)NPT, 0, (uint32_t)(p * NPT)};
      ft[p] = crs_task(at.crs_of(p), p * fix_parts);
    }
  }
  // ---- the groups of `lp`, stage 1 of the grouped check: lp.NT tasks (launch_check), every group's CRS part from its sums row ----
  void group_tasks(const LocatePlan& lp, size_t fix_parts, MsmTask* mt, FixTask* ft) const {
    group_msm_tasks(lp, mt);
    for (size_t g = 0; g < lp.NT; g++) ft[g] = crs_task(at.sum_row(g), lp.s1_out_first(g, fix_parts));
  }
  // ---- fused: the group MSM tasks of fused_plan(B) and ONE fixed-base task over sums row 0 (launch_check_fused) ----
  static LocatePlan fused_plan(size_t B) { return locate_plan(B, kLocateGroupsMax); }
  void fused_tasks(MsmTask* mt, FixTask* ft) const {
    group_msm_tasks(fused_plan(B), mt);
    *ft = crs_task(at.sum_row(0), 0);
  }
  // ---- the suspects list[0 .. S), stage 2 of the grouped check: S dense tasks (launch_check) over the scalars stage 1 left in place ----
  void suspect_tasks(const std::vector<uint32_t>& list, size_t fix_parts, MsmTask* mt, FixTask* ft) const {
    for (size_t s = 0; s < list.size(); s++) {
      const size_t p = list[s];
      mt[s] = range_task(p * NPT, NPT, LocatePlan::s2_conv_off(s, NPT));
      ft[s] = crs_task(at.crs_of(p), LocatePlan::s2_out_first(s, fix_parts));
    }
  }

 private:
  // the points [first, first + count) of the batch through the global gather list
  MsmTask range_task(size_t first, size_t count, size_t conv_off) const {
    return MsmTask{points, gidx + first, at.pts + first, (uint32_t)count, 0, (uint32_t)conv_off};
  }
  void group_msm_tasks(const LocatePlan& lp, MsmTask* mt) const {
    for (size_t g = 0; g < lp.NT; g++) mt[g] = range_task(lp.s1_task_off(g, NPT), lp.s1_task_n(g, NPT), lp.s1_task_off(g, NPT));
  }
  FixTask crs_task(const Fr* scalars, size_t out_first) const { return FixTask{nullptr, scalars, 0, (uint32_t)n, 0, (uint32_t)out_first}; }
};

// The per-proof mode's verdict from a proof's flag word and whether its sum is the identity: decode > structural > check
// (locate_verdicts is the grouped mode's form of the same rule).
inline int check_verdict(uint32_t flag_word, bool passed) {
  return (flag_word & kLocateFlagDecode) ? CPX_ERR_DESERIALIZE : ((flag_word & kLocateFlagStruct) || !passed) ? CPX_ERR_VERIFY : CPX_OK;
}

}  // namespace cpx
