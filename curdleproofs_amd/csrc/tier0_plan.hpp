// Planner of the per-round tier-0 calls (cpx_g1_msm_many, cpx_g1_fold_many) — host code without a HIP call: where every task of a
// call of `count` ragged MSMs lives in the scratch of the endomorphism bucket-list path (k_to_table_endo + k_msm_tblw<2, true> +
// k_reduce_sets + k_msm_tail, kernels.h), how much of each scratch the call needs, and which form of the scalar multiplication a fold
// call takes.  One definition for Engine::msm_many / Engine::fold_many and for tests/host_emul/tier0_plan_emul.cpp, which compiles it
// for the CPU (tests/test_tier0_rounds_cpu.py).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace cpx {

constexpr size_t kTier0ManyTasks = (size_t)1 << 16;    // MSMs per cpx_g1_msm_many (the second grid dimension of k_to_table_endo)
constexpr size_t kTier0ManyPoints = (size_t)1 << 24;   // points per cpx_g1_msm_many, elements per cpx_g1_fold_many (int grids, 32-bit offsets)

// Waves per window of a task over its points (kernels.h msm_tblw_slices; `pinned` = option tbw_slices): only for the two-window waves,
// only when the GPU would otherwise stand almost empty (16 waves per task, 1024 SIMDs) and a slice keeps >= 256 points — below that the
// longest of a wave's 128 bucket lists no longer shrinks with the slice, while every slice costs two more sets to reduce.
inline int tbw_slices_rule(long pinned, int ntasks, int wpw, int max_n) {
  if (pinned) return (int)pinned;   // 1|2|4 pins it
  if (wpw != 2) return 1;
  const long waves = (long)ntasks * 16;
  int s = waves * 4 <= 1024 ? 4 : waves * 2 <= 1024 ? 2 : 1;
  while (s > 1 && max_n / s < 256) s >>= 1;
  return s;
}

// `count` MSMs of lens[i] points, bases and scalars task after task.  Task i's points sit at offset conv_off[i] (in points) of the
// uploaded bases and scalars; the kernels address everything else from that offset and from the task's index:
//   table-form bases   conv[2 conv_off[i] .. + 2 lens[i])      P then -phi(P)                     (TAff entries)
//   digits             dig[9 conv_off[i] .. + 9 lens[i])       9 words per point                  (32-bit words)
//   raw sets, partials 32 slices per task from 32 slices * i;  part[(16 i + w) * 2 slices + d] carries the weight 2^(8 w)
// A task of no points owns empty ranges of the first two and still its 32 slices sets: its waves sort an empty range and leave
// identity accumulators (msm_body.hpp: tbw_sort reads no point when next == ntot, every bucket is parked as the identity — what a
// slice beyond the end of a short task does in every launch with slices > 1), so its result is the identity.
struct Tier0MsmPlan {
  size_t count = 0, points = 0;
  uint32_t max_n = 0;
  int slices = 1;
  std::vector<uint32_t> conv_off;   // per task, in points
  size_t conv_entries() const { return 2 * points; }
  size_t digit_words() const { return 9 * points; }
  size_t sets() const { return count * 32 * (size_t)slices; }   // raw sets = partial sums
  int tail_dup() const { return 2 * slices; }                   // consecutive partial sums of one weight (launch_msm_tail)
  size_t conv_first(size_t i) const { return 2 * (size_t)conv_off[i]; }
  size_t digit_first(size_t i) const { return 9 * (size_t)conv_off[i]; }
  size_t part_first(size_t i) const { return i * 32 * (size_t)slices; }
  size_t part_slot(size_t i, int w, int d) const { return (i * 16 + (size_t)w) * 2 * (size_t)slices + (size_t)d; }
};
// false: more tasks or points than a call takes (count is looked at before lens is read)
inline bool tier0_msm_plan(size_t count, const uint32_t* lens, Tier0MsmPlan& pl) {
  if (count > kTier0ManyTasks) return false;
  pl.count = count;
  pl.points = 0;
  pl.max_n = 0;
  pl.conv_off.assign(count, 0);
  for (size_t i = 0; i < count; i++) {
    pl.conv_off[i] = (uint32_t)pl.points;
    pl.points += lens[i];
    if (pl.points > kTier0ManyPoints) return false;
    if (lens[i] > pl.max_n) pl.max_n = lens[i];
  }
  return true;
}

// cpx_g1_fold_many: family f's elements are [f half, (f + 1) half) of PL / PR, its gamma is scalar f.  false: too many elements
inline bool tier0_fold_fits(size_t families, size_t half) { return !families || half <= kTier0ManyPoints / families; }
// the quad_max a fold call of `total` elements hands to launch_smul: > 0 = a quad per element (k_smul_quad), 0 = the one-lane k_smul —
// above option fold_quad_max, at 0, and always for the plain double-and-add (scale_any_point: SMUL_PLAIN tasks never take the quad form)
inline long tier0_fold_quad_max(size_t total, long fold_quad_max, bool plain) {
  return !plain && fold_quad_max > 0 && total <= (size_t)fold_quad_max ? fold_quad_max : 0;
}

// What a sub-argument call needs of every kind of tier-0 scratch, and what leads the inner proof in its outputs.  Every plan of the stack
// (subarg_prove_plan.hpp / subarg_check_plan.hpp -> gprod_plan.hpp -> same_perm_plan.hpp) answers with its totals(): the end of the last
// region of each kind at its depth, a layer taking the totals of the plan it wraps and moving those ends it lies behind.  The engine asks
// the outermost plan in use (engine_subarg.cpp).
struct SubargTotals {
  size_t fr, jac, aff, bytes, flags, ix, tasks, res;   // elements of Fr memory, Jacobian inputs, affine points, bytes, flag / status bytes, index words, MSM tasks, MSM sums
  size_t lead_bytes, lead_challenges;                  // ahead of the inner-product / same-multiscalar proof's bytes resp. challenges, per item
};

}  // namespace cpx
