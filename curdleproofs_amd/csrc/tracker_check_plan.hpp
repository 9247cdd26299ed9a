// Plan and scalar rules of the grouped / fused check of Whisk tracker proofs (cpx_whisk_verify_tracker_proofs_grouped / _fused, include/cpx.h)
// — host + device code without a HIP call: which MSM task every group of items is, where every base and scalar of an item sits in it, how
// much of each scratch the call needs, and the five scalars plus the generator term of one item.  One definition for k_tracker_check_scalars
// (tracker.hip), Engine::tracker_check (whisk.cpp) and tests/host_emul/tracker_check_emul.cpp, which compiles it for the CPU
// (tests/test_tracker_grouped_cpu.py).
//
// The two relations of whisk.rs:219-223, weighted by the caller's factors a, b and summed:
//   a (s G + c k_G - A) + b (s r_G + c k_r_G - B)
// Over a group of items that is ONE MSM: the generator with the scalar  sum a_i s_i,  and per item the five points
//   k_G  a c      A  -a      r_G  b s      k_r_G  b c      B  -b
// The sum is linear in the independent factors, so a group that contains a false relation sums to the identity with probability <= 1 / r.
//
// Grouping is locate_plan.hpp's, with the decode flag only.  Group g is task g: 1 + 5 group_count(g) points, the generator first, then the
// items in batch order, five points each in the order above; the tasks lie one behind the other (Tier0MsmPlan's conv_off).
// Identity points: k_to_table_endo has no test here that shows 96 zero bytes to be a base that contributes nothing, so an identity point
// (k = 0: k_G and k_r_G; blinder = 0: A and B) is replaced by the generator with the scalar 0, as are the five terms of a flagged item.
#pragma once
#include <cstddef>
#include <cstdint>
#include "locate_plan.hpp"
#include "mont32.hpp"

namespace cpx {

constexpr size_t kTrackerCheckMax = (size_t)1 << 21;   // items per call: 5 count + 256 points stay within kTier0ManyPoints = 2^24
constexpr int TCK_TERMS = 5;
enum : int { TCK_K_G = 0, TCK_A = 1, TCK_R_G = 2, TCK_K_R_G = 3, TCK_B = 4 };
// the plane of k_decompress's output that holds term j (the batched verifier decodes A, B, k_r_G, r_G, k_G plane-major: whisk.cpp)
CPX_HD int tck_plane(int j) { return j == TCK_K_G ? 4 : j == TCK_A ? 0 : j == TCK_R_G ? 3 : j == TCK_K_R_G ? 2 : 1; }

// The inputs of `count` items as both batched verifiers upload them: trackers (96 B each) | k_commitments (48 B) | proofs (128 B), and where
// the decoder reads the five points of item i from: plane_off[pl] + plane_rec[pl] * i, planes A, B (inside the proof), k_r_G, r_G (inside
// the tracker), k_G — the order tck_plane() names.
constexpr int TCK_PLANES = 5;
struct TrackerInputLayout {
  size_t trackers, k_commitments, proofs, bytes;   // the three arrays' offsets and the size of the whole
  size_t plane_off[TCK_PLANES], plane_rec[TCK_PLANES];
};
inline TrackerInputLayout tracker_input_layout(size_t count) {
  const size_t kc = 96 * count, prf = 144 * count;
  return TrackerInputLayout{0, kc, prf, 272 * count, {prf, prf + 48, 48, 0, kc}, {128, 128, 96, 96, 48}};
}

struct TrackerCheckPlan {
  LocatePlan lp;
  size_t count() const { return lp.B; }
  size_t tasks() const { return lp.NT; }
  // ---- task g of the stage-1 MSM ----
  size_t task_off(size_t g) const { return g + TCK_TERMS * lp.group_first(g); }       // its first point = its conv_off: the generator
  size_t task_n(size_t g) const { return 1 + TCK_TERMS * lp.group_count(g); }
  size_t max_n() const { return lp.B ? 1 + TCK_TERMS * lp.G : 0; }                   // points of the largest task
  size_t points() const { return lp.NT + TCK_TERMS * lp.B; }                         // bases = scalars of all tasks
  size_t gen_slot(size_t g) const { return task_off(g); }
  size_t slot(size_t p, int j) const {                                               // term j of item p
    const size_t g = lp.group_of(p);
    return task_off(g) + 1 + TCK_TERMS * (p - lp.group_first(g)) + (size_t)j;
  }
  // ---- scratch of a call (beside the tier-0 MSM scratch for tasks() tasks of points() points: tier0_plan.hpp) ----
  size_t input_bytes() const { return tracker_input_layout(lp.B).bytes; }
  size_t weight_scalars() const { return 2 * lp.B; }   // a_i, b_i
  size_t result_points() const { return lp.NT; }       // the group sums, Jacobian standard form
  // stage 2: S suspects, dense — five decoded planes of S points, S proofs, S challenges, S clear flags, S verdicts
  static size_t s2_points(size_t S) { return TCK_TERMS * S; }
  static size_t s2_proof_bytes(size_t S) { return 128 * S; }
};
inline bool tracker_check_fits(size_t count) { return count <= kTrackerCheckMax; }
inline TrackerCheckPlan tracker_check_plan(size_t count, long groups_max) {
  TrackerCheckPlan pl;
  pl.lp = locate_plan(count, groups_max);
  return pl;
}

// The scalars of one item, all in Montgomery form (a, b: the weights; s: the proof's response; c: the challenge).
struct TrackerCheckScalars {
  Fr term[TCK_TERMS];   // of k_G, A, r_G, k_r_G, B
  Fr gen;               // the item's share of its group's generator scalar
};
CPX_HD TrackerCheckScalars tracker_check_scalars(const Fr& a, const Fr& b, const Fr& s, const Fr& c) {
  TrackerCheckScalars o;
  o.term[TCK_K_G] = fe_mul(a, c);
  o.term[TCK_A] = fe_neg(a);
  o.term[TCK_R_G] = fe_mul(b, s);
  o.term[TCK_K_R_G] = fe_mul(b, c);
  o.term[TCK_B] = fe_neg(b);
  o.gen = fe_mul(a, s);
  return o;
}

}  // namespace cpx
