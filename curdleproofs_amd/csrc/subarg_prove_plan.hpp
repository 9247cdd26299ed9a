// Planner of the stand-alone sub-argument provers (cpx_ipa_prove, cpx_same_msm_prove; the core layer of Engine::subarg_prove,
// engine_subarg.cpp) — host code without a HIP call.
// InnerProductProof::new (inner_product_argument.rs:98-199) and SameMultiscalarProof::new (same_multiscalar_argument.rs:69-150) for `count`
// independent items are the steps before the log-round loop — blinders, the B points, step 1 of the transcript, the rewrite of the
// vectors by alpha, for the IPA H = beta crs_H — followed by the loop of loop_plan.hpp on the same device memory.  This header says where
// the steps before the loop keep their values BEHIND the loop's own regions (LoopPlan lp: the item rows of bases, the Fr memory, the
// results), and how the proof bytes are put together from what comes down.  One definition for Engine::subarg_prove, the kernels of
// subarg_prove.hip and tests/host_emul/subarg_prove_plan_emul.cpp, which compiles it for the CPU (tests/test_subarg_prove_cpu.py).
//
//   Fr memory      the loop's regions | witness, per item c | d resp. x | draws, per item r [n] | z [n - 2] resp. r [n] | IPA: r_d, per
//                  item n (the z draws with the two solved entries behind them) | IPA: z, one per item | alpha (, beta), per item
//   Jacobian       B points, item-major B_c B_d resp. B_a B_t B_u | statement points, item-major crs_H C D resp. A Z_t Z_u
//   bytes          the loop's round encodings | the encodings of those points in the same order | SameMSM: T | U per item | rng states
//   affine         the loop's round results | the normalised forms of those points in the same order (the IPA reads crs_H there)
//   MSM tasks      the loop's L rounds of tasks | the B tasks: item-major, n points each
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "mont32.hpp"
#include "loop_plan.hpp"

namespace cpx {

struct SubargProvePlan {
  LoopPlan lp;        // host side; the accessors below (which the kernels call too) read the copies subarg_prove_plan() takes of it
  bool ipa_ = true;
  size_t count_ = 0, n_ = 0, L_ = 0, loop_fr_ = 0, loop_results_ = 0;   // lp.fr_total(), lp.results()

  CPX_HD bool ipa() const { return ipa_; }
  CPX_HD size_t count() const { return count_; }
  CPX_HD size_t n() const { return n_; }
  CPX_HD size_t L() const { return L_; }
  static constexpr size_t kStatement = 3;                                          // crs_H C D resp. A Z_t Z_u
  CPX_HD size_t first() const { return ipa() ? 2 : 3; }                            // B_c B_d resp. B_a B_t B_u
  CPX_HD size_t nvec() const { return ipa() ? 2 : 1; }
  CPX_HD size_t draws_each() const { return ipa() ? 2 * n() - 2 : n(); }           // inner_product_argument.rs:46-47, same_multiscalar_argument.rs:78
  CPX_HD size_t ab_each() const { return ipa() ? 2 : 1; }                          // alpha, beta resp. alpha
  CPX_HD size_t challenges() const { return ab_each() + L(); }
  // ---- Fr memory behind the loop's ----
  CPX_HD size_t fr_wit() const { return loop_fr_; }
  CPX_HD size_t fr_draws() const { return fr_wit() + count() * nvec() * n(); }
  CPX_HD size_t fr_rd() const { return fr_draws() + count() * draws_each(); }
  CPX_HD size_t fr_z() const { return fr_rd() + (ipa() ? count() * n() : 0); }
  CPX_HD size_t fr_ab() const { return fr_z() + (ipa() ? count() : 0); }
  CPX_HD size_t fr_total() const { return fr_ab() + count() * ab_each(); }
  // ---- points: B then statement; the same index among the Jacobian inputs, and behind the loop's results among the affine forms and the encodings ----
  CPX_HD size_t pt_first(size_t item, size_t b) const { return item * first() + b; }
  CPX_HD size_t pt_statement(size_t item, size_t k) const { return count() * first() + item * kStatement + k; }
  CPX_HD size_t points() const { return count() * (first() + kStatement); }
  CPX_HD size_t aff_points() const { return loop_results_; }
  CPX_HD size_t aff_total() const { return aff_points() + points(); }
  // ---- bytes ----
  CPX_HD size_t by_points() const { return loop_results_ * 48; }
  CPX_HD size_t by_tu() const { return by_points() + points() * 48; }
  CPX_HD size_t by_rng() const { return by_tu() + (ipa() ? 0 : count() * 2 * n() * 48); }
  CPX_HD size_t by_total() const { return by_rng() + count() * 40; }
  // ---- the proof bytes (inner_product_argument.rs:328-338, same_multiscalar_argument.rs:263-275): the B points, then one block of L
  // points per name — grouped by name over the rounds, not by round as the transcript takes them —, then the finals ----
  CPX_HD size_t blocks() const { return ipa() ? 4 : 6; }
  CPX_HD int block_term(size_t b) const {                                          // which cross term of a round (transcript order) block b holds:
    return ipa() ? (int)(((b & 1) << 1) | (b >> 1)) : (int)b;                      // bytes L_C R_C L_D R_D, a round L_C L_D R_C R_D; SameMSM the same both ways
  }
  CPX_HD size_t proof_points() const { return first() + blocks() * L(); }
  CPX_HD size_t proof_bytes() const { return 48 * proof_points() + 32 * nvec(); }
  CPX_HD size_t point_byte(size_t slot) const { return 48 * slot; }
  CPX_HD size_t round_slot(size_t j, size_t b) const { return first() + b * L() + j; }
  CPX_HD size_t scalar_byte(size_t i) const { return 48 * proof_points() + 32 * i; }
  // ---- MSM tasks ----
  CPX_HD size_t task_first() const { return L() * count() * blocks(); }
  CPX_HD size_t task_total() const { return task_first() + count() * first(); }
  CPX_HD int first_family(size_t b) const { return (int)b; }                       // B_c: G, B_d: G'; B_a: G, B_t: T, B_u: U
  bool first_msm(Tier0MsmPlan& pl, std::vector<uint32_t>& lens) const {
    lens.assign(count() * first(), (uint32_t)n());
    return tier0_msm_plan(lens.size(), lens.data(), pl);
  }
  SubargTotals totals() const { return {fr_total(), points(), aff_total(), by_total(), count(), lp.idx_total(), task_total(), lp.results(), 0, 0}; }   // flags: one per item
};

// Same limits and verdicts as the loop's plan: a prover call is one loop call with a B-point MSM of count * first() tasks of n points
// ahead, which stays below what a round takes (2 count n < count (2 n + 2), 3 count n).
inline LoopPlanStatus subarg_prove_plan(bool ipa, size_t count, size_t n, SubargProvePlan& sp) {
  const LoopPlanStatus st = loop_plan(ipa, count, n, sp.lp);
  if (st != LOOP_OK) return st;
  sp.ipa_ = ipa;
  sp.count_ = count;
  sp.n_ = n;
  sp.L_ = sp.lp.L;
  sp.loop_fr_ = sp.lp.fr_total();
  sp.loop_results_ = sp.lp.results();
  return LOOP_OK;
}

}  // namespace cpx
