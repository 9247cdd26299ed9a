// Planner of the stand-alone grand-product prover (cpx_gprod_prove; the grand-product layer of Engine::subarg_prove, engine_subarg.cpp) — host code without a HIP call.
// GrandProductProof::new (grand_product_argument.rs:43-166) for `count` independent items of ell factors and n_blinders blinders,
// n = ell + n_blinders = 2^L, is the grand-product layer — prefix products, C, r_p, the two challenges, vec_d, D — followed by
// InnerProductProof::new on G | H, G' = u o (G | H), crs_U, C, D, inner_prod and c = vec_c | vec_c_blinders, d = vec_d | vec_d_blinders.
// This header says where that layer keeps its values BEHIND the regions of the IPA prover (SubargProvePlan sp, which keeps its own behind
// the loop's), the same way that plan builds on LoopPlan, and how the proof bytes are put together.  One definition for the engine, the
// kernels of gprod.hip and tests/host_emul/gprod_plan_emul.cpp, which compiles it for the CPU (tests/test_gprod_cpu.py).
//
//   bases          the item's row of the loop: family 0 = G | H, family 1 = the same points again (no G' is formed: u seeds the loop's
//                  fold coefficients of family 1 and multiplies r_d for B_d)
//   Fr memory      the IPA prover's regions (its witness c | d is where vec_c | vec_c_blinders and vec_d | vec_d_blinders are written, its
//                  z slot takes inner_prod) | gprod_result, one per item | vec_b, ell per item | vec_b_blinders | vec_c_blinders (the first
//                  n_blinders draws) | u, n per item | D's scalars, n per item | r_d o u, n per item | r_p | alpha, beta per item
//                  (the powers of beta are never stored: every thread starts its chunk from beta^lo)
//   Jacobian       the IPA prover's points | B, one per item.  The sums of the C and D tasks land in the loop's result memory, which no
//                  round has used yet: C at item, D at count + item; they are copied into the IPA's statement slots
//   affine, bytes  the IPA prover's | the normalised B per item (what k_finalize adds to the D task's sum)  resp.  the encodings of B, then
//                  of C, per item (what steps 1 and 2 of the transcript absorb)
//   flags          the IPA prover's [count] (generate_ipa_blinders panics) | [count] beta = 0 (:86)
//   index words    the loop's lists | k_finalize's addend list over the IPA prover's points: B's affine slot at the item's D, ~0 elsewhere
//   MSM tasks      the IPA prover's | the C tasks | the D tasks: one per item, n points each
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "subarg_check_plan.hpp"
#include "subarg_prove_plan.hpp"

namespace cpx {

struct GprodProvePlan {
  SubargProvePlan sp;   // the inner-product prover on n elements: every region below starts where one of its totals ends
  size_t count_ = 0, ell_ = 0, nb_ = 0, n_ = 0;

  CPX_HD size_t count() const { return count_; }
  CPX_HD size_t ell() const { return ell_; }
  CPX_HD size_t nb() const { return nb_; }
  CPX_HD size_t n() const { return n_; }
  CPX_HD size_t draws_each() const { return nb() + sp.draws_each(); }                     // vec_c_blinders (:75), then generate_ipa_blinders' r [n] | z [n - 2]
  CPX_HD size_t challenges() const { return 2 + sp.challenges(); }                         // gprod alpha, beta, then the IPA's
  // ---- Fr memory behind the IPA prover's ----
  CPX_HD size_t fr_result() const { return sp.fr_total(); }
  CPX_HD size_t fr_b() const { return fr_result() + count(); }
  CPX_HD size_t fr_rb() const { return fr_b() + count() * ell(); }
  CPX_HD size_t fr_cbl() const { return fr_rb() + count() * nb(); }
  CPX_HD size_t fr_u() const { return fr_cbl() + count() * nb(); }
  CPX_HD size_t fr_dsc() const { return fr_u() + count() * n(); }
  CPX_HD size_t fr_rdu() const { return fr_dsc() + count() * n(); }
  CPX_HD size_t fr_rp() const { return fr_rdu() + count() * n(); }
  CPX_HD size_t fr_chal() const { return fr_rp() + count(); }
  CPX_HD size_t fr_total() const { return fr_chal() + 2 * count(); }
  // ---- points ----
  CPX_HD size_t pt_B(size_t item) const { return sp.points() + item; }               // among the Jacobian inputs and, behind aff_points(), the affine forms
  CPX_HD size_t jac_total() const { return sp.points() + count(); }
  CPX_HD size_t aff_total() const { return sp.aff_total() + count(); }
  CPX_HD size_t res_C(size_t item) const { return item; }
  CPX_HD size_t res_D(size_t item) const { return count() + item; }
  CPX_HD size_t res_total() const { return 2 * count(); }
  // ---- bytes ----
  CPX_HD size_t by_B() const { return sp.by_total(); }
  CPX_HD size_t by_C() const { return by_B() + count() * 48; }
  CPX_HD size_t by_total() const { return by_C() + count() * 48; }
  // ---- flags, index words, MSM tasks ----
  CPX_HD size_t flag_beta() const { return count(); }
  CPX_HD size_t flags_total() const { return 2 * count(); }
  size_t ix_addend() const { return sp.lp.idx_total(); }                            // (host: the engine alone reads the lists' places)
  size_t ix_total() const { return ix_addend() + sp.points(); }
  CPX_HD size_t task_C() const { return sp.task_total(); }
  CPX_HD size_t task_D() const { return task_C() + count(); }
  CPX_HD size_t task_total() const { return task_D() + count(); }
  // ---- the proof bytes (:248-253): C, r_p, then the InnerProductProof's ----
  CPX_HD size_t byte_C() const { return 0; }
  CPX_HD size_t byte_rp() const { return 48; }
  CPX_HD size_t byte_ipa() const { return 80; }
  CPX_HD size_t proof_bytes() const { return byte_ipa() + sp.proof_bytes(); }
  void fill_addend(std::vector<uint32_t>& ix) const {
    ix.assign(sp.points(), ~0u);
    for (size_t i = 0; i < count(); i++) ix[sp.pt_statement(i, 2)] = (uint32_t)pt_B(i);
  }
  bool item_msm(Tier0MsmPlan& pl, std::vector<uint32_t>& lens) const {               // the C tasks, and the D tasks again
    lens.assign(count(), (uint32_t)n());
    return tier0_msm_plan(lens.size(), lens.data(), pl);
  }
  SubargTotals totals() const {                                                      // (C and D land in the loop's result memory: the larger of the two)
    const size_t res = sp.lp.results() > res_total() ? sp.lp.results() : res_total();
    return {fr_total(), jac_total(), aff_total(), by_total(), flags_total(), ix_total(), task_total(), res, byte_ipa(), 2};
  }
};

enum GprodPlanStatus { GPROD_OK = 0, GPROD_NOT_POW2 = 1, GPROD_TOO_LARGE = 2, GPROD_NO_FACTOR = 3, GPROD_NO_BLINDERS = 4 };

// ell = 0: the reference's `ell - 1` underflows (:71); n = 1: the IPA's n - 2 does (inner_product_argument.rs:47).  The limits are those
// of the IPA prover on n elements, that is of one cpx_ipa_rounds: the C and D tasks (count n points each) stay below a round's.
inline GprodPlanStatus gprod_prove_plan(size_t count, size_t ell, size_t n_blinders, GprodProvePlan& gp) {
  if (!ell) return GPROD_NO_FACTOR;
  const size_t n = ell + n_blinders;
  if (n < ell) return GPROD_TOO_LARGE;
  switch (subarg_prove_plan(true, count, n, gp.sp)) {
    case LOOP_NOT_POW2: return GPROD_NOT_POW2;
    case LOOP_TOO_LARGE: return GPROD_TOO_LARGE;
    default: break;
  }
  if (n == 1) return GPROD_NO_BLINDERS;
  gp.count_ = count;
  gp.ell_ = ell;
  gp.nb_ = n_blinders;
  gp.n_ = n;
  return GPROD_OK;
}

// The stand-alone grand-product verifier (cpx_gprod_verify; the grand-product layer of Engine::subarg_verify, engine_subarg.cpp): GrandProductProof::verify
// (grand_product_argument.rs:180-246) is the inner-product check of subarg_check_plan.hpp on G | H, crs_U, the proof's C and
// D = B - beta^-1 crs_G_sum + alpha crs_H_sum, whose row, weights and regions are used as they are; what the steps ahead of it need lies
// BEHIND its regions:
//   bytes          the check's | heads: C, r_p of every proof [count][80] | the encodings of B [count][48] | of D [count][48]
//   status bytes   the check's (decoder verdicts [count][proof_points], flags [count]) | the decoder's verdict of C [count] | flags of C / r_p [count]
//   Fr memory      the check's (z takes inner_prod, vec_u takes u) | gprod_result | -beta^-1 | alpha, one per item each | alpha, beta per item
//   index words    the check's | C's byte offsets among the heads | C's row slots | crs_U's row slots, [count] each
//   affine, dense  B | crs_G_sum | crs_H_sum | B - beta^-1 crs_G_sum | D, [count] each
struct GprodCheckPlan {
  SubargCheckPlan sp;   // the inner-product check on n elements
  size_t ell = 0, nb = 0;

  CPX_HD size_t count() const { return sp.count; }
  static constexpr size_t kHead = 80;                                                // C (48), r_p (32) ahead of the InnerProductProof's bytes (:248-253)
  CPX_HD size_t proof_bytes() const { return kHead + sp.proof_bytes(); }
  CPX_HD size_t rp_byte() const { return 48; }
  CPX_HD size_t challenges() const { return 2 + sp.challenges(); }
  // ---- bytes ----
  CPX_HD size_t by_heads() const { return (sp.by_total() + 15) / 16 * 16; }
  CPX_HD size_t by_B() const { return by_heads() + count() * kHead; }
  CPX_HD size_t by_D() const { return by_B() + count() * 48; }
  CPX_HD size_t by_total() const { return by_D() + count() * 48; }
  // ---- status bytes ----
  CPX_HD size_t st_C() const { return sp.st_total(); }
  CPX_HD size_t st_bad() const { return st_C() + count(); }
  CPX_HD size_t st_total() const { return st_bad() + count(); }
  // ---- Fr memory ----
  CPX_HD size_t fr_result() const { return sp.fr_total(); }
  CPX_HD size_t fr_neg_beta_inv() const { return fr_result() + count(); }
  CPX_HD size_t fr_alpha() const { return fr_neg_beta_inv() + count(); }
  CPX_HD size_t fr_chal() const { return fr_alpha() + count(); }
  CPX_HD size_t fr_total() const { return fr_chal() + 2 * count(); }
  // ---- index words ----
  CPX_HD size_t ix_C_src() const { return sp.ix_total(); }
  CPX_HD size_t ix_C_dst() const { return ix_C_src() + count(); }
  CPX_HD size_t ix_U_dst() const { return ix_C_dst() + count(); }
  CPX_HD size_t ix_total() const { return ix_U_dst() + count(); }
  void fill_idx(std::vector<uint32_t>& ix) const {                                   // the three lists, relative to ix_C_src()
    ix.resize(3 * count());
    for (size_t i = 0; i < count(); i++) {
      ix[i] = (uint32_t)(i * kHead);
      ix[count() + i] = (uint32_t)(i * sp.points() + sp.statement_off() + 1);
      ix[2 * count() + i] = (uint32_t)(i * sp.points() + sp.statement_off());
    }
  }
  // ---- affine points, dense ----
  CPX_HD size_t aff_B() const { return 0; }
  CPX_HD size_t aff_g_sum() const { return count(); }
  CPX_HD size_t aff_h_sum() const { return 2 * count(); }
  CPX_HD size_t aff_partial() const { return 3 * count(); }
  CPX_HD size_t aff_D() const { return 4 * count(); }
  CPX_HD size_t aff_total() const { return 5 * count(); }
  SubargTotals totals() const {                                                      // (crs_U and B lie within the check's Jacobian inputs)
    const SubargTotals t = sp.totals();
    return {fr_total(), t.jac, aff_total(), by_total(), st_total(), ix_total(), t.tasks, t.res, kHead, 2};
  }
};

// ell = 0 is refused (no prover can make such a proof); n = 1 is a real check.  The limits are those of the inner-product check.
inline SubargPlanStatus gprod_check_plan(size_t count, size_t ell, size_t n_blinders, GprodCheckPlan& gp) {
  gp.ell = ell;
  gp.nb = n_blinders;
  return subarg_check_plan(true, count, ell + n_blinders, gp.sp);
}

}  // namespace cpx
