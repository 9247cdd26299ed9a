// Planner of the stand-alone same-permutation prover and verifier (cpx_same_perm_prove, cpx_same_perm_verify; the same-permutation layer of
// Engine::subarg_prove and Engine::subarg_verify, engine_subarg.cpp) — host and device code without a HIP call.  SamePermutationProof::new
// (same_permutation_argument.rs:40-99) is step 1 of the transcript, the permuted factors, their product, vec_b_blinders and
// B = A + alpha M + beta sum G, then GrandProductProof::new on B, the product, the factors and vec_b_blinders; ::verify (:112-171) is step
// 1, the index factors and their product, one accumulate_check (:149) and GrandProductProof::verify.  This header says where that layer
// keeps its values BEHIND the regions of the grand-product plans (gprod_plan.hpp), the same way those build on the inner-product ones, and
// how the verifier's row and weights are extended.  One definition for the engine, the kernels of same_perm.hip and
// tests/host_emul/same_perm_plan_emul.cpp, which compiles it for the CPU (tests/test_same_perm_cpu.py).
//
// Prover, behind GprodProvePlan gp (whose gprod_result, vec_b, vec_b_blinders and B are written on the device instead of uploaded):
//   Fr memory      gp's | vec_a, ell per item | vec_a_blinders | vec_m_blinders, n_blinders per item each | B's scalars, ell + 1 per item
//                  (beta on the positions of G, alpha on M) | alpha, beta per item
//   index words    gp's | the permutation, ell per item | the gather list of the B tasks, ell + 1 words shared by all items: G_0..G_{ell-1}
//                  of the item's row, then the row's H slot, which holds the normalised M until the inner-product prover writes beta crs_U
//                  there | k_finalize's addend list over the B sums: A's affine slot
//   Jacobian       gp's | A | M, one per item each.  The sums of the B tasks land in gp's B slots.
//   affine         gp's | A | M normalised
//   bytes          gp's | the encodings of A | of M, per item (what step 1 absorbs)
//   MSM tasks      gp's | the B tasks: one per item, ell + 1 points
//   proof bytes    B compressed, then the grand-product proof (:173-177)
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "gprod_plan.hpp"

namespace cpx {

constexpr int SAME_PERM_PIECE = 128;   // scalars of vec_a converted and absorbed at a time: 4 KiB of LDS whatever ell is

struct SamePermProvePlan {
  GprodProvePlan gp;

  CPX_HD size_t count() const { return gp.count(); }
  CPX_HD size_t ell() const { return gp.ell(); }
  CPX_HD size_t nb() const { return gp.nb(); }
  CPX_HD size_t draws_each() const { return gp.draws_each(); }          // the layer draws nothing
  CPX_HD size_t challenges() const { return 2 + gp.challenges(); }      // same-perm alpha, beta, then the grand product's
  CPX_HD size_t message_bytes() const { return 8 + 32 * ell(); }        // vec_a as a Vec<Fr>: the u64 length, then the scalars
  // ---- Fr memory ----
  CPX_HD size_t fr_a() const { return gp.fr_total(); }
  CPX_HD size_t fr_ra() const { return fr_a() + count() * ell(); }
  CPX_HD size_t fr_rm() const { return fr_ra() + count() * nb(); }
  CPX_HD size_t fr_bsc() const { return fr_rm() + count() * nb(); }
  CPX_HD size_t fr_chal() const { return fr_bsc() + count() * (ell() + 1); }
  CPX_HD size_t fr_total() const { return fr_chal() + 2 * count(); }
  // ---- index words ----
  size_t ix_perm() const { return gp.ix_total(); }
  size_t ix_gather() const { return ix_perm() + count() * ell(); }
  size_t ix_addend() const { return ix_gather() + ell() + 1; }
  size_t ix_total() const { return ix_addend() + count(); }
  // ---- points ----
  CPX_HD size_t jac_A() const { return gp.jac_total(); }
  CPX_HD size_t jac_M() const { return jac_A() + count(); }
  CPX_HD size_t jac_total() const { return jac_M() + count(); }
  CPX_HD size_t aff_A() const { return gp.aff_total(); }
  CPX_HD size_t aff_M() const { return aff_A() + count(); }
  CPX_HD size_t aff_total() const { return aff_M() + count(); }
  CPX_HD size_t aff_B() const { return gp.sp.aff_points() + gp.pt_B(0); }   // where the grand-product layer keeps the normalised B
  // ---- bytes ----
  CPX_HD size_t by_A() const { return gp.by_total(); }
  CPX_HD size_t by_M() const { return by_A() + count() * 48; }
  CPX_HD size_t by_total() const { return by_M() + count() * 48; }
  // ---- MSM tasks ----
  CPX_HD size_t task_B() const { return gp.task_total(); }
  CPX_HD size_t task_total() const { return task_B() + count(); }
  // ---- the proof bytes (:173-177) ----
  CPX_HD size_t byte_B() const { return 0; }
  CPX_HD size_t byte_gprod() const { return 48; }
  CPX_HD size_t proof_bytes() const { return byte_gprod() + gp.proof_bytes(); }
  // the gather list (relative to the item's row) and the addend list (relative to aff_B())
  void fill_lists(std::vector<uint32_t>& gather, std::vector<uint32_t>& addend) const {
    gather.resize(ell() + 1);
    for (size_t i = 0; i < ell(); i++) gather[i] = (uint32_t)(gp.sp.lp.family_off(0) + i);
    gather[ell()] = (uint32_t)gp.sp.lp.h_index();
    addend.resize(count());
    for (size_t i = 0; i < count(); i++) addend[i] = (uint32_t)(aff_A() + i - aff_B());
  }
  bool item_msm(Tier0MsmPlan& pl, std::vector<uint32_t>& lens) const {   // the B tasks
    lens.assign(count(), (uint32_t)(ell() + 1));
    return tier0_msm_plan(lens.size(), lens.data(), pl);
  }
  SubargTotals totals() const {                                          // (the B sums land in gp's B slots, the layer raises no flag)
    const SubargTotals t = gp.totals();
    return {fr_total(), jac_total(), aff_total(), by_total(), t.flags, ix_total(), task_total(), t.res, byte_gprod() + t.lead_bytes, 2 + t.lead_challenges};
  }
};

// the argument rules are those of the grand-product prover
inline GprodPlanStatus same_perm_prove_plan(size_t count, size_t ell, size_t n_blinders, SamePermProvePlan& pl) { return gprod_prove_plan(count, ell, n_blinders, pl.gp); }

// Verifier, behind GprodCheckPlan gp.  The extra relation  beta <1, G> - (B - A - alpha M) == O  (:149) joins the item's ONE multi-scalar
// multiplication with the first of the item's three factors, a_0: its row grows by kExtra points behind the statement slots,
//   B (already normalised for forming D)   -a_0        A   +a_0        M   +a_0 alpha
// and a_0 beta is added to the weights of G_0..G_{ell-1} (the convention of subarg_check_plan.hpp: sum_k a_k (<x_k, V_k> - lhs_k)).
//   bytes          gp's | the encodings of A | of M per item       (B's encoding, the proof's first 48 bytes, goes to gp's by_B)
//   status bytes   gp's | the decoder's verdict of B [count]
//   Fr memory      gp's | a_0 per item | vec_a, ell per item | same-perm alpha, beta per item
//   index words    gp's | the row slots of A, then of M [count] each
//   Jacobian       the check's count * 3 inputs (crs_U and, unused here, B) | A | M
struct SamePermCheckPlan {
  GprodCheckPlan gp;
  static constexpr size_t kExtra = 3;

  CPX_HD size_t count() const { return gp.count(); }
  CPX_HD size_t ell() const { return gp.ell; }
  CPX_HD int checks() const { return 1 + gp.sp.checks(); }
  CPX_HD size_t challenges() const { return 2 + gp.challenges(); }
  CPX_HD size_t message_bytes() const { return 8 + 32 * ell(); }
  static constexpr size_t kHead = 48;                                    // B ahead of the grand-product proof's bytes
  CPX_HD size_t proof_bytes() const { return kHead + gp.proof_bytes(); }
  // ---- the row's extension ----
  CPX_HD size_t row_B() const { return gp.sp.statement_off() + SubargCheckPlan::kStatement; }
  CPX_HD size_t row_A() const { return row_B() + 1; }
  CPX_HD size_t row_M() const { return row_B() + 2; }
  // ---- bytes, status bytes ----
  CPX_HD size_t by_A() const { return gp.by_total(); }
  CPX_HD size_t by_M() const { return by_A() + count() * 48; }
  CPX_HD size_t by_total() const { return by_M() + count() * 48; }
  CPX_HD size_t st_B() const { return gp.st_total(); }
  CPX_HD size_t st_total() const { return st_B() + count(); }
  // ---- Fr memory ----
  CPX_HD size_t fr_a0() const { return gp.fr_total(); }
  CPX_HD size_t fr_a() const { return fr_a0() + count(); }
  CPX_HD size_t fr_chal() const { return fr_a() + count() * ell(); }
  CPX_HD size_t fr_total() const { return fr_chal() + 2 * count(); }
  // ---- index words, Jacobian inputs ----
  CPX_HD size_t ix_AM_dst() const { return gp.ix_total(); }
  CPX_HD size_t ix_total() const { return ix_AM_dst() + 2 * count(); }
  CPX_HD size_t jac_A() const { return count() * SubargCheckPlan::kStatement; }
  CPX_HD size_t jac_total() const { return jac_A() + 2 * count(); }
  void fill_idx(std::vector<uint32_t>& ix) const {                       // the list of A's and M's row slots, relative to ix_AM_dst()
    ix.resize(2 * count());
    for (size_t i = 0; i < count(); i++) {
      ix[i] = (uint32_t)(i * gp.sp.points() + row_A());
      ix[count() + i] = (uint32_t)(i * gp.sp.points() + row_M());
    }
  }
  SubargTotals totals() const {                                          // (the dense affine points are gp's)
    const SubargTotals t = gp.totals();
    return {fr_total(), jac_total(), t.aff, by_total(), st_total(), ix_total(), t.tasks, t.res, kHead + t.lead_bytes, 2 + t.lead_challenges};
  }
};

// the argument rules are those of the grand-product verifier; the limit counts the three further points of every row
inline SubargPlanStatus same_perm_check_plan(size_t count, size_t ell, size_t n_blinders, SamePermCheckPlan& pl) {
  pl.gp.ell = ell;
  pl.gp.nb = n_blinders;
  return subarg_check_plan(true, count, ell + n_blinders, pl.gp.sp, SamePermCheckPlan::kExtra);
}

}  // namespace cpx
