// Planner of the log-round loops as one call (cpx_ipa_rounds, cpx_same_msm_rounds; Engine::loop_rounds) — host code without a HIP call.
// `count` independent items of n = 2^L elements run inner_product_argument.rs:150-186 or same_multiscalar_argument.rs:99-136 in the
// all-MSM form: no basis is ever folded.  Per item the device keeps the scalar vectors and one fold coefficient per
// original base, starting at 1; round j (half = n >> (j + 1)) multiplies the coefficients of the bases whose index has bit `half` set by
// gamma_j or its inverse, and every cross term of every round is an MSM of n/2 of the ORIGINAL bases, gathered through an index list that
// depends on (n, j) only:
//     lo_j[t] = (t / half) * 2 half + t % half,   hi_j[t] = lo_j[t] + half,   t < n/2
// with scalar t = (entry t % half of the folded vector's left or right half) x (the coefficient of base idx[t]) — round_algebra.hpp.
// One definition of where everything lives for Engine::loop_rounds, k_loop_step (loop.hip) and tests/host_emul/loop_plan_emul.cpp, which
// compiles it for the CPU (tests/test_loop_rounds_cpu.py).
//
//   bases, per item    IPA: G [n] | G' [n] | H [1]  (H = the loop's local crs_H * beta, index 2n of the item)     SameMSM: G [n] | T [n] | U [n]
//   vectors, per item  IPA: c | d | SG | SGp  (4n Fr)                                                              SameMSM: x | SM  (2n Fr)
//   scalar row         IPA: L_C (n/2), <c_L,d_R> | L_D (n/2) | R_C (n/2), <c_R,d_L> | R_D (n/2)  (2n + 2 Fr)       SameMSM: L_* (n/2) | R_* (n/2)  (n Fr)
//   tasks of a round   item-major, the item's cross terms in transcript order: L_C L_D R_C R_D / L_A L_T L_U R_A R_T R_U
//   results            [L][count][terms]: round j's sums, affine points and 48-byte encodings at (j count + item) terms + q
// An IPA index list carries H's index behind its n/2 entries: the L_C and R_C tasks read n/2 + 1 entries and find the inner product as
// their last scalar, L_D and R_D read the first n/2 of the same list from G'.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "tier0_plan.hpp"

namespace cpx {

enum LoopPlanStatus { LOOP_OK = 0, LOOP_NOT_POW2 = 1, LOOP_TOO_LARGE = 2 };

struct LoopPlan {
  bool ipa = true;
  size_t count = 0, n = 0, L = 0;

  int terms() const { return ipa ? 4 : 6; }
  size_t hn() const { return n / 2; }
  size_t tasks() const { return count * (size_t)terms(); }                       // per round
  size_t round_points() const { return count * (ipa ? 2 * n + 2 : 3 * n); }      // per round: every task's n/2 (+ 1)
  // ---- bases ----
  size_t base_stride() const { return ipa ? 2 * n + 1 : 3 * n; }                 // points per item
  size_t h_index() const { return 2 * n; }                                       // IPA: H, relative to the item's G
  int term_family(int q) const { return ipa ? (q & 1) : q % 3; }                 // IPA: 0 = G, 1 = G'; SameMSM: 0 = G, 1 = T, 2 = U
  size_t family_off(int f) const { return (size_t)f * n; }
  bool term_hi(int q) const { return ipa ? (q == 0 || q == 3) : q < 3; }         // the L terms of G / T / U and R_D read the hi bases
  bool term_has_h(int q) const { return ipa && (q == 0 || q == 2); }
  uint32_t term_len(int q) const { return (uint32_t)(hn() + (term_has_h(q) ? 1 : 0)); }
  // ---- the folded vectors a term's scalars come from, and what a round does to the fold coefficients ----
  int term_vec(int q) const { return ipa ? (q & 1) : 0; }                        // IPA: 0 = c, 1 = d; SameMSM: x
  bool term_vec_right(int q) const { return ipa ? (q == 1 || q == 2) : q >= 3; } // L_D takes d_R, R_C takes c_R, the R terms x_R
  int family_gamma_power(int f) const { return ipa && f == 1 ? -1 : 1; }         // coefficient[hi] *= gamma^power; G' folds by the inverse
  int vec_gamma_power(int v) const { return ipa && v == 1 ? 1 : -1; }            // v_L += gamma^power v_R: c and x by the inverse, d by gamma
  // ---- Fr memory: vectors | scalar rows | ones (IPA: beta of the shared formulas) | challenges | finals ----
  size_t vec_words() const { return (ipa ? 4 : 2) * n; }
  size_t row_words() const { return ipa ? 2 * n + 2 : n; }
  size_t scal_off(int q) const {
    if (!ipa) return q < 3 ? 0 : hn();
    const size_t o[4] = {0, hn() + 1, 2 * hn() + 1, 3 * hn() + 2};
    return o[q];
  }
  size_t finals_each() const { return ipa ? 2 : 1; }
  size_t fr_vec() const { return 0; }
  size_t fr_rows() const { return fr_vec() + count * vec_words(); }
  size_t fr_ones() const { return fr_rows() + count * row_words(); }
  size_t fr_gammas() const { return fr_ones() + (ipa ? count : 0); }
  size_t fr_finals() const { return fr_gammas() + count * L; }
  size_t fr_total() const { return fr_finals() + count * finals_each(); }
  // ---- index lists: per round lo then hi, idx_len() entries each ----
  size_t idx_len() const { return hn() + (ipa ? 1 : 0); }
  size_t idx_off(size_t j, bool hi) const { return (2 * j + (hi ? 1 : 0)) * idx_len(); }
  size_t idx_total() const { return 2 * L * idx_len(); }
  void fill_idx(std::vector<uint32_t>& idx) const {
    idx.assign(idx_total(), 0);
    for (size_t j = 0; j < L; j++) {
      const size_t half = n >> (j + 1);
      uint32_t *lo = idx.data() + idx_off(j, false), *hi = idx.data() + idx_off(j, true);
      for (size_t t = 0; t < hn(); t++) {
        lo[t] = (uint32_t)((t / half) * 2 * half + t % half);
        hi[t] = lo[t] + (uint32_t)half;
      }
      if (ipa) lo[hn()] = hi[hn()] = (uint32_t)h_index();
    }
  }
  // ---- results ----
  size_t result_index(size_t j, size_t item, int q) const { return (j * count + item) * (size_t)terms() + (size_t)q; }
  size_t results() const { return L * tasks(); }
  // the MSM plan of one round (the same for every round: the lengths do not depend on j); slices are the caller's (msm_tblw_slices)
  bool round_msm(Tier0MsmPlan& pl, std::vector<uint32_t>& lens) const {
    lens.resize(tasks());
    for (size_t i = 0; i < count; i++)
      for (int q = 0; q < terms(); q++) lens[i * (size_t)terms() + (size_t)q] = term_len(q);
    return tier0_msm_plan(lens.size(), lens.data(), pl);
  }
};

// The limits follow from those of one cpx_g1_msm_many, which a round is: terms * count <= kTier0ManyTasks MSMs (IPA: count <= 16384,
// SameMSM: count <= 10922) of together count (2n + 2) resp. 3 count n <= kTier0ManyPoints points.  Looked at before anything is read.
inline LoopPlanStatus loop_plan(bool ipa, size_t count, size_t n, LoopPlan& pl) {
  if (!n || (n & (n - 1))) return LOOP_NOT_POW2;
  pl.ipa = ipa;
  pl.count = count;
  pl.n = n;
  pl.L = 0;
  while (((size_t)1 << pl.L) < n) pl.L++;
  const size_t terms = (size_t)pl.terms();
  if (count > kTier0ManyTasks / terms) return LOOP_TOO_LARGE;
  if (n > kTier0ManyPoints) return LOOP_TOO_LARGE;
  const size_t per_item = ipa ? 2 * n + 2 : 3 * n;
  if (count && per_item > kTier0ManyPoints / count) return LOOP_TOO_LARGE;
  return LOOP_OK;
}

}  // namespace cpx
