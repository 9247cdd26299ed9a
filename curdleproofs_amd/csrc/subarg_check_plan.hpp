// Planner of the stand-alone sub-argument verifiers (cpx_ipa_verify, cpx_same_msm_verify; the core layer of Engine::subarg_verify,
// engine_subarg.cpp) — host code without a HIP call.  `count` independent items of n = 2^L elements: InnerProductProof::verify (inner_product_argument.rs:202-326) or
// SameMultiscalarProof::verify (same_multiscalar_argument.rs:153-261), each against an MsmAccumulator of its own
// (msm_accumulator.rs:37-68) whose random factors a_1, a_2 (, a_3) the caller drew.  The accumulator's verdict is flattened into ONE
// multi-scalar multiplication per item:
//     accepted  <=>  sum_k a_k (<x_k, V_k> - lhs_k) == O
// over the item's row of points, every point with one weight.  This header is the one statement of where an item's points and scalars
// sit and of those weights, for Engine::subarg_verify, k_subarg_scalars (subarg.hip) and tests/host_emul/subarg_check_plan_emul.cpp,
// which compiles it for the CPU (tests/test_subarg_verify_cpu.py).
//
//   proof bytes        IPA: B_c B_d | L_C [L] | R_C [L] | L_D [L] | R_D [L] | c_final d_final           48 (2 + 4L) + 64
//   (`serialize`)      SameMSM: B_a B_t B_u | L_A L_T L_U R_A R_T R_U [L each] | x_final                48 (3 + 6L) + 32
//   point row          IPA: G [n] | the proof's points in byte order | crs_H C D                        n + 4L + 5 points
//                      SameMSM: G [n] | T [n] | U [n] | the proof's points in byte order | A Z_t Z_u    3n + 6L + 6 points
//   weights            G_i    a1 c s_i + a2 d u_i / s_i          resp.  G_i, T_i, U_i   a_k x s_i
//                      crs_H  a1 beta (c d - alpha^2 z)
//                      B_*    -a_k                               L_*[j]  -a_k gamma_j          R_*[j]  -a_k / gamma_j
//                      C, D   -a_k alpha                         resp.  A, Z_t, Z_u     -a_k alpha
//   with s_i = prod_{j : bit L-1-j of i set} gamma_j (util.rs:40-64) and 1 / s_i the same product over the inverted challenges.
// The row is contiguous, so an item is one plain task of the tier-0 MSM chain: the decoder and the normaliser scatter their outputs
// into it (dst_index), no gather list is needed.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>
#include "mont32.hpp"
#include "tier0_plan.hpp"

namespace cpx {

enum SubargPlanStatus { SUBARG_OK = 0, SUBARG_NOT_POW2 = 1, SUBARG_TOO_LARGE = 2 };

struct SubargCheckPlan {
  bool ipa = true;
  size_t count = 0, n = 0, L = 0;
  size_t extra = 0;   // further points behind the statement slots, weighted by the caller's own kernel (same_perm_plan.hpp); 0 for every other check

  // ---- what an item consists of ----
  CPX_HD int checks() const { return ipa ? 2 : 3; }                     // accumulate_check calls = random factors per item
  CPX_HD int families() const { return ipa ? 1 : 3; }                   // G resp. G | T | U
  CPX_HD size_t proof_points() const { return ipa ? 2 + 4 * L : 3 + 6 * L; }
  CPX_HD size_t proof_scalars() const { return ipa ? 2 : 1; }
  CPX_HD size_t proof_bytes() const { return 48 * proof_points() + 32 * proof_scalars(); }
  CPX_HD size_t point_byte(size_t slot) const { return 48 * slot; }     // of proof point `slot` inside the proof
  CPX_HD size_t scalar_byte(size_t i) const { return 48 * proof_points() + 32 * i; }
  static constexpr size_t kStatement = 3;                               // crs_H, C, D resp. A, Z_t, Z_u
  CPX_HD size_t challenges() const { return (ipa ? 2 : 1) + L; }        // alpha, beta, gamma_1..L resp. alpha, gamma_1..L
  // ---- proof point slots, in byte order ----
  CPX_HD int terms() const { return ipa ? 4 : 6; }                      // cross terms per round
  CPX_HD size_t first_round_slot() const { return ipa ? 2 : 3; }
  // block b of the cross terms (L slots each): IPA 0 L_C, 1 R_C, 2 L_D, 3 R_D; SameMSM 0..2 L_A L_T L_U, 3..5 R_A R_T R_U
  CPX_HD size_t block_slot(int b, size_t j) const { return first_round_slot() + (size_t)b * L + j; }
  // the q-th point round j appends to the transcript: L_C, L_D, R_C, R_D resp. L_A, L_T, L_U, R_A, R_T, R_U
  CPX_HD size_t round_slot(size_t j, int q) const { return block_slot(ipa ? ((q & 1) << 1 | (q >> 1)) : q, j); }
  CPX_HD bool block_is_right(int b) const { return ipa ? (b & 1) : b >= 3; }
  CPX_HD int block_check(int b) const { return ipa ? b >> 1 : b % 3; }  // which accumulate_check (random factor) the block belongs to
  // ---- the point row of an item ----
  CPX_HD size_t base_off(int f) const { return (size_t)f * n; }
  CPX_HD size_t proof_off() const { return (size_t)families() * n; }
  CPX_HD size_t statement_off() const { return proof_off() + proof_points(); }
  CPX_HD size_t points() const { return statement_off() + kStatement + extra; }
  // ---- Fr memory of the call: weights [count][points] | z [count] | vec_u [count][n] (IPA) | factors [count][checks] | challenges ----
  CPX_HD size_t fr_weights() const { return 0; }
  CPX_HD size_t fr_z() const { return count * points(); }
  CPX_HD size_t fr_u() const { return fr_z() + (ipa ? count : 0); }
  CPX_HD size_t fr_rand() const { return fr_u() + (ipa ? count * n : 0); }
  CPX_HD size_t fr_challenges() const { return fr_rand() + count * (size_t)checks(); }
  CPX_HD size_t fr_total() const { return fr_challenges() + count * challenges(); }
  // ---- bytes of the call: proofs | statement encodings [count][3][48] | T, U encodings [count][2n][48] (SameMSM) ----
  CPX_HD size_t by_proofs() const { return 0; }
  CPX_HD size_t by_statement() const { return (count * proof_bytes() + 15) / 16 * 16; }
  CPX_HD size_t by_tu() const { return by_statement() + count * kStatement * 48; }
  CPX_HD size_t by_total() const { return by_tu() + (ipa ? 0 : count * 2 * n * 48); }
  // ---- index words: the decoder's byte offsets and destinations [count][proof_points] each, the normaliser's destinations [count][3] ----
  CPX_HD size_t ix_src() const { return 0; }
  CPX_HD size_t ix_dst() const { return count * proof_points(); }
  CPX_HD size_t ix_statement() const { return 2 * count * proof_points(); }
  CPX_HD size_t ix_total() const { return ix_statement() + count * kStatement; }
  // ---- status bytes: the decoder's verdicts [count][proof_points] | the items' flags [count]; Jacobian inputs: the statement points
  // [count][3]; dense affine points: none (gprod_plan.hpp has some) ----
  CPX_HD size_t st_bad() const { return count * proof_points(); }
  CPX_HD size_t st_total() const { return st_bad() + count; }
  CPX_HD size_t jac_total() const { return count * kStatement; }
  CPX_HD size_t aff_total() const { return 0; }
  void fill_idx(std::vector<uint32_t>& ix) const {
    ix.resize(ix_total());
    const size_t pp = proof_points();
    for (size_t i = 0; i < count; i++) {
      for (size_t s = 0; s < pp; s++) {
        ix[ix_src() + i * pp + s] = (uint32_t)(by_proofs() + i * proof_bytes() + point_byte(s));
        ix[ix_dst() + i * pp + s] = (uint32_t)(i * points() + proof_off() + s);
      }
      for (size_t k = 0; k < kStatement; k++) ix[ix_statement() + i * kStatement + k] = (uint32_t)(i * points() + statement_off() + k);
    }
  }
  // the MSM plan: one task per item, its row
  bool msm(Tier0MsmPlan& pl, std::vector<uint32_t>& lens) const {
    lens.assign(count, (uint32_t)points());
    return tier0_msm_plan(count, lens.data(), pl);
  }
  SubargTotals totals() const { return {fr_total(), jac_total(), aff_total(), by_total(), st_total(), ix_total(), count, count, 0, 0}; }   // one task, one sum per item
};

// An item is one task of one cpx_g1_msm_many: at most kTier0ManyTasks items of together count * points() <= kTier0ManyPoints points (which
// also keeps every byte offset of the call below 2^32).  Looked at before anything is read.
inline SubargPlanStatus subarg_check_plan(bool ipa, size_t count, size_t n, SubargCheckPlan& pl, size_t extra = 0) {
  if (!n || (n & (n - 1))) return SUBARG_NOT_POW2;
  pl.ipa = ipa;
  pl.extra = extra;
  pl.count = count;
  pl.n = n;
  pl.L = 0;
  while (((size_t)1 << pl.L) < n) pl.L++;
  if (count > kTier0ManyTasks || n > kTier0ManyPoints) return SUBARG_TOO_LARGE;
  if (count && pl.points() > kTier0ManyPoints / count) return SUBARG_TOO_LARGE;
  return SUBARG_OK;
}

// s_i = prod_{j : bit (L-1-j) of i set} g_j (util.rs:40-64), per index: what the device does (k_vs_scalars, k_subarg_scalars); with the
// inverted challenges it is 1 / s_i, the value ark_ff::batch_inversion gives the reference
template <class F>
CPX_HD F verification_scalar(const F* g, int L, int i) {
  F r = F::one();
  for (int j = 0; j < L; j++)
    if ((i >> (L - 1 - j)) & 1) r = fe_mul(r, g[j]);
  return r;
}

// The weights, in gather form (the weight OF a point) over a scalar type F with fe_mul / fe_add / fe_sub / fe_neg (Fr: mont32.hpp).
template <class F>
struct SubargTerms {
  F a[3];                   // the item's random factors, in the order accumulate_check draws them
  F alpha, beta, z;         // beta, z: IPA only
  F fin[2];                 // c_final, d_final resp. x_final
  const F *gam, *gam_inv;   // [L]
  F af[3], h;               // a_1 c, a_2 d resp. a_k x; the weight of crs_H: set()
  CPX_HD void set(bool ipa) {
    if (ipa) {
      af[0] = fe_mul(a[0], fin[0]);
      af[1] = fe_mul(a[1], fin[1]);
      h = fe_mul(fe_mul(a[0], beta), fe_sub(fe_mul(fin[0], fin[1]), fe_mul(fe_mul(alpha, alpha), z)));
    } else {
      af[0] = fe_mul(a[0], fin[0]), af[1] = fe_mul(a[1], fin[0]), af[2] = fe_mul(a[2], fin[0]);
    }
  }
};
// base i of family f, given s_i and (IPA) u_i / s_i
template <class F>
CPX_HD F subarg_base_weight(const SubargTerms<F>& t, bool ipa, int f, const F& s_i, const F& u_over_s) {
  if (ipa) return fe_add(fe_mul(t.af[0], s_i), fe_mul(t.af[1], u_over_s));
  F w = t.af[0];   // (a factor picked by a run-time index is copied: check_weights.hpp misc_weight)
  if (f == 1) w = t.af[1];
  if (f == 2) w = t.af[2];
  return fe_mul(w, s_i);
}
// proof point `slot` (byte order)
template <class F>
CPX_HD F subarg_proof_weight(const SubargTerms<F>& t, const SubargCheckPlan& pl, int slot) {
  const int first = (int)pl.first_round_slot(), L = (int)pl.L;
  int k, b = -1, j = 0;
  if (slot < first) {
    k = slot;   // B_c, B_d resp. B_a, B_t, B_u
  } else {
    b = (slot - first) / L, j = (slot - first) % L;
    k = pl.block_check(b);
  }
  F w = t.a[0];
  if (k == 1) w = t.a[1];
  if (k == 2) w = t.a[2];
  if (b >= 0) w = fe_mul(w, pl.block_is_right(b) ? t.gam_inv[j] : t.gam[j]);
  return fe_neg(w);
}
// statement point k: crs_H, C, D resp. A, Z_t, Z_u
template <class F>
CPX_HD F subarg_statement_weight(const SubargTerms<F>& t, bool ipa, int k) {
  if (ipa && k == 0) return t.h;
  F w = t.a[0];
  const int c = ipa ? k - 1 : k;
  if (c == 1) w = t.a[1];
  if (c == 2) w = t.a[2];
  return fe_neg(fe_mul(w, t.alpha));
}

}  // namespace cpx
