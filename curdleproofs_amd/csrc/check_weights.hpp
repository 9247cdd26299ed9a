// The weights of the verifier's accumulated check — the ONE definition both verifier paths use: the host-driven one
// (host_verify.hpp, over host::S) and the device-resident one (k_vs_scalars of protocol.hip, over Fr).  No HIP.
//
// The verifier folds every check of a proof into one sum  sum_i a_i (lhs_i - x_i . V_i) == O  (msm_accumulator.rs:38-68),
// flattened here into one weight per point:
//   CRS part       G | Hvec (n bases)                                  crs_weight
//   instance part  R | S | T | U (ell each)                            instance_weights
//   misc part      the CRS singles, M and every proof point (slots)    misc_weight
// from inner_product_argument.rs:202-326, same_scalar_argument.rs:112-137, same_multiscalar_argument.rs:153-261,
// grand_product_argument.rs:211-246, same_permutation_argument.rs:146-171 and curdleproofs.rs:283-297.
//
// All three are in gather form (the weight OF a point) over a scalar type F with fe_mul / fe_add / fe_sub / fe_neg: Fr has them in
// mont32.hpp, host::S in host_math.hpp.  How s_i = prod_{j : bit (L-1-j) of i set} gamma_j (util.rs:40-64) is produced is the
// caller's business: by doubling on the host, per index on the device.
#pragma once
#include "layout.hpp"

namespace cpx {

template <class F>
struct CheckTerms {
  F a1, a2, a3, a4, a5, a6, a7, a8;   // the caller's random factors (layout.hpp VF_*)
  F w1, w2, w3, w4;                   // weights of the four SameScalar equalities: set_same_scalar_weights
  F alpha_sp, beta_sp, alpha_g, beta_g_inv, alpha_i, beta_i, alpha_s, alpha_m;   // challenges
  F c_fin, d_fin, z_k, z_t, z_u, x_fin;   // the proof's scalars (r_p enters through z_ip)
  F z_ip;                                 // r_p beta^(ell+1) + gprod beta^ell - 1 (grand_product_argument.rs:224-227)
  const F *gam_i, *gam_i_inv, *gam_m, *gam_m_inv;   // [L] round challenges of the IPA and of SameMSM, and their inverses
  F sm_l2, sm_l3;                         // s_m[ell + 2], s_m[ell + 3]: the SameMSM scalars of G_t and G_u
  F a2c, a3d, a4x, a5x, a6x, a1b, a4am, a5am, a6am, a3ai;   // products that several weights share: set_factors

  // f: the proof's row of random factors.  The challenges and the proof's scalars must be set.
  CPX_HD void set_factors(const F* f) {
    a1 = f[VF_SAMEPERM], a2 = f[VF_IPA_C], a3 = f[VF_IPA_D], a4 = f[VF_SMSM_A], a5 = f[VF_SMSM_T], a6 = f[VF_SMSM_U], a7 = f[VF_R], a8 = f[VF_S];
    a2c = fe_mul(a2, c_fin), a3d = fe_mul(a3, d_fin), a4x = fe_mul(a4, x_fin), a5x = fe_mul(a5, x_fin), a6x = fe_mul(a6, x_fin);
    a1b = fe_mul(a1, beta_sp);
    a4am = fe_mul(a4, alpha_m), a5am = fe_mul(a5, alpha_m), a6am = fe_mul(a6, alpha_m), a3ai = fe_mul(a3, alpha_i);
  }
  // The four SameScalar equalities (same_scalar_argument.rs:127-137) join the accumulated sum with random weights of their own:
  // factors 9..12 of a fused batch; for per-proof verdicts the pairwise products a1 a2, a3 a4, a5 a6, a7 a8 of the caller's eight
  // factors — the accumulated sum is then a polynomial of degree 2 in independent uniform factors whose coefficients are the
  // individual check values, so it vanishes with probability <= 2/r unless every check holds (Schwartz-Zippel), the same argument
  // that backs msm_accumulator.rs itself.  (f has VF_FUSED_COUNT entries when fused, VF_COUNT otherwise.)
  CPX_HD void set_same_scalar_weights(const F* f, bool fused) {
    if (fused) {
      w1 = f[VF_SS_A1], w2 = f[VF_SS_A2], w3 = f[VF_SS_B1], w4 = f[VF_SS_B2];
    } else {
      w1 = fe_mul(a1, a2), w2 = fe_mul(a3, a4), w3 = fe_mul(a5, a6), w4 = fe_mul(a7, a8);
    }
  }
};

// (1) weight of column i of G | Hvec, given s_i, s_i^-1 u_i (u of grand_product_argument.rs:211-219) and the SameMSM scalar s_m,i
template <class F>
CPX_HD F crs_weight(const CheckTerms<F>& t, int i, int ell, const F& s_i, const F& s_inv_u, const F& s_m) {
  F k = fe_add(fe_mul(t.a2c, s_i), fe_mul(t.a3d, s_inv_u));
  if (i < ell) k = fe_add(k, t.a1b);
  if (i < ell + 2) k = fe_add(k, fe_mul(t.a4x, s_m));   // G_b = G | Hvec[0..2) | G_t | G_u
  return fe_neg(k);
}

// (2) weights of R_i, S_i, T_i, U_i (i < ell), given vec_a[i] and s_m,i
template <class F>
CPX_HD void instance_weights(const CheckTerms<F>& t, const F& vec_a_i, const F& s_m, F k[4]) {
  k[0] = fe_neg(fe_mul(t.a7, vec_a_i));
  k[1] = fe_neg(fe_mul(t.a8, vec_a_i));
  k[2] = fe_neg(fe_mul(t.a5x, s_m));
  k[3] = fe_neg(fe_mul(t.a6x, s_m));
}

// (3) weight of slot s < SL_A + n_points(): a CRS single, M or a proof point.  The SameScalar equalities, each "... == O":
//   cm_A.T_1 + alpha cm_T.T_1 - z_t G_t,   cm_A.T_2 + alpha cm_T.T_2 - z_k R - z_t H,
//   cm_B.T_1 + alpha cm_U.T_1 - z_u G_u,   cm_B.T_2 + alpha cm_U.T_2 - z_k S - z_u H
template <class F>
CPX_HD F misc_weight(const CheckTerms<F>& t, const SlotMap& sm, int s) {
  const int L = sm.L;
  if (s == SL_H) {
    const F k = fe_sub(fe_sub(fe_sub(fe_mul(t.a2, fe_mul(fe_mul(fe_mul(t.alpha_i, t.alpha_i), t.z_ip), t.beta_i)), fe_mul(fe_mul(t.a2c, t.d_fin), t.beta_i)),
                              fe_mul(t.a5x, t.sm_l2)),
                       fe_mul(t.a6x, t.sm_l3));
    return fe_sub(fe_sub(k, fe_mul(t.w2, t.z_t)), fe_mul(t.w4, t.z_u));
  }
  if (s == SL_GT) return fe_neg(fe_add(fe_mul(t.a4x, t.sm_l2), fe_mul(t.w1, t.z_t)));
  if (s == SL_GU) return fe_neg(fe_add(fe_mul(t.a4x, t.sm_l3), fe_mul(t.w3, t.z_u)));
  if (s == SL_GSUM) return fe_neg(fe_mul(t.a3ai, t.beta_g_inv));
  if (s == SL_HSUM) return fe_mul(t.a3ai, t.alpha_g);
  if (s == SL_M) return fe_neg(fe_mul(t.a1, t.alpha_sp));
  if (s == SL_A) return fe_sub(t.a4am, t.a1);
  if (s == SL_CMT1) return fe_add(t.a4am, fe_mul(t.w1, t.alpha_s));
  if (s == SL_CMT2) return fe_add(t.a5am, fe_mul(t.w2, t.alpha_s));
  if (s == SL_CMU1) return fe_add(t.a4am, fe_mul(t.w3, t.alpha_s));
  if (s == SL_CMU2) return fe_add(t.a6am, fe_mul(t.w4, t.alpha_s));
  if (s == SL_R) return fe_sub(t.a7, fe_mul(t.w2, t.z_k));
  if (s == SL_S) return fe_sub(t.a8, fe_mul(t.w4, t.z_k));
  if (s == SL_B) return fe_add(t.a1, t.a3ai);
  if (s == SL_C) return fe_mul(t.a2, t.alpha_i);
  if (s == SL_BC) return t.a2;
  if (s == SL_BD) return t.a3;
  if (s < sm.CMA1()) {   // IPA cross terms: L_C | R_C | L_D | R_D, L each
    // (a factor picked by a run-time index is copied: a reference into CheckTerms chosen at run time would keep the whole struct in
    // the kernel's scratch memory)
    const int q = s - SL_IPA0, blk = q / L, j = q % L;
    const F* g = (blk & 1) ? t.gam_i_inv : t.gam_i;
    F a = t.a2;
    if (blk >= 2) a = t.a3;
    return fe_mul(a, g[j]);
  }
  if (s == sm.CMA1()) return t.w1;
  if (s == sm.CMA2()) return t.w2;
  if (s == sm.CMB1()) return t.w3;
  if (s == sm.CMB2()) return t.w4;
  if (s == sm.BA()) return t.a4;
  if (s == sm.BT()) return t.a5;
  if (s == sm.BU()) return t.a6;
  // SameMSM cross terms: L_A | L_T | L_U | R_A | R_T | R_U, L each
  const int q = s - sm.LA(0), blk = q / L, j = q % L, col = blk % 3;
  const F* g = blk < 3 ? t.gam_m : t.gam_m_inv;
  F a = t.a4;
  if (col == 1) a = t.a5;
  if (col == 2) a = t.a6;
  return fe_mul(a, g[j]);
}

}  // namespace cpx
