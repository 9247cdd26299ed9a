// The Fiat-Shamir schedule of CurdleproofsProof::{new, verify}, spelled ONCE for the two host paths: the host-driven prover
// (host_prove.hpp) and the host verifier (host_verify.hpp) absorb the same messages under the same labels and draw the same challenges;
// they differ in where a point's bytes come from.  So every step takes `slot`, a callable that returns the 48 compressed bytes of a
// SlotMap slot: the prover reads its registry of compressed results, the verifier the proof bytes and the two points it computed, D and
// A'.  With them the two bits of challenge algebra both sides need.  The device-resident paths hash the same schedule in protocol.hip;
// tests/transcript_cases.py restates it independently.  No HIP.
#pragma once
#include "host_math.hpp"
#include "layout.hpp"

namespace cpx {
namespace host {

// curdleproofs.rs:81-83 / 223-225: the instance rows R | S | T | U (ic: ell compressed points each) and M; returns vec_a
inline SVec absorb_instance(Transcript& tr, size_t ell, const uint8_t* ic, const uint8_t* mcomp) {
  const char* const step = "curdleproofs_step1";
  for (int v = 0; v < 4; v++) tr.append_point_vec_bytes(step, ic + v * ell * 48, ell);
  tr.append_point_bytes(step, mcomp);
  return tr.get_and_append_challenges("curdleproofs_vec_a", ell);
}
// same_permutation_argument.rs:60-63 / 134-137
template <class Slot> void same_perm_challenges(Transcript& tr, Slot&& slot, const SVec& vec_a, S* alpha, S* beta) {
  const char* const step = "same_perm_step1";
  tr.append_point_bytes(step, slot(SL_A));
  tr.append_point_bytes(step, slot(SL_M));
  tr.append_scalar_vec(step, vec_a);
  *alpha = tr.get_and_append_challenge("same_perm_alpha");
  *beta = tr.get_and_append_challenge("same_perm_beta");
}
// grand_product_argument.rs:63-65 / 202-204: returns alpha
template <class Slot> S gprod_step1(Transcript& tr, Slot&& slot, const S& gprod) {
  const char* const step = "gprod_step1";
  tr.append_point_bytes(step, slot(SL_B));
  tr.append_scalar(step, gprod);
  return tr.get_and_append_challenge("gprod_alpha");
}
// grand_product_argument.rs:83-85 / 207-209: returns beta
template <class Slot> S gprod_step2(Transcript& tr, Slot&& slot, const S& r_p) {
  const char* const step = "gprod_step2";
  tr.append_point_bytes(step, slot(SL_C));
  tr.append_scalar(step, r_p);
  return tr.get_and_append_challenge("gprod_beta");
}
// inner_product_argument.rs:129-133 / 283-287
template <class Slot> void ipa_step1(Transcript& tr, const SlotMap& sm, Slot&& slot, const S& z_ip, S* alpha, S* beta) {
  const char* const step = "ipa_step1";
  tr.append_point_bytes(step, slot(SL_C));
  tr.append_point_bytes(step, slot(sm.D()));
  tr.append_scalar(step, z_ip);
  tr.append_point_bytes(step, slot(SL_BC));
  tr.append_point_bytes(step, slot(SL_BD));
  *alpha = tr.get_and_append_challenge("ipa_alpha");
  *beta = tr.get_and_append_challenge("ipa_beta");
}
// one round of inner_product_argument.rs:169-170 / same_multiscalar_argument.rs:121-122: the round's points in SlotMap order; returns gamma
template <class Slot> S ipa_round_gamma(Transcript& tr, const SlotMap& sm, int j, Slot&& slot) {
  int q[4];
  sm.ipa_round(j, q);
  for (int s : q) tr.append_point_bytes("ipa_loop", slot(s));
  return tr.get_and_append_challenge("ipa_gamma");
}
template <class Slot> S smsm_round_gamma(Transcript& tr, const SlotMap& sm, int j, Slot&& slot) {
  int q[6];
  sm.same_msm_round(j, q);
  for (int s : q) tr.append_point_bytes("same_msm_loop", slot(s));
  return tr.get_and_append_challenge("same_msm_gamma");
}
// same_scalar_argument.rs:63-70 / 111-126: returns alpha
template <class Slot> S same_scalar_alpha(Transcript& tr, const SlotMap& sm, Slot&& slot) {
  int q[10];
  sm.sameexp_points(q);
  for (int s : q) tr.append_point_bytes("sameexp_points", slot(s));
  return tr.get_and_append_challenge("same_scalar_alpha");
}
// same_multiscalar_argument.rs:84-87 / 230-233: A', cm_T.T_2, cm_U.T_2, then the two
// n-point vectors T | O O H O and U | O O O H (ic: the instance rows, O: the identity, crs_h_comp: the compressed H of the CRS), then
// B_a, B_t, B_u; returns alpha
template <class Slot> S same_msm_step1(Transcript& tr, const SlotMap& sm, Slot&& slot, size_t ell, const uint8_t* ic, const uint8_t* crs_h_comp) {
  const char* const step = "same_msm_step1";
  const size_t n = ell + N_BLINDERS;
  tr.append_point_bytes(step, slot(sm.APRIME()));
  tr.append_point_bytes(step, slot(SL_CMT2));
  tr.append_point_bytes(step, slot(SL_CMU2));
  std::vector<uint8_t> vb(n * 48);
  for (size_t v = 2; v < 4; v++) {   // the row of T with H at ell + 2, the row of U with H at ell + 3
    memcpy(vb.data(), ic + v * ell * 48, ell * 48);
    memset(&vb[ell * 48], 0, N_BLINDERS * 48);
    for (size_t i = 0; i < N_BLINDERS; i++) vb[(ell + i) * 48] = kCompIdentity;
    memcpy(&vb[(ell + v) * 48], crs_h_comp, 48);
    tr.append_point_vec_bytes(step, vb.data(), n);
  }
  tr.append_point_bytes(step, slot(sm.BA()));
  tr.append_point_bytes(step, slot(sm.BT()));
  tr.append_point_bytes(step, slot(sm.BU()));
  return tr.get_and_append_challenge("same_msm_alpha");
}

// u_i = beta^-(i+1) for i < ell, beta^-(ell+1) on the blinder entries (grand_product_argument.rs:90-102 / 213-220): the rescaling G' = u o G
inline void u_powers(const S& beta_inv, size_t ell, S* u) {
  S pw = beta_inv;
  for (size_t i = 0; i < ell; i++) {
    u[i] = pw;
    pw *= beta_inv;
  }
  for (size_t i = ell; i < ell + N_BLINDERS; i++) u[i] = pw;
}
// the inner product the IPA proves: z = r_p beta^(ell+1) + gprod beta^ell - 1 (grand_product_argument.rs:141 / 230); beta_l1 receives beta^(ell+1)
inline S gprod_inner_product(const S& r_p, const S& gprod, const S& beta, size_t ell, S* beta_l1) {
  const S beta_l = beta.pow_u64(ell);
  *beta_l1 = beta_l * beta;
  return r_p * *beta_l1 + gprod * beta_l - S::one();
}

}  // namespace host
}  // namespace cpx
