// The host-driven verifier's per-proof work that needs no GPU: deserialising the proof's scalars, the Fiat-Shamir transcript and the
// scalars of the accumulated check.  Engine::verify_core (engine.cpp) launches and waits around these two steps and stages the scalars
// (VerifyState::scal) in the layout of check_plan.hpp, the same for every mode of the check; the device-resident path does the same
// work in k_vs_prefix / k_vs_scalars (protocol.hip).  No HIP: the tests compile this for the CPU.
#pragma once
#include "check_weights.hpp"
#include "host_math.hpp"

namespace cpx {
namespace host {

struct VerifyState {
  Transcript tr{"curdleproofs"};
  bool bad = false;           // deserialisation failure
  bool reject = false;        // structural rejection
  S r_p, c_fin, d_fin, z_k, z_t, z_u, x_fin;
  SVec vec_a;
  S alpha_sp, beta_sp, gprod, alpha_g, beta_g, beta_g_inv, z_ip, alpha_i, beta_i, alpha_s, alpha_m;
  SVec gam_i, gam_i_inv, gam_m, gam_m_inv;
  const uint8_t* pb;          // proof bytes
  // after verify_prefix: [0] the scalars of D; after verify_scalars: the weights of G | Hvec (n), R | S | T | U (4 ell) and the misc points
  SVec scal[3];
};

// V1a: the proof's scalars, the transcript up to the grand-product beta, the scalars of D.
// pb: the proof; ic: the compressed instance rows R | S | T | U (ell points each); mcomp: the compressed M.
inline void verify_prefix(VerifyState& s, size_t ell, size_t L, const uint8_t* pb, const uint8_t* ic, const uint8_t* mcomp) {
  const ProofLayout pl(L);
  s.pb = pb;
  auto P = [&](int slot_id) { return pb + pl.point_offset(slot_id - SL_A); };
  S* vals[ProofLayout::N_SCALARS] = {&s.r_p, &s.c_fin, &s.d_fin, &s.z_k, &s.z_t, &s.z_u, &s.x_fin};
  for (int i = 0; i < ProofLayout::N_SCALARS; i++)
    if (!S::from_le_bytes(pb + pl.scalar_offset(i), vals[i])) s.bad = true;
  // curdleproofs.rs:218: the randomiser must not have wiped the ciphertexts
  if (ic[2 * ell * 48] == kCompIdentity) s.reject = true;
  for (int v = 0; v < 4; v++) s.tr.append_point_vec_bytes("curdleproofs_step1", ic + v * ell * 48, ell);   // curdleproofs.rs:213-222
  s.tr.append_point_bytes("curdleproofs_step1", mcomp);
  s.vec_a = s.tr.get_and_append_challenges("curdleproofs_vec_a", ell);
  // same_permutation_argument.rs:131-145
  s.tr.append_point_bytes("same_perm_step1", P(SL_A));
  s.tr.append_point_bytes("same_perm_step1", mcomp);
  s.tr.append_scalar_vec("same_perm_step1", s.vec_a);
  s.alpha_sp = s.tr.get_and_append_challenge("same_perm_alpha");
  s.beta_sp = s.tr.get_and_append_challenge("same_perm_beta");
  s.gprod = S::one();
  for (size_t i = 0; i < ell; i++) s.gprod *= s.vec_a[i] + S::from_u64(i) * s.alpha_sp + s.beta_sp;
  // grand_product_argument.rs:200-209
  s.tr.append_point_bytes("gprod_step1", P(SL_B));
  s.tr.append_scalar("gprod_step1", s.gprod);
  s.alpha_g = s.tr.get_and_append_challenge("gprod_alpha");
  s.tr.append_point_bytes("gprod_step2", P(SL_C));
  s.tr.append_scalar("gprod_step2", s.r_p);
  s.beta_g = s.tr.get_and_append_challenge("gprod_beta");
  s.beta_g_inv = s.beta_g.inverse();
  s.scal[0] = {S::one(), -s.beta_g_inv, s.alpha_g};    // D = B - beta^-1 sum(G) + alpha sum(H)  (grand_product_argument.rs:223)
}

// V1c: the rest of the transcript and the weights of the accumulated check (check_weights.hpp).
// crs_h_comp: the compressed H of the CRS; d_comp, aprime_comp: D and A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.rs:258) compressed;
// factors: the proof's random factors in wire form, VF_FUSED_COUNT of them for a fused batch, else VF_COUNT.
inline void verify_scalars(VerifyState& s, size_t ell, size_t L, const uint8_t* ic, const uint8_t* crs_h_comp, const uint8_t* d_comp, const uint8_t* aprime_comp,
                           const uint8_t* factors, bool fused) {
  const size_t n = ell + 4;
  const SlotMap sm(L);
  const ProofLayout pl(L);
  const uint8_t* pb = s.pb;
  auto P = [&](int slot_id) { return pb + pl.point_offset(slot_id - SL_A); };
  const S beta_l = s.beta_g.pow_u64(ell), beta_l1 = beta_l * s.beta_g;
  s.z_ip = s.r_p * beta_l1 + s.gprod * beta_l - S::one();
  // inner_product_argument.rs:283-290, 202-250
  s.tr.append_point_bytes("ipa_step1", P(SL_C));
  s.tr.append_point_bytes("ipa_step1", d_comp);
  s.tr.append_scalar("ipa_step1", s.z_ip);
  s.tr.append_point_bytes("ipa_step1", P(SL_BC));
  s.tr.append_point_bytes("ipa_step1", P(SL_BD));
  s.alpha_i = s.tr.get_and_append_challenge("ipa_alpha");
  s.beta_i = s.tr.get_and_append_challenge("ipa_beta");
  s.gam_i.resize(L);
  for (size_t j = 0; j < L; j++) {
    int four[4];
    sm.ipa_round((int)j, four);
    for (int q : four) s.tr.append_point_bytes("ipa_loop", P(q));
    s.gam_i[j] = s.tr.get_and_append_challenge("ipa_gamma");
  }
  s.gam_i_inv = s.gam_i;
  batch_inverse(s.gam_i_inv);
  // same_scalar_argument.rs:112-128
  int sp[10];
  sm.sameexp_points(sp);
  for (int q : sp) s.tr.append_point_bytes("sameexp_points", P(q));
  s.alpha_s = s.tr.get_and_append_challenge("same_scalar_alpha");
  // same_multiscalar_argument.rs:229-233, 167-186
  s.tr.append_point_bytes("same_msm_step1", aprime_comp);
  s.tr.append_point_bytes("same_msm_step1", P(SL_CMT2));
  s.tr.append_point_bytes("same_msm_step1", P(SL_CMU2));
  {
    std::vector<uint8_t> vb(n * 48, 0);
    memcpy(vb.data(), ic + 2 * ell * 48, ell * 48);
    for (int i = 0; i < 4; i++) vb[(ell + i) * 48] = kCompIdentity;
    memcpy(&vb[(ell + 2) * 48], crs_h_comp, 48);
    s.tr.append_point_vec_bytes("same_msm_step1", vb.data(), n);
    std::fill(vb.begin() + ell * 48, vb.end(), 0);
    memcpy(vb.data(), ic + 3 * ell * 48, ell * 48);
    for (int i = 0; i < 4; i++) vb[(ell + i) * 48] = kCompIdentity;
    memcpy(&vb[(ell + 3) * 48], crs_h_comp, 48);
    s.tr.append_point_vec_bytes("same_msm_step1", vb.data(), n);
  }
  s.tr.append_point_bytes("same_msm_step1", P(sm.BA()));
  s.tr.append_point_bytes("same_msm_step1", P(sm.BT()));
  s.tr.append_point_bytes("same_msm_step1", P(sm.BU()));
  s.alpha_m = s.tr.get_and_append_challenge("same_msm_alpha");
  s.gam_m.resize(L);
  for (size_t j = 0; j < L; j++) {
    int six[6];
    sm.same_msm_round((int)j, six);
    for (int q : six) s.tr.append_point_bytes("same_msm_loop", P(q));
    s.gam_m[j] = s.tr.get_and_append_challenge("same_msm_gamma");
  }
  s.gam_m_inv = s.gam_m;
  batch_inverse(s.gam_m_inv);

  // verification scalars s_i = prod_{j : bit (L-1-j) of i set} gamma_j  (util.rs:40-64), built by doubling
  auto svec = [&](const SVec& g) {
    SVec sv(n);
    sv[0] = S::one();
    for (size_t j = 0; j < L; j++) {          // after step j, entries < 2^(j+1) are final for the low (j+1) bits
      const size_t w = size_t(1) << j;
      const S gj = g[L - 1 - j];              // bit j of i  <->  round L-1-j
      for (size_t i = 0; i < w; i++) sv[w + i] = sv[i] * gj;
    }
    return sv;
  };
  const SVec s_i = svec(s.gam_i), s_m = svec(s.gam_m);
  SVec s_i_inv = s_i;
  batch_inverse(s_i_inv);
  // u (grand_product_argument.rs:211-219)
  SVec u(n);
  {
    S pw = s.beta_g_inv;
    for (size_t i = 0; i < ell; i++) {
      u[i] = pw;
      pw *= s.beta_g_inv;
    }
    for (size_t i = ell; i < n; i++) u[i] = pw;
  }
  // ---- flattened accumulated check: one weight per point ----
  CheckTerms<S> t;
  t.alpha_sp = s.alpha_sp, t.beta_sp = s.beta_sp, t.alpha_g = s.alpha_g, t.beta_g_inv = s.beta_g_inv;
  t.alpha_i = s.alpha_i, t.beta_i = s.beta_i, t.alpha_s = s.alpha_s, t.alpha_m = s.alpha_m;
  t.c_fin = s.c_fin, t.d_fin = s.d_fin, t.z_k = s.z_k, t.z_t = s.z_t, t.z_u = s.z_u, t.x_fin = s.x_fin, t.z_ip = s.z_ip;
  t.gam_i = s.gam_i.data(), t.gam_i_inv = s.gam_i_inv.data(), t.gam_m = s.gam_m.data(), t.gam_m_inv = s.gam_m_inv.data();
  t.sm_l2 = s_m[ell + 2], t.sm_l3 = s_m[ell + 3];
  S f[VF_FUSED_COUNT];
  for (int i = 0; i < (fused ? VF_FUSED_COUNT : VF_COUNT); i++) f[i] = S_from_wire(factors + 32 * i);
  t.set_factors(f);
  t.set_same_scalar_weights(f, fused);
  SVec& k1 = s.scal[0];
  k1.resize(n);
  for (size_t i = 0; i < n; i++) k1[i] = crs_weight(t, (int)i, (int)ell, s_i[i], s_i_inv[i] * u[i], s_m[i]);
  SVec& k2 = s.scal[1];
  k2.resize(4 * ell);
  for (size_t i = 0; i < ell; i++) {
    S k[4];
    instance_weights(t, s.vec_a[i], s_m[i], k);
    for (int v = 0; v < 4; v++) k2[v * ell + i] = k[v];
  }
  SVec& k3 = s.scal[2];
  k3.resize((size_t)SL_A + pl.n_points());
  for (size_t slot = 0; slot < k3.size(); slot++) k3[slot] = misc_weight(t, sm, (int)slot);
}

}  // namespace host
}  // namespace cpx
