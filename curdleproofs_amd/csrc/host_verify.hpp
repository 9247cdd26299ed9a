// The host-driven verifier's per-proof work that needs no GPU: deserialising the proof's scalars, the Fiat-Shamir transcript and the
// scalars of the accumulated check.  Engine::verify_core (engine.cpp) launches and waits around these two steps and stages the scalars
// (VerifyState::scal) in the layout of check_plan.hpp, the same for every mode of the check; the device-resident path does the same
// work in k_vs_prefix / k_vs_scalars (protocol.hip).  No HIP: the tests compile this for the CPU.
#pragma once
#include "check_weights.hpp"
#include "host_transcript.hpp"

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

// the 48 bytes of a slot as the verifier has them: M, a proof point, or one of the two points it computed, D and A'
struct VerifySlots {
  const uint8_t* pb;
  ProofLayout pl;
  SlotMap sm;
  const uint8_t *mcomp, *d_comp, *aprime_comp;
  const uint8_t* operator()(int q) const { return q == SL_M ? mcomp : q == sm.D() ? d_comp : q == sm.APRIME() ? aprime_comp : pb + pl.point_offset(q - SL_A); }
};

// V1a: the proof's scalars, the transcript up to the grand-product beta, the scalars of D.
// pb: the proof; ic: the compressed instance rows R | S | T | U (ell points each); mcomp: the compressed M.
inline void verify_prefix(VerifyState& s, size_t ell, size_t L, const uint8_t* pb, const uint8_t* ic, const uint8_t* mcomp) {
  const ProofLayout pl(L);
  s.pb = pb;
  const VerifySlots P{pb, pl, SlotMap(L), mcomp, nullptr, nullptr};
  S* vals[ProofLayout::N_SCALARS] = {&s.r_p, &s.c_fin, &s.d_fin, &s.z_k, &s.z_t, &s.z_u, &s.x_fin};
  for (int i = 0; i < ProofLayout::N_SCALARS; i++)
    if (!S::from_le_bytes(pb + pl.scalar_offset(i), vals[i])) s.bad = true;
  // curdleproofs.rs:218: the randomiser must not have wiped the ciphertexts
  if (ic[2 * ell * 48] == kCompIdentity) s.reject = true;
  s.vec_a = absorb_instance(s.tr, ell, ic, mcomp);
  same_perm_challenges(s.tr, P, s.vec_a, &s.alpha_sp, &s.beta_sp);
  s.gprod = S::one();   // same_permutation_argument.rs:139-145
  for (size_t i = 0; i < ell; i++) s.gprod *= s.vec_a[i] + S::from_u64(i) * s.alpha_sp + s.beta_sp;
  s.alpha_g = gprod_step1(s.tr, P, s.gprod);
  s.beta_g = gprod_step2(s.tr, P, s.r_p);
  s.beta_g_inv = s.beta_g.inverse();
  s.scal[0] = {S::one(), -s.beta_g_inv, s.alpha_g};    // D = B - beta^-1 sum(G) + alpha sum(H)  (grand_product_argument.rs:223)
}

// V1c: the rest of the transcript and the weights of the accumulated check (check_weights.hpp).
// crs_h_comp: the compressed H of the CRS; d_comp, aprime_comp: D and A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.rs:258) compressed;
// factors: the proof's random factors in wire form, VF_FUSED_COUNT of them for a fused batch, else VF_COUNT.
inline void verify_scalars(VerifyState& s, size_t ell, size_t L, const uint8_t* ic, const uint8_t* crs_h_comp, const uint8_t* d_comp, const uint8_t* aprime_comp,
                           const uint8_t* factors, bool fused) {
  const size_t n = ell + N_BLINDERS;
  const SlotMap sm(L);
  const ProofLayout pl(L);
  const VerifySlots P{s.pb, pl, sm, nullptr, d_comp, aprime_comp};
  S beta_l1;
  s.z_ip = gprod_inner_product(s.r_p, s.gprod, s.beta_g, ell, &beta_l1);
  ipa_step1(s.tr, sm, P, s.z_ip, &s.alpha_i, &s.beta_i);
  s.gam_i.resize(L);
  for (size_t j = 0; j < L; j++) s.gam_i[j] = ipa_round_gamma(s.tr, sm, (int)j, P);
  s.gam_i_inv = s.gam_i;
  batch_inverse(s.gam_i_inv);
  s.alpha_s = same_scalar_alpha(s.tr, sm, P);
  s.alpha_m = same_msm_step1(s.tr, sm, P, ell, ic, crs_h_comp);
  s.gam_m.resize(L);
  for (size_t j = 0; j < L; j++) s.gam_m[j] = smsm_round_gamma(s.tr, sm, (int)j, P);
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
  SVec u(n);
  u_powers(s.beta_g_inv, ell, u.data());
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
