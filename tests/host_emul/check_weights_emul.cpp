// TEST-ONLY: the host verifier's transcript and scalar work (curdleproofs_amd/csrc/host_verify.hpp) and the weights of the accumulated
// check (check_weights.hpp) compiled for the CPU, the latter in both instantiations: over host::S as the host-driven path runs it, and
// over Fr — the device's scalar type — with the per-index s_i of k_vs_scalars (protocol.hip).  Scalars cross in wire form (32 bytes).
#include <cstring>
#include "../../curdleproofs_amd/csrc/host_verify.hpp"

using namespace cpx;
using host::S;

extern "C" {

void* cw_new() { return new host::VerifyState(); }
void cw_free(void* st) { delete static_cast<host::VerifyState*>(st); }

// layout.hpp as the tests need it
int cw_n_points(int L) { return ProofLayout(L).n_points(); }
int cw_n_slots(int L) { return SL_A + ProofLayout(L).n_points(); }
size_t cw_proof_size(int L) { return ProofLayout(L).size(); }
size_t cw_point_offset(int L, int slot) { return ProofLayout(L).point_offset(slot - SL_A); }
size_t cw_scalar_offset(int L, int i) { return ProofLayout(L).scalar_offset(i); }

// V1a.  d_scal: the three scalars of D = 1 . B - beta^-1 . sum(G) + alpha . sum(H).  Returns bad | reject << 1.
int cw_prefix(void* st, size_t ell, size_t L, const uint8_t* pb, const uint8_t* ic, const uint8_t* mcomp, uint8_t* d_scal) {
  host::VerifyState& s = *static_cast<host::VerifyState*>(st);
  host::verify_prefix(s, ell, L, pb, ic, mcomp);
  memcpy(d_scal, s.scal[0].data(), 3 * 32);
  return (s.bad ? 1 : 0) | (s.reject ? 2 : 0);
}

// V1c.  k1 [n], k2 [4 ell], k3 [cw_n_slots]: the weights as the host-driven path stages them
void cw_scalars(void* st, size_t ell, size_t L, const uint8_t* ic, const uint8_t* crs_h_comp, const uint8_t* d_comp, const uint8_t* aprime_comp, const uint8_t* factors,
                int fused, uint8_t* k1, uint8_t* k2, uint8_t* k3) {
  host::VerifyState& s = *static_cast<host::VerifyState*>(st);
  host::verify_scalars(s, ell, L, ic, crs_h_comp, d_comp, aprime_comp, factors, fused != 0);
  memcpy(k1, s.scal[0].data(), s.scal[0].size() * 32);
  memcpy(k2, s.scal[1].data(), s.scal[1].size() * 32);
  memcpy(k3, s.scal[2].data(), s.scal[2].size() * 32);
}

// The same three arrays from CheckTerms<Fr>, driven the way k_vs_scalars drives it: the challenges of `st` (after cw_scalars), every
// s_i from its index.
void cw_scalars_fr(void* st, size_t ell_, size_t L_, const uint8_t* factors, int fused, uint8_t* k1, uint8_t* k2, uint8_t* k3) {
  const host::VerifyState& s = *static_cast<host::VerifyState*>(st);
  const int ell = (int)ell_, L = (int)L_, n = ell + 4;
  const SlotMap sm(L);
  std::vector<Fr> gam(4 * L), u(ell + 1), f(VF_FUSED_COUNT, Fr::zero());
  for (int j = 0; j < L; j++) gam[j] = s.gam_i[j].f, gam[L + j] = s.gam_m[j].f, gam[2 * L + j] = s.gam_i_inv[j].f, gam[3 * L + j] = s.gam_m_inv[j].f;
  u[0] = s.beta_g_inv.f;
  for (int i = 1; i <= ell; i++) u[i] = fe_mul(u[i - 1], s.beta_g_inv.f);
  for (int i = 0; i < (fused ? VF_FUSED_COUNT : VF_COUNT); i++) memcpy(f[i].v, factors + 32 * i, 32);
  CheckTerms<Fr> w;
  w.alpha_sp = s.alpha_sp.f, w.beta_sp = s.beta_sp.f, w.alpha_g = s.alpha_g.f, w.beta_g_inv = s.beta_g_inv.f;
  w.alpha_i = s.alpha_i.f, w.beta_i = s.beta_i.f, w.alpha_s = s.alpha_s.f, w.alpha_m = s.alpha_m.f;
  w.c_fin = s.c_fin.f, w.d_fin = s.d_fin.f, w.z_k = s.z_k.f, w.z_t = s.z_t.f, w.z_u = s.z_u.f, w.x_fin = s.x_fin.f, w.z_ip = s.z_ip.f;
  w.gam_i = gam.data(), w.gam_m = gam.data() + L, w.gam_i_inv = gam.data() + 2 * L, w.gam_m_inv = gam.data() + 3 * L;
  w.set_factors(f.data());
  auto svec = [&](const Fr* g, int i) {
    Fr r = Fr::one();
    for (int j = 0; j < L; j++)
      if ((i >> (L - 1 - j)) & 1) r = fe_mul(r, g[j]);
    return r;
  };
  Fr* o1 = reinterpret_cast<Fr*>(k1);
  Fr* o2 = reinterpret_cast<Fr*>(k2);
  Fr* o3 = reinterpret_cast<Fr*>(k3);
  for (int i = 0; i < n; i++) {
    const Fr s_i = svec(w.gam_i, i), s_i_inv = svec(w.gam_i_inv, i), s_m = svec(w.gam_m, i);
    o1[i] = crs_weight(w, i, ell, s_i, fe_mul(s_i_inv, u[i < ell ? i : ell]), s_m);
    if (i < ell) {
      Fr k[4];
      instance_weights(w, s.vec_a[i].f, s_m, k);
      for (int q = 0; q < 4; q++) o2[q * ell + i] = k[q];
    }
    if (i == ell + 2) w.sm_l2 = s_m;
    if (i == ell + 3) w.sm_l3 = s_m;
  }
  w.set_same_scalar_weights(f.data(), fused != 0);
  for (int slot = 0; slot < SL_A + ProofLayout(L).n_points(); slot++) o3[slot] = misc_weight(w, sm, slot);
}

}  // extern "C"
