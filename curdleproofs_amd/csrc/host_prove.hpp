// The host-driven prover's per-proof work that needs no GPU: the Fiat-Shamir transcript of CurdleproofsProof::new (host_transcript.hpp)
// and the scalar-field algebra between two device phases, one function per block.  Engine::batch_prove_tables (engine.cpp) launches and
// waits around these steps, stages the scalars they leave in ProveState for the requests of prove_reqs.hpp and hands each step the
// compressed results of the phase before it (take); the device-resident path does the same work in the k_ps_* kernels (protocol.hip).
// Scalars arrive in wire form (Montgomery residues, 32 bytes) and leave as Fr rows the caller owns.  No HIP: the tests compile this for
// the CPU (tests/test_host_prove_cpu.py).
#pragma once
#include "host_transcript.hpp"
#include "prove_reqs.hpp"

namespace cpx {
namespace host {

struct ProveState {
  Transcript tr{"curdleproofs"};
  // the scalars under the names the device-resident prover keeps them by (protocol.h, layout.hpp): the RandIdx row, the vectors V_*
  // (V_FACT: its first ell entries — the host-driven B is a sum of points, not the commitment form that reads the blinder entries),
  // the small scalars SC_*
  SVec rnd;
  SVec vec[V_COUNT];
  S sc[SC_COUNT];
  S k;
  SVec vec_a, rb_plus_alpha;
  std::vector<uint8_t> comp;        // compressed bytes of every slot (count * 48)
  const uint8_t* operator()(int slot) const { return &comp[(size_t)slot * 48]; }   // the `slot` of host_transcript.hpp
};

// the compressed results of a phase (this proof's, in request order) into the slots its requests name
inline void take(ProveState& s, const ReqList& l, const uint8_t* results) {
  for (int i = 0; i < l.n; i++)
    if (l.r[i].out >= 0) memcpy(&s.comp[(size_t)l.r[i].out * 48], results + (size_t)i * 48, 48);
}
// ... and the slots `q` out of a window of consecutive compressed slots that starts at slot `first`
inline void take(ProveState& s, const int* q, int nq, const uint8_t* window, int first) {
  for (int i = 0; i < nq; i++) memcpy(&s.comp[(size_t)q[i] * 48], window + (size_t)(q[i] - first) * 48, 48);
}

// Before phase 1.  rand: the proof's RandIdx row, k: its scalar (wire form); perm: its permutation; ic: its compressed instance rows
// R | S | T | U; mcomp: its compressed M.
inline void prove_begin(ProveState& s, size_t ell, size_t L, const uint8_t* rand, const uint8_t* k, const uint32_t* perm, const uint8_t* ic, const uint8_t* mcomp) {
  const size_t n = ell + N_BLINDERS;
  const RandIdx ri((int)n);
  s.rnd.resize((size_t)ri.count());
  for (size_t i = 0; i < s.rnd.size(); i++) s.rnd[i] = S_from_wire(rand + i * 32);
  s.k = S_from_wire(k);
  s.comp.assign((size_t)SlotMap(L).count() * 48, 0);
  memcpy(&s.comp[SL_M * 48], mcomp, 48);
  s.vec_a = absorb_instance(s.tr, ell, ic, mcomp);
  // the scalars of A: vec_a permuted, then the two vec_a_blinders and two zeros (curdleproofs.rs:85-93)
  SVec& ap = s.vec[V_APERM];
  ap.resize(n);
  for (size_t i = 0; i < ell; i++) ap[i] = s.vec_a[perm[i]];
  for (size_t i = 0; i < N_BLINDERS; i++) ap[ell + i] = i < 2 ? s.rnd[ri.AB() + i] : S::zero();
}

// The scalars of the side stream's six MSMs over vec_R / vec_S: a for R, S (curdleproofs.rs:112-113), k a for k R, k S (115-116),
// r_k a for r_k R, r_k S (same_scalar_argument.rs:60-61); ell entries each.
inline void prove_side_scalars(const ProveState& s, size_t ell, Fr* a, Fr* ka, Fr* rka) {
  const S r_k = s.rnd[RandIdx((int)(ell + N_BLINDERS)).RK()];
  for (size_t i = 0; i < ell; i++) {
    a[i] = s.vec_a[i].f;
    ka[i] = (s.vec_a[i] * s.k).f;
    rka[i] = (s.vec_a[i] * r_k).f;
  }
}

// After phase 1 (A): same_permutation_argument.rs:60-83, and the partial products c of grand_product_argument.rs:66-75 — they need
// the factors only, so C joins the phase of B and A'.
// (B = A + alpha M + beta * sum(G) (same_permutation_argument.rs:75-76): the point A of phase 1 plus two single-point terms with the
// scalars beta, alpha — G_sum sits in the CRS tables)
inline void prove_after_phase1(ProveState& s, size_t ell, const uint32_t* perm) {
  const RandIdx ri((int)(ell + N_BLINDERS));
  same_perm_challenges(s.tr, s, s.vec_a, &s.sc[SC_ALPHA_SP], &s.sc[SC_BETA_SP]);
  s.vec[V_FACT].resize(ell);
  s.sc[SC_GPROD] = S::one();
  for (size_t i = 0; i < ell; i++) {
    s.vec[V_FACT][i] = s.vec[V_APERM][i] + S::from_u64(perm[i]) * s.sc[SC_ALPHA_SP] + s.sc[SC_BETA_SP];
    s.sc[SC_GPROD] *= s.vec[V_FACT][i];
  }
  SVec& c = s.vec[V_C];
  c.assign(1, S::one());
  for (size_t i = 0; i + 1 < ell; i++) c.push_back(c[i] * s.vec[V_FACT][i]);
  c.insert(c.end(), &s.rnd[ri.CB()], &s.rnd[ri.CB()] + N_BLINDERS);   // vec_c_blinders
}

// After phase 2 (B, A', C): the grand-product argument up to the vectors of its inner-product argument.  The transcript takes B, draws
// alpha, then takes C: an order of hashing, not of computing.  m_blinders: the proof's four vec_m_blinders (wire form).
inline void prove_after_phase2(ProveState& s, size_t ell, const uint8_t* m_blinders) {
  const size_t n = ell + N_BLINDERS;
  const RandIdx ri((int)n);
  s.sc[SC_ALPHA_G] = gprod_step1(s.tr, s, s.sc[SC_GPROD]);
  const S* ab = &s.vec[V_APERM][ell];   // vec_a_blinders | 0 0
  s.rb_plus_alpha.resize(N_BLINDERS);   // grand_product_argument.rs:79-81 over the vec_b_blinders of same_permutation_argument.rs:78-81
  for (size_t i = 0; i < N_BLINDERS; i++) s.rb_plus_alpha[i] = (ab[i] + s.sc[SC_ALPHA_SP] * S_from_wire(m_blinders + i * 32)) + s.sc[SC_ALPHA_G];
  s.sc[SC_RP] = inner_product(s.rb_plus_alpha.data(), &s.rnd[ri.CB()], N_BLINDERS);
  const S beta = s.sc[SC_BETA_G] = gprod_step2(s.tr, s, s.sc[SC_RP]);
  s.sc[SC_BETA_G_INV] = beta.inverse();
  s.vec[V_U].resize(n);
  u_powers(s.sc[SC_BETA_G_INV], ell, s.vec[V_U].data());
  S beta_l1;
  s.sc[SC_ZIP] = gprod_inner_product(s.sc[SC_RP], s.sc[SC_GPROD], beta, ell, &beta_l1);
  SVec& d = s.vec[V_D];   // grand_product_argument.rs:104-126
  d.resize(n);
  S pb = beta, pbm = S::one();
  for (size_t i = 0; i < ell; i++) {
    d[i] = s.vec[V_FACT][i] * pb - pbm;
    pbm = pb;
    pb *= beta;
  }
  for (size_t i = 0; i < N_BLINDERS; i++) d[ell + i] = beta_l1 * s.rb_plus_alpha[i];
  // D = B - beta^-1 sum(G) + alpha sum(Hvec) (grand_product_argument.rs:132): the point B plus two single-point terms
  s.sc[SC_NEG_BETA_G_INV] = -s.sc[SC_BETA_G_INV];
  // generate_ipa_blinders (inner_product_argument.rs:42-82): r_c = the IR draws, r_d = the IZ draws with its last two entries solved for
  const S* r = &s.rnd[ri.IR()];
  const SVec& c = s.vec[V_C];
  SVec& zz = s.vec[V_ZZ];
  zz.assign(&s.rnd[ri.IZ()], &s.rnd[ri.IZ()] + n - 2);
  zz.resize(n);
  const S omega = inner_product(r, d.data(), n) + inner_product(zz.data(), c.data(), n - 2);
  const S delta = inner_product(r, zz.data(), n - 2);
  const S inv_c = c[n - 2].inverse();
  const S last_z = (r[n - 2] * inv_c * omega - delta) * ((-r[n - 2]) * inv_c * c[n - 1] + r[n - 1]).inverse();
  zz[n - 2] = (-inv_c) * (last_z * c[n - 1] + omega);
  zz[n - 1] = last_z;
  s.vec[V_ZZU].resize(n);                             // B_d = msm(G', r_d) = msm(G, r_d o u)
  for (size_t i = 0; i < n; i++) s.vec[V_ZZU][i] = zz[i] * s.vec[V_U][i];
}

// After phase 3 (D, B_d): the round vectors of the inner-product argument, which live on the device from here on: row = c | d | S_G |
// S_G' (4 n entries; inner_product_argument.rs:129-148; the fold coefficients start at 1 and at u), and the argument's beta.
inline void prove_ipa_setup(ProveState& s, size_t ell, size_t L, Fr* row, Fr* beta) {
  const size_t n = ell + N_BLINDERS;
  const RandIdx ri((int)n);
  ipa_step1(s.tr, SlotMap(L), s, s.sc[SC_ZIP], &s.sc[SC_ALPHA_I], &s.sc[SC_BETA_I]);
  for (size_t i = 0; i < n; i++) {
    row[i] = (s.rnd[ri.IR() + i] + s.sc[SC_ALPHA_I] * s.vec[V_C][i]).f;
    row[n + i] = (s.vec[V_ZZ][i] + s.sc[SC_ALPHA_I] * s.vec[V_D][i]).f;
    row[2 * n + i] = S::one().f;
    row[3 * n + i] = s.vec[V_U][i].f;
  }
  *beta = s.sc[SC_BETA_I].f;
}

// After the MSMs of round j: the host hashes the round's points and returns gamma, gamma^-1 for the device's folds.
inline void prove_ipa_round(ProveState& s, size_t L, int j, Fr gamma[2]) {
  const S g = ipa_round_gamma(s.tr, SlotMap(L), j, s);
  gamma[0] = g.f;
  gamma[1] = g.inverse().f;
}
inline void prove_smsm_round(ProveState& s, size_t L, int j, Fr gamma[2]) {
  const S g = smsm_round_gamma(s.tr, SlotMap(L), j, s);
  gamma[0] = g.f;
  gamma[1] = g.inverse().f;
}

// After the last IPA round and the side and table streams (R, S, the T_2 commitments, B_t, B_u): c_final, d_final = c[0], d[0] after the
// last fold (inner_product_argument.rs:188-195), the SameScalar responses (same_scalar_argument.rs:63-75), SameMSM step 1 and its round
// vectors: row = x | S_M (2 n entries) — the witness x = vec_r + alpha (a_sigma | a_blinders 0 0) with r_t, r_u on the last two bases
// (same_multiscalar_argument.rs:93-95, curdleproofs.rs:136-143) and the fold coefficients, which start at 1.
inline void prove_smsm_setup(ProveState& s, size_t ell, size_t L, const Fr& c_final, const Fr& d_final, const uint8_t* ic, const uint8_t* crs_h_comp, Fr* row) {
  const size_t n = ell + N_BLINDERS;
  const RandIdx ri((int)n);
  const SlotMap sm(L);
  s.sc[SC_CFIN] = S(c_final);
  s.sc[SC_DFIN] = S(d_final);
  const S alpha = s.sc[SC_ALPHA_S] = same_scalar_alpha(s.tr, sm, s);
  s.sc[SC_ZK] = s.rnd[ri.RK()] + s.k * alpha;
  s.sc[SC_ZT] = s.rnd[ri.RA()] + s.rnd[ri.RT()] * alpha;
  s.sc[SC_ZU] = s.rnd[ri.RB()] + s.rnd[ri.RU()] * alpha;
  s.sc[SC_ALPHA_M] = same_msm_step1(s.tr, sm, s, ell, ic, crs_h_comp);
  for (size_t i = 0; i < n; i++) {
    const S& w = i + 2 < n ? s.vec[V_APERM][i] : s.rnd[i + 2 == n ? ri.RT() : ri.RU()];
    row[i] = (s.rnd[ri.VR() + i] + s.sc[SC_ALPHA_M] * w).f;
    row[n + i] = S::one().f;
  }
}

// After the last SameMSM round: x_final = x[0] after the last fold (same_multiscalar_argument.rs:138-141), and the proof's bytes.
inline void prove_serialize(ProveState& s, size_t L, const Fr& x_final, uint8_t* out) {
  const ProofLayout pl(L);
  s.sc[SC_XFIN] = S(x_final);
  for (int q = 0; q < pl.n_points(); q++) memcpy(out + pl.point_offset(q), s(SL_A + q), 48);
  const int vals[ProofLayout::N_SCALARS] = {SC_RP, SC_CFIN, SC_DFIN, SC_ZK, SC_ZT, SC_ZU, SC_XFIN};
  for (int i = 0; i < ProofLayout::N_SCALARS; i++) s.sc[vals[i]].to_le_bytes(out + pl.scalar_offset(i));
}

}  // namespace host
}  // namespace cpx
