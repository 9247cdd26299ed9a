// TEST INFRASTRUCTURE: a shared library over oracle/protocol.h (read-only) for the tests of cpx_ipa_prove / cpx_same_msm_prove
// (tests/subarg_prove_lib.py builds it through check_harness.build_emul).
//   sp_inputs  from a seed the inputs of one stand-alone InnerProductProof::new / SameMultiscalarProof::new.  consistent = 0: an arbitrary
//              statement, drawn in the order tests/host_emul/subarg_oracle.cpp `sub_ipa` / `sub_samemsm` draw theirs (same seed, same
//              inputs), `pad` identities on the tail of G' / T / U as there.  consistent = 1: a statement the witness satisfies, as the
//              reference's own tests make one (inner_product_argument.rs:364-392, same_multiscalar_argument.rs:300-321): G' = u o G,
//              C = <c, G>, D = <d, G'>, z = <c, d> resp. A / Z_t / Z_u = <x, G / T / U>; with `pad` the last u are zero (G' ends in
//              identities) resp. the tails of T and U are identities.
//   sp_prove   the oracle's OWN ipa_new / samemsm_new on the caller's inputs and draws, on a transcript Transcript::new("subarg") + filler:
//              the serialised proof (inner_product_argument.rs:328-338, same_multiscalar_argument.rs:263-275), the state afterwards, and
//              the challenges — the latter from a second transcript driven call by call with the oracle's primitives on the proof's own
//              points, which must end in the same state.  Where the reference panics in generate_ipa_blinders (an inverse of zero,
//              inner_product_argument.rs:69, :71) the shim says so (status 1) without calling the prover: zero bytes, the state as it was.
// Wire forms as oracle/capi.cpp: Fr = 4 x u64 LE Montgomery, affine = x || y with zeros for the identity, Jacobian = X || Y || Z.
#include "../../oracle/protocol.h"

using namespace orc;

namespace {

enum { IPA = 0, SMSM = 1 };

G1Aff aff_from_wire(const uint8_t* b) {
  G1Aff p;
  memcpy(p.x.v, b, 48);
  memcpy(p.y.v, b + 48, 48);
  p.inf = p.x.is_zero() && p.y.is_zero();
  return p;
}
void aff_to_wire(const G1Aff& p, uint8_t* b) {
  if (p.inf) {
    memset(b, 0, 96);
    return;
  }
  memcpy(b, p.x.v, 48);
  memcpy(b + 48, p.y.v, 48);
}
G1 jac_from_wire(const uint8_t* b) {
  G1 p;
  memcpy(p.x.v, b, 48);
  memcpy(p.y.v, b + 48, 48);
  memcpy(p.z.v, b + 96, 48);
  return p;
}
void jac_to_wire(const G1& p, uint8_t* b) {
  memcpy(b, p.x.v, 48);
  memcpy(b + 48, p.y.v, 48);
  memcpy(b + 96, p.z.v, 48);
}
Fr fr_from_wire(const uint8_t* b) {
  Fr x;
  memcpy(x.v, b, 32);
  return x;
}
void fr_to_wire(const Fr& x, uint8_t* b) { memcpy(b, x.v, 32); }
std::vector<G1Aff> affs_from_wire(const uint8_t* b, size_t n) {
  std::vector<G1Aff> v(n);
  for (size_t i = 0; i < n; i++) v[i] = aff_from_wire(b + 96 * i);
  return v;
}
void affs_to_wire(const std::vector<G1Aff>& v, uint8_t* b) {
  for (size_t i = 0; i < v.size(); i++) aff_to_wire(v[i], b + 96 * i);
}
std::vector<Fr> frs_from_wire(const uint8_t* b, size_t n) {
  std::vector<Fr> v(n);
  for (size_t i = 0; i < n; i++) v[i] = fr_from_wire(b + 32 * i);
  return v;
}
void frs_to_wire(const std::vector<Fr>& v, uint8_t* b) {
  for (size_t i = 0; i < v.size(); i++) fr_to_wire(v[i], b + 32 * i);
}
void state_words(const Transcript& t, uint8_t out[216]) {
  uint64_t w[27];
  memcpy(w, t.strobe.state, 200);
  w[25] = t.strobe.pos;
  w[26] = t.strobe.pos_begin;
  memcpy(out, w, 216);
}
std::vector<G1Aff> rand_points(StdRng& rng, size_t n) {
  std::vector<G1Aff> v(n);
  for (auto& p : v) p = g1_to_affine(rand_g1(rng));
  return v;
}
std::vector<Fr> rand_scalars(StdRng& rng, size_t n) {
  std::vector<Fr> v(n);
  for (auto& x : v) x = rand_fr(rng);
  return v;
}
Transcript start(const uint8_t* filler, size_t filler_len) {
  Transcript t("subarg");
  if (filler_len) t.append_message("filler", filler, filler_len);
  return t;
}
struct Replayer {   // the given draws, in call order
  const uint8_t* buf;
  size_t n, pos = 0;
  bool overrun = false;
  Fr operator()() {
    if (pos >= n) {
      overrun = true;
      return Fr::one();
    }
    return fr_from_wire(buf + 32 * pos++);
  }
};

}  // namespace

extern "C" {

// bases: IPA G | G' [2 n]; SameMSM G | T | U [3 n].  stmt: crs_H, C, D resp. A, Z_t, Z_u (Jacobian, not normalised).  vecs: c | d resp. x.
// z_out, u_out: IPA only (u_out: consistent only, else zeros)
int sp_inputs(int kind, uint64_t seed, size_t n, int consistent, size_t pad, uint8_t* bases, uint8_t* stmt, uint8_t* z_out, uint8_t* vecs, uint8_t* u_out) {
  if (!n || (n & (n - 1)) || pad > n) return -1;
  StdRng in(seed);
  if (kind == IPA) {
    std::vector<G1Aff> G = rand_points(in, n), Gp;
    G1 crs_H, C, D;
    Fr z;
    std::vector<Fr> vec_c, vec_d, vec_u(n, Fr::zero());
    if (consistent) {
      vec_u = rand_scalars(in, n);
      for (size_t i = n - pad; i < n; i++) vec_u[i] = Fr::zero();
      Gp.resize(n);
      for (size_t i = 0; i < n; i++) Gp[i] = g1_to_affine(g1_mul(G1::from_affine(G[i]), vec_u[i]));
      crs_H = rand_g1(in);
      vec_c = rand_scalars(in, n);
      vec_d = rand_scalars(in, n);
      z = inner_product(vec_c, vec_d);
      C = g1_msm(G, vec_c);
      D = g1_msm(Gp, vec_d);
    } else {   // the order of sub_ipa
      Gp = rand_points(in, n);
      for (size_t i = n - pad; i < n; i++) Gp[i] = G1Aff::identity();
      crs_H = rand_g1(in);
      C = rand_g1(in);
      D = rand_g1(in);
      z = rand_fr(in);
      vec_c = rand_scalars(in, n);
      vec_d = rand_scalars(in, n);
    }
    affs_to_wire(G, bases);
    affs_to_wire(Gp, bases + 96 * n);
    jac_to_wire(crs_H, stmt);
    jac_to_wire(C, stmt + 144);
    jac_to_wire(D, stmt + 288);
    fr_to_wire(z, z_out);
    frs_to_wire(vec_c, vecs);
    frs_to_wire(vec_d, vecs + 32 * n);
    frs_to_wire(vec_u, u_out);
    return 0;
  }
  std::vector<G1Aff> G = rand_points(in, n), T = rand_points(in, n), U = rand_points(in, n);
  for (size_t i = n - pad; i < n; i++) {   // the tails of sub_samemsm (curdleproofs.rs:141-155: O O H O / O O O H)
    if (i != n - 2) T[i] = G1Aff::identity();
    if (i != n - 1) U[i] = G1Aff::identity();
  }
  G1 A, Z_t, Z_u;
  std::vector<Fr> vec_x;
  if (consistent) {
    vec_x = rand_scalars(in, n);
    A = g1_msm(G, vec_x);
    Z_t = g1_msm(T, vec_x);
    Z_u = g1_msm(U, vec_x);
  } else {
    A = rand_g1(in);
    Z_t = rand_g1(in);
    Z_u = rand_g1(in);
    vec_x = rand_scalars(in, n);
  }
  affs_to_wire(G, bases);
  affs_to_wire(T, bases + 96 * n);
  affs_to_wire(U, bases + 192 * n);
  jac_to_wire(A, stmt);
  jac_to_wire(Z_t, stmt + 144);
  jac_to_wire(Z_u, stmt + 288);
  frs_to_wire(vec_x, vecs);
  return 0;
}

// draws: IPA 2 n - 2 (r [n], then z [n - 2]), SameMSM n.  challenges: alpha, beta, gamma_1..L resp. alpha, gamma_1..L.
// status: 0 = a proof, 1 = the reference panics in generate_ipa_blinders (proof and challenges zero, state_out = the state before).
// Returns 0, or -1 for an argument the shim cannot take, -3 when the call-by-call transcript disagrees with the oracle's.
int sp_prove(int kind, size_t n, const uint8_t* filler, size_t filler_len, const uint8_t* bases, const uint8_t* stmt, const uint8_t* z_in, const uint8_t* vecs,
             const uint8_t* draws, size_t ndraws, uint8_t* proof, size_t* proof_len, uint8_t* challenges, uint8_t state_out[216], int* status) {
  if (!n || (n & (n - 1))) return -1;
  if (kind == IPA && n < 2) return -1;
  if (ndraws != (kind == IPA ? 2 * n - 2 : n)) return -1;
  size_t L = 0;
  while (((size_t)1 << L) < n) L++;
  const size_t nchal = (kind == IPA ? 2 : 1) + L, plen = 48 * ((kind == IPA ? 2 : 3) + (kind == IPA ? 4 : 6) * L) + (kind == IPA ? 64 : 32);
  Transcript transcript = start(filler, filler_len), again = transcript;
  Replayer rp{draws, ndraws};
  FrDraw draw = [&rp]() { return rp(); };
  std::vector<Fr> chal;
  ByteWriter w;
  *status = 0;
  *proof_len = plen;
  if (kind == IPA) {
    const std::vector<G1Aff> G = affs_from_wire(bases, n), Gp = affs_from_wire(bases + 96 * n, n);
    const G1 crs_H = jac_from_wire(stmt), C = jac_from_wire(stmt + 144), D = jac_from_wire(stmt + 288);
    const Fr z = fr_from_wire(z_in);
    const std::vector<Fr> c = frs_from_wire(vecs, n), d = frs_from_wire(vecs + 32 * n, n), r = frs_from_wire(draws, n);
    // inner_product_argument.rs:69 `c[n-2].inverse().unwrap()`, :71 the denominator's
    bool panics = c[n - 2].is_zero();
    if (!panics) panics = ((-r[n - 2]) * c[n - 2].inverse() * c[n - 1] + r[n - 1]).is_zero();
    if (panics) {
      *status = 1;
      memset(proof, 0, plen);
      memset(challenges, 0, 32 * nchal);
      state_words(transcript, state_out);
      return 0;
    }
    const InnerProductProof pf = ipa_new(G, Gp, crs_H, C, D, z, c, d, transcript, draw);
    w.g1(pf.B_c);
    w.g1(pf.B_d);
    w.g1v(pf.vec_L_C);
    w.g1v(pf.vec_R_C);
    w.g1v(pf.vec_L_D);
    w.g1v(pf.vec_R_D);
    w.fr(pf.c_final);
    w.fr(pf.d_final);
    again.append_g1("ipa_step1", C);
    again.append_g1("ipa_step1", D);
    again.append_fr("ipa_step1", z);
    again.append_g1("ipa_step1", pf.B_c);
    again.append_g1("ipa_step1", pf.B_d);
    chal.push_back(again.get_and_append_challenge("ipa_alpha"));
    chal.push_back(again.get_and_append_challenge("ipa_beta"));
    for (size_t j = 0; j < L; j++) {
      again.append_g1("ipa_loop", pf.vec_L_C[j]);
      again.append_g1("ipa_loop", pf.vec_L_D[j]);
      again.append_g1("ipa_loop", pf.vec_R_C[j]);
      again.append_g1("ipa_loop", pf.vec_R_D[j]);
      chal.push_back(again.get_and_append_challenge("ipa_gamma"));
    }
  } else {
    const std::vector<G1Aff> G = affs_from_wire(bases, n), T = affs_from_wire(bases + 96 * n, n), U = affs_from_wire(bases + 192 * n, n);
    const G1 A = jac_from_wire(stmt), Z_t = jac_from_wire(stmt + 144), Z_u = jac_from_wire(stmt + 288);
    const std::vector<Fr> x = frs_from_wire(vecs, n);
    const SameMultiscalarProof pf = samemsm_new(G, A, Z_t, Z_u, T, U, x, transcript, draw);
    w.g1(pf.B_a);
    w.g1(pf.B_t);
    w.g1(pf.B_u);
    w.g1v(pf.vec_L_A);
    w.g1v(pf.vec_L_T);
    w.g1v(pf.vec_L_U);
    w.g1v(pf.vec_R_A);
    w.g1v(pf.vec_R_T);
    w.g1v(pf.vec_R_U);
    w.fr(pf.x_final);
    again.append_g1("same_msm_step1", A);
    again.append_g1("same_msm_step1", Z_t);
    again.append_g1("same_msm_step1", Z_u);
    again.append_g1_vec("same_msm_step1", T);
    again.append_g1_vec("same_msm_step1", U);
    again.append_g1("same_msm_step1", pf.B_a);
    again.append_g1("same_msm_step1", pf.B_t);
    again.append_g1("same_msm_step1", pf.B_u);
    chal.push_back(again.get_and_append_challenge("same_msm_alpha"));
    for (size_t j = 0; j < L; j++) {
      const G1* six[6] = {&pf.vec_L_A[j], &pf.vec_L_T[j], &pf.vec_L_U[j], &pf.vec_R_A[j], &pf.vec_R_T[j], &pf.vec_R_U[j]};
      for (auto p : six) again.append_g1("same_msm_loop", *p);
      chal.push_back(again.get_and_append_challenge("same_msm_gamma"));
    }
  }
  if (rp.overrun || rp.pos != rp.n || w.b.size() != plen || chal.size() != nchal) return -1;
  uint8_t other[216];
  state_words(transcript, state_out);
  state_words(again, other);
  if (memcmp(state_out, other, 216) != 0) return -3;
  memcpy(proof, w.b.data(), plen);
  for (size_t i = 0; i < nchal; i++) fr_to_wire(chal[i], challenges + 32 * i);
  return 0;
}

}  // extern "C"
