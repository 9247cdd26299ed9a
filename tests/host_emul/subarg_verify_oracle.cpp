// TEST INFRASTRUCTURE: a shared library over oracle/protocol.h (read-only) for the tests of cpx_ipa_verify / cpx_same_msm_verify
// (tests/subarg_verify_lib.py builds it through check_harness.build_emul).
//   sv_make    from a seed a CONSISTENT statement, as the reference's own tests make one (inner_product_argument.rs:364-392,
//              same_multiscalar_argument.rs:300-321): G' = u o G, C = <c, G>, D = <d, G'>, z = <c, d> resp. A / Z_t / Z_u = <x, G / T / U>,
//              and the oracle's own ipa_new / samemsm_new on it, serialised (inner_product_argument.rs:328-338,
//              same_multiscalar_argument.rs:263-275).  The oracle's blinder generator needs n >= 2 for the IPA; the one proof that n = 1
//              admits is built by hand: zero blinders, so B_c = B_d = O and the finals are alpha c, alpha d.
//   sv_entry   for the same statement what stands at the entry of the prover's log-round loop (the inputs of cpx_ipa_rounds /
//              cpx_same_msm_rounds), so that a proof can be assembled from that call's outputs.
//   sv_verify  deserialises proof bytes as the reference does before it can call `verify`, then runs the oracle's OWN ipa_verify /
//              samemsm_verify on a fresh transcript and a fresh MsmAccumulator with the given draws, and reports the accumulator's verdict,
//              the state afterwards and the challenges — the latter from a second transcript driven call by call with the oracle's
//              primitives, which must end in the same state.  The inputs are the caller's, so a test can change any of them.
// A filler message ahead moves the rate position (tests/host_emul/subarg_oracle.cpp `sub_state` gives the state before `verify`).
// Wire forms as oracle/capi.cpp: Fr = 4 x u64 LE Montgomery, affine = x || y with zeros for the identity, Jacobian = X || Y || Z.
#include "../../oracle/protocol.h"

using namespace orc;

namespace {

enum { IPA = 0, SMSM = 1 };
enum { SV_OK = 0, SV_ERR_VERIFY = -4, SV_ERR_DESERIALIZE = -5 };   // include/cpx.h CPX_OK, CPX_ERR_VERIFY, CPX_ERR_DESERIALIZE

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
size_t log2_of(size_t n) {
  size_t L = 0;
  while (((size_t)1 << L) < n) L++;
  return L;
}
std::vector<uint8_t> serialize(const InnerProductProof& pf) {   // inner_product_argument.rs:328-338
  ByteWriter w;
  w.g1(pf.B_c);
  w.g1(pf.B_d);
  w.g1v(pf.vec_L_C);
  w.g1v(pf.vec_R_C);
  w.g1v(pf.vec_L_D);
  w.g1v(pf.vec_R_D);
  w.fr(pf.c_final);
  w.fr(pf.d_final);
  return w.b;
}
std::vector<uint8_t> serialize(const SameMultiscalarProof& pf) {   // same_multiscalar_argument.rs:263-275
  ByteWriter w;
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
  return w.b;
}
bool deserialize(const uint8_t* b, size_t len, size_t L, InnerProductProof* pf) {   // inner_product_argument.rs:340-352
  ByteReader r{b, len};
  pf->B_c = r.g1();
  pf->B_d = r.g1();
  pf->vec_L_C = r.g1v(L);
  pf->vec_R_C = r.g1v(L);
  pf->vec_L_D = r.g1v(L);
  pf->vec_R_D = r.g1v(L);
  pf->c_final = r.fr();
  pf->d_final = r.fr();
  return r.ok && r.left == 0;
}
bool deserialize(const uint8_t* b, size_t len, size_t L, SameMultiscalarProof* pf) {   // same_multiscalar_argument.rs:276-290
  ByteReader r{b, len};
  pf->B_a = r.g1();
  pf->B_t = r.g1();
  pf->B_u = r.g1();
  pf->vec_L_A = r.g1v(L);
  pf->vec_L_T = r.g1v(L);
  pf->vec_L_U = r.g1v(L);
  pf->vec_R_A = r.g1v(L);
  pf->vec_R_T = r.g1v(L);
  pf->vec_R_U = r.g1v(L);
  pf->x_final = r.fr();
  return r.ok && r.left == 0;
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

// bases: IPA G [n]; SameMSM G | T | U [3 n].  stmt: crs_H, C, D resp. A, Z_t, Z_u (Jacobian, not normalised).  z, vec_u: IPA only
int sv_make(int kind, uint64_t seed, size_t n, const uint8_t* filler, size_t filler_len, uint8_t* bases, uint8_t* stmt, uint8_t* z_out, uint8_t* u_out, uint8_t* proof,
            size_t* proof_len) {
  if (!n || (n & (n - 1))) return -1;
  StdRng in(seed);
  StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
  FrDraw draw = [&rng]() { return rand_fr(rng); };
  Transcript transcript = start(filler, filler_len);
  std::vector<uint8_t> bytes;
  if (kind == IPA) {
    std::vector<G1Aff> G = rand_points(in, n), Gp(n);
    std::vector<Fr> vec_u = rand_scalars(in, n);
    for (size_t i = 0; i < n; i++) Gp[i] = g1_to_affine(g1_mul(G1::from_affine(G[i]), vec_u[i]));
    const G1 crs_H = rand_g1(in);
    std::vector<Fr> vec_c = rand_scalars(in, n), vec_d = rand_scalars(in, n);
    const Fr z = inner_product(vec_c, vec_d);
    const G1 C = g1_msm(G, vec_c), D = g1_msm(Gp, vec_d);
    InnerProductProof pf;
    if (n >= 2) {
      pf = ipa_new(G, Gp, crs_H, C, D, z, vec_c, vec_d, transcript, draw);
    } else {   // zero blinders: ipa_new :183-197 with vec_r_c = vec_r_d = 0
      pf.B_c = G1::identity();
      pf.B_d = G1::identity();
      transcript.append_g1("ipa_step1", C);
      transcript.append_g1("ipa_step1", D);
      transcript.append_fr("ipa_step1", z);
      transcript.append_g1("ipa_step1", pf.B_c);
      transcript.append_g1("ipa_step1", pf.B_d);
      const Fr alpha = transcript.get_and_append_challenge("ipa_alpha");
      pf.c_final = alpha * vec_c[0];
      pf.d_final = alpha * vec_d[0];
    }
    affs_to_wire(G, bases);
    jac_to_wire(crs_H, stmt);
    jac_to_wire(C, stmt + 144);
    jac_to_wire(D, stmt + 288);
    fr_to_wire(z, z_out);
    for (size_t i = 0; i < n; i++) fr_to_wire(vec_u[i], u_out + 32 * i);
    bytes = serialize(pf);
  } else {
    std::vector<G1Aff> G = rand_points(in, n), T = rand_points(in, n), U = rand_points(in, n);
    std::vector<Fr> vec_x = rand_scalars(in, n);
    const G1 A = g1_msm(G, vec_x), Z_t = g1_msm(T, vec_x), Z_u = g1_msm(U, vec_x);
    const SameMultiscalarProof pf = samemsm_new(G, A, Z_t, Z_u, T, U, vec_x, transcript, draw);
    affs_to_wire(G, bases);
    affs_to_wire(T, bases + 96 * n);
    affs_to_wire(U, bases + 192 * n);
    jac_to_wire(A, stmt);
    jac_to_wire(Z_t, stmt + 144);
    jac_to_wire(Z_u, stmt + 288);
    bytes = serialize(pf);
  }
  memcpy(proof, bytes.data(), bytes.size());
  *proof_len = bytes.size();
  return 0;
}

// What stands at the entry of the prover's log-round loop for the statement sv_make(kind, seed, n, filler) makes (n >= 2), the steps before
// the loop with the oracle's primitives (protocol.h ipa_new :181-198, samemsm_new :526-541, as tests/host_emul/subarg_oracle.cpp restates
// them): the inputs of cpx_ipa_rounds / cpx_same_msm_rounds.  fam2: IPA G' [n] | H [1]; unused for SameMSM (T, U are sv_make's).
// vecs: c | d resp. x.  pre: B_c B_d resp. B_a B_t B_u, compressed — the head of the proof.
int sv_entry(int kind, uint64_t seed, size_t n, const uint8_t* filler, size_t filler_len, uint8_t* fam2, uint8_t* vecs, uint8_t state[216], uint8_t* pre) {
  if (n < 2 || (n & (n - 1))) return -1;
  StdRng in(seed);
  StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
  FrDraw draw = [&rng]() { return rand_fr(rng); };
  Transcript transcript = start(filler, filler_len);
  if (kind == IPA) {
    std::vector<G1Aff> G = rand_points(in, n), Gp(n);
    std::vector<Fr> vec_u = rand_scalars(in, n);
    for (size_t i = 0; i < n; i++) Gp[i] = g1_to_affine(g1_mul(G1::from_affine(G[i]), vec_u[i]));
    const G1 crs_H = rand_g1(in);
    std::vector<Fr> vec_c = rand_scalars(in, n), vec_d = rand_scalars(in, n);
    const Fr z = inner_product(vec_c, vec_d);
    const G1 C = g1_msm(G, vec_c), D = g1_msm(Gp, vec_d);
    std::vector<Fr> vec_r_c, vec_r_d;
    generate_ipa_blinders(draw, vec_c, vec_d, &vec_r_c, &vec_r_d);
    const G1 B_c = g1_msm(G, vec_r_c), B_d = g1_msm(Gp, vec_r_d);
    transcript.append_g1("ipa_step1", C);
    transcript.append_g1("ipa_step1", D);
    transcript.append_fr("ipa_step1", z);
    transcript.append_g1("ipa_step1", B_c);
    transcript.append_g1("ipa_step1", B_d);
    const Fr alpha = transcript.get_and_append_challenge("ipa_alpha");
    const Fr beta = transcript.get_and_append_challenge("ipa_beta");
    for (size_t i = 0; i < n; i++) {
      fr_to_wire(vec_r_c[i] + alpha * vec_c[i], vecs + 32 * i);
      fr_to_wire(vec_r_d[i] + alpha * vec_d[i], vecs + 32 * (n + i));
    }
    affs_to_wire(Gp, fam2);
    aff_to_wire(g1_to_affine(g1_mul(crs_H, beta)), fam2 + 96 * n);
    g1_compress(B_c, pre);
    g1_compress(B_d, pre + 48);
  } else {
    std::vector<G1Aff> G = rand_points(in, n), T = rand_points(in, n), U = rand_points(in, n);
    std::vector<Fr> vec_x = rand_scalars(in, n);
    const G1 A = g1_msm(G, vec_x), Z_t = g1_msm(T, vec_x), Z_u = g1_msm(U, vec_x);
    std::vector<Fr> vec_r = generate_blinders(draw, n);
    const G1 B_a = g1_msm(G, vec_r), B_t = g1_msm(T, vec_r), B_u = g1_msm(U, vec_r);
    transcript.append_g1("same_msm_step1", A);
    transcript.append_g1("same_msm_step1", Z_t);
    transcript.append_g1("same_msm_step1", Z_u);
    transcript.append_g1_vec("same_msm_step1", T);
    transcript.append_g1_vec("same_msm_step1", U);
    transcript.append_g1("same_msm_step1", B_a);
    transcript.append_g1("same_msm_step1", B_t);
    transcript.append_g1("same_msm_step1", B_u);
    const Fr alpha = transcript.get_and_append_challenge("same_msm_alpha");
    for (size_t i = 0; i < n; i++) fr_to_wire(vec_r[i] + alpha * vec_x[i], vecs + 32 * i);
    g1_compress(B_a, pre);
    g1_compress(B_t, pre + 48);
    g1_compress(B_u, pre + 96);
  }
  state_words(transcript, state);
  return 0;
}

// verdict: SV_OK, SV_ERR_VERIFY or SV_ERR_DESERIALIZE (then state_out = the state before, challenges = zeros).
// challenges: alpha, beta, gamma_1..L resp. alpha, gamma_1..L.  Returns 0, or -1 for an argument the shim cannot take, -2 when the oracle's
// verify returned false before the accumulator, -3 when the call-by-call transcript disagrees with the oracle's.
int sv_verify(int kind, size_t n, const uint8_t* filler, size_t filler_len, const uint8_t* bases, const uint8_t* stmt, const uint8_t* z_in, const uint8_t* u_in,
              const uint8_t* proof, size_t proof_len, const uint8_t* rand, int* verdict, uint8_t* challenges, uint8_t state_out[216]) {
  if (!n || (n & (n - 1))) return -1;
  const size_t L = log2_of(n), nchal = (kind == IPA ? 2 : 1) + L;
  Transcript transcript = start(filler, filler_len), again = transcript;
  MsmAccumulator acc;
  Replayer rp{rand, (size_t)(kind == IPA ? 2 : 3)};
  FrDraw draw = [&rp]() { return rp(); };
  std::vector<Fr> chal;
  memset(challenges, 0, 32 * nchal);
  if (kind == IPA) {
    InnerProductProof pf;
    if (!deserialize(proof, proof_len, L, &pf)) {
      *verdict = SV_ERR_DESERIALIZE;
      state_words(transcript, state_out);
      return 0;
    }
    const std::vector<G1Aff> G = affs_from_wire(bases, n);
    const G1 crs_H = jac_from_wire(stmt), C = jac_from_wire(stmt + 144), D = jac_from_wire(stmt + 288);
    const Fr z = fr_from_wire(z_in);
    std::vector<Fr> vec_u(n);
    for (size_t i = 0; i < n; i++) vec_u[i] = fr_from_wire(u_in + 32 * i);
    if (!ipa_verify(pf, G, crs_H, C, D, z, vec_u, transcript, acc, draw)) return -2;
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
    SameMultiscalarProof pf;
    if (!deserialize(proof, proof_len, L, &pf)) {
      *verdict = SV_ERR_DESERIALIZE;
      state_words(transcript, state_out);
      return 0;
    }
    const std::vector<G1Aff> G = affs_from_wire(bases, n), T = affs_from_wire(bases + 96 * n, n), U = affs_from_wire(bases + 192 * n, n);
    const G1 A = jac_from_wire(stmt), Z_t = jac_from_wire(stmt + 144), Z_u = jac_from_wire(stmt + 288);
    if (!samemsm_verify(pf, G, A, Z_t, Z_u, T, U, transcript, acc, draw)) return -2;
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
  if (rp.overrun || rp.pos != rp.n) return -1;
  uint8_t other[216];
  state_words(transcript, state_out);
  state_words(again, other);
  if (memcmp(state_out, other, 216) != 0) return -3;
  for (size_t i = 0; i < nchal; i++) fr_to_wire(chal[i], challenges + 32 * i);
  *verdict = acc.verify() ? SV_OK : SV_ERR_VERIFY;
  return 0;
}

// the serialised lengths of the oracle's proofs with L rounds of identity points (what `serialize` writes does not depend on the points)
size_t sv_serialized_len(int kind, size_t L) {
  const std::vector<G1> v(L, G1::identity());
  if (kind == IPA) {
    InnerProductProof pf;
    pf.B_c = pf.B_d = G1::identity();
    pf.vec_L_C = pf.vec_R_C = pf.vec_L_D = pf.vec_R_D = v;
    pf.c_final = pf.d_final = Fr::zero();
    return serialize(pf).size();
  }
  SameMultiscalarProof pf;
  pf.B_a = pf.B_t = pf.B_u = G1::identity();
  pf.vec_L_A = pf.vec_L_T = pf.vec_L_U = pf.vec_R_A = pf.vec_R_T = pf.vec_R_U = v;
  pf.x_final = Fr::zero();
  return serialize(pf).size();
}

}  // extern "C"
