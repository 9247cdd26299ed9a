// TEST INFRASTRUCTURE: a shared library over oracle/protocol.h (read-only) for the tests of cpx_ipa_rounds / cpx_same_msm_rounds and of the
// cpx_transcript_* calls (tests/subarg_lib.py builds it through check_harness.build_emul).  From a seed it makes the inputs of one
// stand-alone InnerProductProof::new / SameMultiscalarProof::new, runs the steps BEFORE the log-round loop with the oracle's primitives
// (protocol.h ipa_new :181-198, samemsm_new :526-541 restated call by call), and exports what stands at loop entry: the bases, the point H,
// the vectors, and the Merlin state as 27 words (Strobe128::state as 25 little-endian u64, pos, pos_begin).  Then it runs the oracle's OWN
// ipa_new / samemsm_new from the start on a second transcript with the same draws and exports every L / R point compressed, the finals,
// the serialised proof and the state afterwards.  Wire forms as oracle/capi.cpp: Fr = 4 x u64 LE Montgomery, affine = x || y, identity = zeros.
#include "../../oracle/protocol.h"

using namespace orc;

namespace {

void aff_to_wire(const G1Aff& p, uint8_t* b) {
  if (p.inf) {
    memset(b, 0, 96);
    return;
  }
  memcpy(b, p.x.v, 48);
  memcpy(b + 48, p.y.v, 48);
}
void fr_to_wire(const Fr& x, uint8_t* b) { memcpy(b, x.v, 32); }
void state_words(const Transcript& t, uint8_t out[216]) {
  uint64_t w[27];
  memcpy(w, t.strobe.state, 200);
  w[25] = t.strobe.pos;
  w[26] = t.strobe.pos_begin;
  memcpy(out, w, 216);
}
void comp(const G1& p, uint8_t* out) { g1_compress(p, out); }
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
// a transcript that something has happened to already: `filler` bytes under a label of their own move pos around the rate
Transcript start(const uint8_t* filler, size_t filler_len) {
  Transcript t("subarg");
  if (filler_len) t.append_message("filler", filler, filler_len);
  return t;
}

}  // namespace

extern "C" {

// the Merlin state after Transcript::new("subarg") and one message of filler_len bytes (none for 0), as 27 words
void sub_state(const uint8_t* filler, size_t filler_len, uint8_t state[216]) { state_words(start(filler, filler_len), state); }

// pad: the last `pad` bases of G' are the identity (what the reference's zero padding looks like to the loop)
int sub_ipa(uint64_t seed, size_t n, size_t pad, const uint8_t* filler, size_t filler_len, uint8_t* G_out, uint8_t* Gp_out, uint8_t* H_out, uint8_t* c_out, uint8_t* d_out,
            uint8_t state_in[216], uint8_t pre_comp[96], uint8_t* rounds_comp, uint8_t finals[64], uint8_t state_out[216], uint8_t* proof, size_t* proof_len) {
  if (n < 2 || (n & (n - 1)) || pad > n) return -1;
  StdRng in(seed);
  std::vector<G1Aff> G = rand_points(in, n), Gp = rand_points(in, n);
  for (size_t i = n - pad; i < n; i++) Gp[i] = G1Aff::identity();
  const G1 crs_H = rand_g1(in), C = rand_g1(in), D = rand_g1(in);
  const Fr z = rand_fr(in);
  std::vector<Fr> vec_c = rand_scalars(in, n), vec_d = rand_scalars(in, n);
  for (size_t i = 0; i < n; i++) {
    aff_to_wire(G[i], G_out + 96 * i);
    aff_to_wire(Gp[i], Gp_out + 96 * i);
  }
  {   // ---- the steps before the loop, ipa_new :181-198
    StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
    FrDraw draw = [&rng]() { return rand_fr(rng); };
    Transcript transcript = start(filler, filler_len);
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
      fr_to_wire(vec_r_c[i] + alpha * vec_c[i], c_out + 32 * i);
      fr_to_wire(vec_r_d[i] + alpha * vec_d[i], d_out + 32 * i);
    }
    aff_to_wire(g1_to_affine(g1_mul(crs_H, beta)), H_out);
    comp(B_c, pre_comp);
    comp(B_d, pre_comp + 48);
    state_words(transcript, state_in);
  }
  // ---- the oracle's own prover, from the start
  StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
  FrDraw draw = [&rng]() { return rand_fr(rng); };
  Transcript transcript = start(filler, filler_len);
  const InnerProductProof pf = ipa_new(G, Gp, crs_H, C, D, z, vec_c, vec_d, transcript, draw);
  for (size_t j = 0; j < pf.vec_L_C.size(); j++) {
    comp(pf.vec_L_C[j], rounds_comp + (4 * j + 0) * 48);
    comp(pf.vec_L_D[j], rounds_comp + (4 * j + 1) * 48);
    comp(pf.vec_R_C[j], rounds_comp + (4 * j + 2) * 48);
    comp(pf.vec_R_D[j], rounds_comp + (4 * j + 3) * 48);
  }
  fr_to_wire(pf.c_final, finals);
  fr_to_wire(pf.d_final, finals + 32);
  state_words(transcript, state_out);
  ByteWriter w;   // inner_product_argument.rs:328-338
  w.g1(pf.B_c);
  w.g1(pf.B_d);
  w.g1v(pf.vec_L_C);
  w.g1v(pf.vec_R_C);
  w.g1v(pf.vec_L_D);
  w.g1v(pf.vec_R_D);
  w.fr(pf.c_final);
  w.fr(pf.d_final);
  memcpy(proof, w.b.data(), w.b.size());
  *proof_len = w.b.size();
  return 0;
}

// pad: the last `pad` entries of T and U are the identity except T[n - 2] and U[n - 1] (curdleproofs.rs:141-155: O O H O / O O O H)
int sub_samemsm(uint64_t seed, size_t n, size_t pad, const uint8_t* filler, size_t filler_len, uint8_t* G_out, uint8_t* T_out, uint8_t* U_out, uint8_t* x_out,
                uint8_t state_in[216], uint8_t pre_comp[144], uint8_t* rounds_comp, uint8_t finals[32], uint8_t state_out[216], uint8_t* proof, size_t* proof_len) {
  if (n < 2 || (n & (n - 1)) || pad > n) return -1;
  StdRng in(seed);
  std::vector<G1Aff> G = rand_points(in, n), T = rand_points(in, n), U = rand_points(in, n);
  for (size_t i = n - pad; i < n; i++) {
    if (i != n - 2) T[i] = G1Aff::identity();
    if (i != n - 1) U[i] = G1Aff::identity();
  }
  const G1 A = rand_g1(in), Z_t = rand_g1(in), Z_u = rand_g1(in);
  std::vector<Fr> vec_x = rand_scalars(in, n);
  for (size_t i = 0; i < n; i++) {
    aff_to_wire(G[i], G_out + 96 * i);
    aff_to_wire(T[i], T_out + 96 * i);
    aff_to_wire(U[i], U_out + 96 * i);
  }
  {   // ---- the steps before the loop, samemsm_new :526-541
    StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
    FrDraw draw = [&rng]() { return rand_fr(rng); };
    Transcript transcript = start(filler, filler_len);
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
    for (size_t i = 0; i < n; i++) fr_to_wire(vec_r[i] + alpha * vec_x[i], x_out + 32 * i);
    comp(B_a, pre_comp);
    comp(B_t, pre_comp + 48);
    comp(B_u, pre_comp + 96);
    state_words(transcript, state_in);
  }
  StdRng rng(seed ^ 0x9e3779b97f4a7c15ULL);
  FrDraw draw = [&rng]() { return rand_fr(rng); };
  Transcript transcript = start(filler, filler_len);
  const SameMultiscalarProof pf = samemsm_new(G, A, Z_t, Z_u, T, U, vec_x, transcript, draw);
  for (size_t j = 0; j < pf.vec_L_A.size(); j++) {
    const G1* six[6] = {&pf.vec_L_A[j], &pf.vec_L_T[j], &pf.vec_L_U[j], &pf.vec_R_A[j], &pf.vec_R_T[j], &pf.vec_R_U[j]};
    for (int q = 0; q < 6; q++) comp(*six[q], rounds_comp + (6 * j + q) * 48);
  }
  fr_to_wire(pf.x_final, finals);
  state_words(transcript, state_out);
  ByteWriter w;   // same_multiscalar_argument.rs:263-275
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
  memcpy(proof, w.b.data(), w.b.size());
  *proof_len = w.b.size();
  return 0;
}

}  // extern "C"
