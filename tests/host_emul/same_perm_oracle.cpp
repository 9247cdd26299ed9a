// TEST INFRASTRUCTURE: a shared library over oracle/protocol.h (read-only) for the tests of cpx_same_perm_prove / cpx_same_perm_verify
// (tests/same_perm_lib.py builds it through check_harness.build_emul).  It takes the wire helpers and the grand-product layer's `derive` of
// gprod_oracle.cpp by including that file, which it does not change.
//   sp_inputs  from a seed the inputs of one stand-alone SamePermutationProof::new.  consistent = 1: a statement the witness satisfies, made
//              as the reference's own test makes one (same_permutation_argument.rs:216-240): A = <sigma(a), G> + <r_a, H>,
//              M = <sigma, G> + <r_m, H> for a seeded permutation sigma.  consistent = 0: A and M are arbitrary.
//   sp_derive  what `new` hands GrandProductProof::new from a given transcript state: B, gprod_result, the factors, vec_b_blinders, alpha,
//              beta and the state after step 1
//   sp_gprod   the oracle's gprod_new from a given transcript STATE (gprod_oracle.cpp's gp_prove starts from a filler): with the state of a
//              filler it must give gp_prove's bytes, which pins this shim's serialisation to that one; with sp_derive's outputs it must
//              give the bytes sp_prove embeds
//   sp_prove   the oracle's OWN sameperm_new on the caller's inputs and draws: the serialised proof (:173-177), the state afterwards and the
//              challenges — the latter from a second transcript driven call by call, which must end in the same state.  status 1 where the
//              reference panics in generate_ipa_blinders: zero bytes, the state as it was.
//   sp_verify  the oracle's sameperm_verify of given proof bytes against a fresh MsmAccumulator with the caller's three factors:
//              0 accepted, 1 rejected, 2 the bytes do not deserialise
#include "gprod_oracle.cpp"

namespace {

Transcript load_state(const uint8_t in[216]) {
  Transcript t("subarg");
  uint64_t w[27];
  memcpy(w, in, 216);
  memcpy(t.strobe.state, w, 200);
  t.strobe.pos = (uint8_t)w[25];
  t.strobe.pos_begin = (uint8_t)w[26];
  t.strobe.cur_flags = 0;
  return t;
}
struct SpDerived {
  Fr alpha, beta, result;
  G1 B;
  std::vector<Fr> factors, rb;
};
// same_permutation_argument.rs:59-81 said again on the oracle's primitives
SpDerived sp_layer(const std::vector<G1Aff>& crs_G, const G1& A, const G1& M, const std::vector<Fr>& a, const std::vector<uint32_t>& perm, const std::vector<Fr>& ra,
                   const std::vector<Fr>& rm, Transcript& t) {
  SpDerived o;
  t.append_g1("same_perm_step1", A);
  t.append_g1("same_perm_step1", M);
  t.append_fr_vec("same_perm_step1", a);
  o.alpha = t.get_and_append_challenge("same_perm_alpha");
  o.beta = t.get_and_append_challenge("same_perm_beta");
  o.result = Fr::one();
  G1 sum = G1::identity();
  for (size_t i = 0; i < crs_G.size(); i++) {
    o.factors.push_back(a[perm[i]] + Fr::from_u64(perm[i]) * o.alpha + o.beta);
    o.result *= o.factors.back();
    sum = g1_add(sum, G1::from_affine(crs_G[i]));
  }
  o.B = g1_add(g1_add(A, g1_mul(M, o.alpha)), g1_mul(sum, o.beta));
  for (size_t k = 0; k < ra.size(); k++) o.rb.push_back(ra[k] + o.alpha * rm[k]);
  return o;
}
std::vector<uint32_t> perm_from_wire(const uint32_t* p, size_t ell) { return std::vector<uint32_t>(p, p + ell); }
void write_gprod(ByteWriter& w, const GrandProductProof& pf) {
  const InnerProductProof& ip = pf.ipa_proof;
  w.g1(pf.C);
  w.fr(pf.r_p);
  w.g1(ip.B_c);
  w.g1(ip.B_d);
  w.g1v(ip.vec_L_C);
  w.g1v(ip.vec_R_C);
  w.g1v(ip.vec_L_D);
  w.g1v(ip.vec_R_D);
  w.fr(ip.c_final);
  w.fr(ip.d_final);
}

}  // namespace

extern "C" {

int sp_inputs(uint64_t seed, size_t ell, size_t nb, int consistent, uint8_t* G, uint8_t* H, uint8_t* crs_U, uint8_t* A, uint8_t* M, uint8_t* vec_a, uint32_t* perm,
              uint8_t* ra, uint8_t* rm, uint8_t* g_sum, uint8_t* h_sum) {
  if (!ell) return -1;
  StdRng in(seed);
  std::vector<G1Aff> vg(ell), vh(nb);
  for (auto& p : vg) p = g1_to_affine(rand_g1(in));
  for (auto& p : vh) p = g1_to_affine(rand_g1(in));
  const G1 U = rand_g1(in);
  std::vector<Fr> va(ell), vra(nb), vrm(nb), a_perm(ell), sigma(ell);
  for (auto& x : va) x = rand_fr(in);
  for (auto& x : vra) x = rand_fr(in);
  for (auto& x : vrm) x = rand_fr(in);
  std::vector<uint32_t> p(ell);
  for (size_t i = 0; i < ell; i++) p[i] = (uint32_t)i;
  for (size_t i = ell - 1; i > 0; i--) std::swap(p[i], p[in.next_u32() % (i + 1)]);
  for (size_t i = 0; i < ell; i++) {
    a_perm[i] = va[p[i]];
    sigma[i] = Fr::from_u64(p[i]);
  }
  G1 vA = g1_add(g1_msm(vg, a_perm), g1_msm(vh, vra)), vM = g1_add(g1_msm(vg, sigma), g1_msm(vh, vrm));
  if (!consistent) {
    vA = rand_g1(in);
    vM = rand_g1(in);
  }
  for (size_t i = 0; i < ell; i++) aff_to_wire(vg[i], G + 96 * i);
  for (size_t i = 0; i < nb; i++) aff_to_wire(vh[i], H + 96 * i);
  jac_to_wire(U, crs_U);
  jac_to_wire(vA, A);
  jac_to_wire(vM, M);
  for (size_t i = 0; i < ell; i++) fr_to_wire(va[i], vec_a + 32 * i);
  memcpy(perm, p.data(), 4 * ell);
  for (size_t i = 0; i < nb; i++) fr_to_wire(vra[i], ra + 32 * i);
  for (size_t i = 0; i < nb; i++) fr_to_wire(vrm[i], rm + 32 * i);
  aff_to_wire(sum_of(vg), g_sum);
  aff_to_wire(sum_of(vh), h_sum);
  return 0;
}

// chal_out: alpha, beta
int sp_derive(size_t ell, size_t nb, const uint8_t state_in[216], const uint8_t* G, const uint8_t* A, const uint8_t* M, const uint8_t* vec_a, const uint32_t* perm,
              const uint8_t* ra, const uint8_t* rm, uint8_t* B_out, uint8_t* result_out, uint8_t* factors_out, uint8_t* rb_out, uint8_t* chal_out, uint8_t state_out[216]) {
  if (!ell) return -1;
  for (size_t i = 0; i < ell; i++)
    if (perm[i] >= ell) return -1;
  Transcript t = load_state(state_in);
  const SpDerived o = sp_layer(affs_from_wire(G, ell), jac_from_wire(A), jac_from_wire(M), frs_from_wire(vec_a, ell), perm_from_wire(perm, ell), frs_from_wire(ra, nb),
                               frs_from_wire(rm, nb), t);
  jac_to_wire(o.B, B_out);
  fr_to_wire(o.result, result_out);
  for (size_t i = 0; i < ell; i++) fr_to_wire(o.factors[i], factors_out + 32 * i);
  for (size_t k = 0; k < nb; k++) fr_to_wire(o.rb[k], rb_out + 32 * k);
  fr_to_wire(o.alpha, chal_out);
  fr_to_wire(o.beta, chal_out + 32);
  state_words(t, state_out);
  return 0;
}

// the oracle's gprod_new from a transcript state; no look at generate_ipa_blinders' panics: the caller hands items that have blinders
int sp_gprod(size_t ell, size_t nb, const uint8_t state_in[216], const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B, const uint8_t* result,
             const uint8_t* b, const uint8_t* rb, const uint8_t* draws, size_t ndraws, uint8_t* proof, uint8_t state_out[216]) {
  const size_t n = ell + nb;
  if (!ell || n < 2 || (n & (n - 1)) || ndraws != nb + 2 * n - 2) return -1;
  Transcript t = load_state(state_in);
  Replayer rp{draws, ndraws};
  FrDraw draw = [&rp]() { return rp(); };
  const GrandProductProof pf = gprod_new(affs_from_wire(G, ell), affs_from_wire(H, nb), jac_from_wire(crs_U), jac_from_wire(B), fr_from_wire(result), frs_from_wire(b, ell),
                                         frs_from_wire(rb, nb), t, draw);
  ByteWriter w;
  write_gprod(w, pf);
  if (rp.overrun || rp.pos != rp.n || w.b.size() != 48 * (3 + 4 * log2_of(n)) + 96) return -1;
  memcpy(proof, w.b.data(), w.b.size());
  state_words(t, state_out);
  return 0;
}

// challenges: same-perm alpha, beta, gprod alpha, beta, ipa alpha, beta, gamma_1..L.  Returns 0, -1 for an argument the shim cannot take, -3
// when the call-by-call transcript disagrees with the oracle's
int sp_prove(size_t ell, size_t nb, const uint8_t state_in[216], const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A, const uint8_t* M,
             const uint8_t* vec_a, const uint32_t* perm, const uint8_t* ra, const uint8_t* rm, const uint8_t* draws, size_t ndraws, uint8_t* proof, size_t* proof_len,
             uint8_t* challenges, uint8_t state_out[216], int* status) {
  const size_t n = ell + nb;
  if (!ell || n < 2 || (n & (n - 1)) || ndraws != nb + 2 * n - 2) return -1;
  for (size_t i = 0; i < ell; i++)
    if (perm[i] >= ell) return -1;
  const size_t L = log2_of(n), nchal = 6 + L, plen = 48 * (4 + 4 * L) + 96;
  Transcript transcript = load_state(state_in), again = transcript, probe = transcript;
  const std::vector<G1Aff> vg = affs_from_wire(G, ell), vh = affs_from_wire(H, nb);
  const G1 U = jac_from_wire(crs_U), vA = jac_from_wire(A), vM = jac_from_wire(M);
  const std::vector<Fr> va = frs_from_wire(vec_a, ell), vra = frs_from_wire(ra, nb), vrm = frs_from_wire(rm, nb);
  const std::vector<uint32_t> vp = perm_from_wire(perm, ell);
  *status = 0;
  *proof_len = plen;
  {   // inner_product_argument.rs:69, :71 on the vectors the grand-product layer extends
    const SpDerived s = sp_layer(vg, vA, vM, va, vp, vra, vrm, probe);
    const Derived o = derive(vg, vh, s.B, s.result, s.factors, s.rb, frs_from_wire(draws, nb), probe);
    const std::vector<Fr> r = frs_from_wire(draws + 32 * nb, n);
    bool panics = o.c[n - 2].is_zero();
    if (!panics) panics = ((-r[n - 2]) * o.c[n - 2].inverse() * o.c[n - 1] + r[n - 1]).is_zero();
    if (panics) {
      *status = 1;
      memset(proof, 0, plen);
      memset(challenges, 0, 32 * nchal);
      state_words(transcript, state_out);
      return 0;
    }
  }
  Replayer rp{draws, ndraws};
  FrDraw draw = [&rp]() { return rp(); };
  const SamePermutationProof pf = sameperm_new(vg, vh, U, vA, vM, va, vp, vra, vrm, transcript, draw);
  const InnerProductProof& ip = pf.grand_product_proof.ipa_proof;
  ByteWriter w;
  w.g1(pf.B);
  write_gprod(w, pf.grand_product_proof);
  std::vector<Fr> chal;
  const SpDerived s = sp_layer(vg, vA, vM, va, vp, vra, vrm, again);
  chal.push_back(s.alpha);
  chal.push_back(s.beta);
  const Derived o = derive(vg, vh, s.B, s.result, s.factors, s.rb, frs_from_wire(draws, nb), again);
  chal.push_back(o.alpha);
  chal.push_back(o.beta);
  again.append_g1("ipa_step1", pf.grand_product_proof.C);
  again.append_g1("ipa_step1", o.D);
  again.append_fr("ipa_step1", o.inner_prod);
  again.append_g1("ipa_step1", ip.B_c);
  again.append_g1("ipa_step1", ip.B_d);
  chal.push_back(again.get_and_append_challenge("ipa_alpha"));
  chal.push_back(again.get_and_append_challenge("ipa_beta"));
  for (size_t j = 0; j < L; j++) {
    again.append_g1("ipa_loop", ip.vec_L_C[j]);
    again.append_g1("ipa_loop", ip.vec_L_D[j]);
    again.append_g1("ipa_loop", ip.vec_R_C[j]);
    again.append_g1("ipa_loop", ip.vec_R_D[j]);
    chal.push_back(again.get_and_append_challenge("ipa_gamma"));
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

// factors: the accumulator's three draws, the same-permutation check's first.  0 accepted, 1 rejected, 2 the bytes do not deserialise
int sp_verify(size_t ell, size_t nb, const uint8_t state_in[216], const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* g_sum, const uint8_t* h_sum,
              const uint8_t* A, const uint8_t* M, const uint8_t* vec_a, const uint8_t* proof, size_t proof_len, const uint8_t* factors, uint8_t state_out[216]) {
  const size_t n = ell + nb;
  if (!ell || (n & (n - 1))) return -1;
  const size_t L = log2_of(n);
  Transcript transcript = load_state(state_in);
  state_words(transcript, state_out);
  SamePermutationProof pf;
  GrandProductProof& gp = pf.grand_product_proof;
  ByteReader r{proof, proof_len};
  pf.B = r.g1();
  gp.C = r.g1();
  gp.r_p = r.fr();
  gp.ipa_proof.B_c = r.g1();
  gp.ipa_proof.B_d = r.g1();
  gp.ipa_proof.vec_L_C = r.g1v(L);
  gp.ipa_proof.vec_R_C = r.g1v(L);
  gp.ipa_proof.vec_L_D = r.g1v(L);
  gp.ipa_proof.vec_R_D = r.g1v(L);
  gp.ipa_proof.c_final = r.fr();
  gp.ipa_proof.d_final = r.fr();
  if (!r.ok || r.left) return 2;
  Replayer rp{factors, 3};
  FrDraw draw = [&rp]() { return rp(); };
  MsmAccumulator acc;
  const bool ok = sameperm_verify(pf, affs_from_wire(G, ell), affs_from_wire(H, nb), jac_from_wire(crs_U), aff_from_wire(g_sum), aff_from_wire(h_sum), jac_from_wire(A),
                                  jac_from_wire(M), frs_from_wire(vec_a, ell), nb, transcript, acc, draw) &&
                  acc.verify();
  state_words(transcript, state_out);
  return ok ? 0 : 1;
}

}  // extern "C"
