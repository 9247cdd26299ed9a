// TEST INFRASTRUCTURE: a shared library over oracle/protocol.h (read-only) for the tests of cpx_gprod_prove (tests/gprod_lib.py builds it
// through check_harness.build_emul).
//   gp_inputs  from a seed the inputs of one stand-alone GrandProductProof::new.  consistent = 1: a statement the witness satisfies, made
//              as the reference's own test makes one (grand_product_argument.rs:275-298): gprod_result = prod b, B = <b, G> + <r_b, H>.
//              consistent = 0: gprod_result and B are arbitrary.  The sums of G and of H come out as well.
//   gp_derive  what `new` hands InnerProductProof::new for given inputs and vec_c_blinders on a transcript Transcript::new("subarg") +
//              filler: G | H, G', crs_U, C, D, inner_prod, c, d — for pinning the embedded IPA bytes to tests/host_emul/subarg_prove_oracle.cpp
//   gp_prove   the oracle's OWN gprod_new on the caller's inputs and draws: the serialised proof (:248-253), the state afterwards, and the
//              challenges — the latter from a second transcript driven call by call with the oracle's primitives on the proof's own
//              points, which must end in the same state.  Where the reference panics in generate_ipa_blinders on the extended vectors
//              (inner_product_argument.rs:69, :71) the shim says so (status 1) without finishing the prover: zero bytes, the state as it was.
//   gp_verify  the oracle's gprod_verify of given proof bytes against a fresh MsmAccumulator with the caller's two factors:
//              0 accepted, 1 rejected, 2 the bytes do not deserialise (:255-261)
// Wire forms as oracle/capi.cpp: Fr = 4 x u64 LE Montgomery, affine = x || y with zeros for the identity, Jacobian = X || Y || Z.
#include "../../oracle/protocol.h"

using namespace orc;

namespace {

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
std::vector<Fr> frs_from_wire(const uint8_t* b, size_t n) {
  std::vector<Fr> v(n);
  for (size_t i = 0; i < n; i++) v[i] = fr_from_wire(b + 32 * i);
  return v;
}
void state_words(const Transcript& t, uint8_t out[216]) {
  uint64_t w[27];
  memcpy(w, t.strobe.state, 200);
  w[25] = t.strobe.pos;
  w[26] = t.strobe.pos_begin;
  memcpy(out, w, 216);
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
size_t log2_of(size_t n) {
  size_t L = 0;
  while (((size_t)1 << L) < n) L++;
  return L;
}
G1Aff sum_of(const std::vector<G1Aff>& v) {
  G1 s = G1::identity();
  for (auto& p : v) s = g1_add(s, G1::from_affine(p));
  return g1_to_affine(s);
}

// the grand-product layer of `new` ahead of InnerProductProof::new (grand_product_argument.rs:62-145), said again on the oracle's
// primitives: what the IPA gets
struct Derived {
  Fr alpha, beta, r_p, inner_prod;
  G1 C, D;
  std::vector<G1Aff> G, G_prime;
  std::vector<Fr> c, d;
};
Derived derive(const std::vector<G1Aff>& crs_G, const std::vector<G1Aff>& crs_H, const G1& B, const Fr& result, const std::vector<Fr>& b, const std::vector<Fr>& rb,
               const std::vector<Fr>& c_blinders, Transcript& t) {
  const size_t ell = crs_G.size(), nb = crs_H.size();
  Derived o;
  t.append_g1("gprod_step1", B);
  t.append_fr("gprod_step1", result);
  o.alpha = t.get_and_append_challenge("gprod_alpha");
  o.c.push_back(Fr::one());
  for (size_t i = 0; i + 1 < ell; i++) o.c.push_back(o.c[i] * b[i]);
  o.C = g1_add(g1_msm(crs_G, o.c), g1_msm(crs_H, c_blinders));
  o.r_p = Fr::zero();
  for (size_t k = 0; k < nb; k++) o.r_p += (rb[k] + o.alpha) * c_blinders[k];
  t.append_g1("gprod_step2", o.C);
  t.append_fr("gprod_step2", o.r_p);
  o.beta = t.get_and_append_challenge("gprod_beta");
  const Fr beta_inv = o.beta.inverse();
  Fr pw = Fr::one(), ipw = beta_inv;
  G1 sum_g = G1::identity(), sum_h = G1::identity();
  for (size_t i = 0; i < ell; i++) {
    o.G_prime.push_back(g1_to_affine(g1_mul(G1::from_affine(crs_G[i]), ipw)));
    o.d.push_back(b[i] * pw * o.beta - pw);
    sum_g = g1_add(sum_g, G1::from_affine(crs_G[i]));
    pw *= o.beta;
    ipw *= beta_inv;
  }
  const Fr beta_l1 = pw * o.beta;   // pw = beta^ell, ipw = beta^-(ell+1)
  for (size_t k = 0; k < nb; k++) {
    o.G_prime.push_back(g1_to_affine(g1_mul(G1::from_affine(crs_H[k]), ipw)));
    o.d.push_back(beta_l1 * (rb[k] + o.alpha));
    sum_h = g1_add(sum_h, G1::from_affine(crs_H[k]));
  }
  o.D = g1_add(g1_sub(B, g1_mul(sum_g, beta_inv)), g1_mul(sum_h, o.alpha));
  o.inner_prod = o.r_p * beta_l1 + result * pw - Fr::one();
  o.G = crs_G;
  o.G.insert(o.G.end(), crs_H.begin(), crs_H.end());
  o.c.insert(o.c.end(), c_blinders.begin(), c_blinders.end());
  return o;
}

}  // namespace

extern "C" {

// G [ell], H [nb] affine; crs_U, B Jacobian; result, b [ell], rb [nb] scalars; g_sum, h_sum affine
int gp_inputs(uint64_t seed, size_t ell, size_t nb, int consistent, uint8_t* G, uint8_t* H, uint8_t* crs_U, uint8_t* B, uint8_t* result, uint8_t* b, uint8_t* rb,
              uint8_t* g_sum, uint8_t* h_sum) {
  if (!ell) return -1;
  StdRng in(seed);
  std::vector<G1Aff> vg(ell), vh(nb);
  for (auto& p : vg) p = g1_to_affine(rand_g1(in));
  for (auto& p : vh) p = g1_to_affine(rand_g1(in));
  const G1 U = rand_g1(in);
  std::vector<Fr> vb(ell), vrb(nb);
  for (auto& x : vb) x = rand_fr(in);
  for (auto& x : vrb) x = rand_fr(in);
  Fr res = Fr::one();
  for (auto& x : vb) res *= x;
  G1 vB = g1_add(g1_msm(vg, vb), g1_msm(vh, vrb));
  if (!consistent) {
    res = rand_fr(in);
    vB = rand_g1(in);
  }
  for (size_t i = 0; i < ell; i++) aff_to_wire(vg[i], G + 96 * i);
  for (size_t i = 0; i < nb; i++) aff_to_wire(vh[i], H + 96 * i);
  jac_to_wire(U, crs_U);
  jac_to_wire(vB, B);
  fr_to_wire(res, result);
  for (size_t i = 0; i < ell; i++) fr_to_wire(vb[i], b + 32 * i);
  for (size_t i = 0; i < nb; i++) fr_to_wire(vrb[i], rb + 32 * i);
  aff_to_wire(sum_of(vg), g_sum);
  aff_to_wire(sum_of(vh), h_sum);
  return 0;
}

// bases_out: G | H [n], then G' [n] affine; stmt_out: crs_U, C, D Jacobian; z_out: inner_prod; vecs_out: c [n] | d [n]
int gp_derive(size_t ell, size_t nb, const uint8_t* filler, size_t filler_len, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
              const uint8_t* result, const uint8_t* b, const uint8_t* rb, const uint8_t* c_blinders, uint8_t* bases_out, uint8_t* stmt_out, uint8_t* z_out,
              uint8_t* vecs_out, uint8_t state_out[216]) {
  if (!ell) return -1;
  const size_t n = ell + nb;
  Transcript t = start(filler, filler_len);
  const Derived o = derive(affs_from_wire(G, ell), affs_from_wire(H, nb), jac_from_wire(B), fr_from_wire(result), frs_from_wire(b, ell), frs_from_wire(rb, nb),
                           frs_from_wire(c_blinders, nb), t);
  for (size_t i = 0; i < n; i++) {
    aff_to_wire(o.G[i], bases_out + 96 * i);
    aff_to_wire(o.G_prime[i], bases_out + 96 * (n + i));
    fr_to_wire(o.c[i], vecs_out + 32 * i);
    fr_to_wire(o.d[i], vecs_out + 32 * (n + i));
  }
  memcpy(stmt_out, crs_U, 144);
  jac_to_wire(o.C, stmt_out + 144);
  jac_to_wire(o.D, stmt_out + 288);
  fr_to_wire(o.inner_prod, z_out);
  state_words(t, state_out);
  return 0;
}

// the oracle's ipa_new on the DERIVED inputs (what gp_derive exports) from the state after step 2, with the draws behind vec_c_blinders:
// the InnerProductProof bytes (inner_product_argument.rs:328-338) and the state afterwards.  draws: all nb + 2 n - 2 of the item
int gp_inner(size_t ell, size_t nb, const uint8_t* filler, size_t filler_len, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
             const uint8_t* result, const uint8_t* b, const uint8_t* rb, const uint8_t* draws, uint8_t* ipa_out, uint8_t state_out[216]) {
  const size_t n = ell + nb;
  if (!ell || n < 2 || (n & (n - 1))) return -1;
  Transcript t = start(filler, filler_len);
  const Derived o = derive(affs_from_wire(G, ell), affs_from_wire(H, nb), jac_from_wire(B), fr_from_wire(result), frs_from_wire(b, ell), frs_from_wire(rb, nb),
                           frs_from_wire(draws, nb), t);
  Replayer rp{draws + 32 * nb, 2 * n - 2};
  FrDraw draw = [&rp]() { return rp(); };
  const InnerProductProof ip = ipa_new(o.G, o.G_prime, jac_from_wire(crs_U), o.C, o.D, o.inner_prod, o.c, o.d, t, draw);
  ByteWriter w;
  w.g1(ip.B_c);
  w.g1(ip.B_d);
  w.g1v(ip.vec_L_C);
  w.g1v(ip.vec_R_C);
  w.g1v(ip.vec_L_D);
  w.g1v(ip.vec_R_D);
  w.fr(ip.c_final);
  w.fr(ip.d_final);
  if (rp.overrun || rp.pos != rp.n) return -1;
  memcpy(ipa_out, w.b.data(), w.b.size());
  state_words(t, state_out);
  return 0;
}

// draws: nb + 2 n - 2 (vec_c_blinders, then r [n], then z [n - 2]).  challenges: gprod alpha, gprod beta, ipa alpha, ipa beta, gamma_1..L.
// status: 0 = a proof, 1 = the reference panics in generate_ipa_blinders (proof and challenges zero, state_out = the state before).
// Returns 0, or -1 for an argument the shim cannot take, -3 when the call-by-call transcript disagrees with the oracle's.
int gp_prove(size_t ell, size_t nb, const uint8_t* filler, size_t filler_len, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
             const uint8_t* result, const uint8_t* b, const uint8_t* rb, const uint8_t* draws, size_t ndraws, uint8_t* proof, size_t* proof_len, uint8_t* challenges,
             uint8_t state_out[216], int* status) {
  const size_t n = ell + nb;
  if (!ell || n < 2 || (n & (n - 1)) || ndraws != nb + 2 * n - 2) return -1;
  const size_t L = log2_of(n), nchal = 4 + L, plen = 48 * (3 + 4 * L) + 96;
  Transcript transcript = start(filler, filler_len), again = transcript, probe = transcript;
  const std::vector<G1Aff> vg = affs_from_wire(G, ell), vh = affs_from_wire(H, nb);
  const G1 U = jac_from_wire(crs_U), vB = jac_from_wire(B);
  const Fr res = fr_from_wire(result);
  const std::vector<Fr> vb = frs_from_wire(b, ell), vrb = frs_from_wire(rb, nb);
  *status = 0;
  *proof_len = plen;
  {   // inner_product_argument.rs:69 `c[n-2].inverse().unwrap()`, :71 the denominator's, on the vectors `new` extends (:144-145)
    const Derived o = derive(vg, vh, vB, res, vb, vrb, frs_from_wire(draws, nb), probe);
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
  const GrandProductProof pf = gprod_new(vg, vh, U, vB, res, vb, vrb, transcript, draw);
  const InnerProductProof& ip = pf.ipa_proof;
  ByteWriter w;
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
  std::vector<Fr> chal;
  const Derived o = derive(vg, vh, vB, res, vb, vrb, frs_from_wire(draws, nb), again);   // steps 1 and 2 call by call, and D for the IPA's step 1
  chal.push_back(o.alpha);
  chal.push_back(o.beta);
  again.append_g1("ipa_step1", pf.C);
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

// factors: the accumulator's two draws.  0 accepted, 1 rejected, 2 the bytes do not deserialise; -1 an argument the shim cannot take
int gp_verify(size_t ell, size_t nb, const uint8_t* filler, size_t filler_len, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* g_sum,
              const uint8_t* h_sum, const uint8_t* B, const uint8_t* result, const uint8_t* proof, size_t proof_len, const uint8_t* factors, uint8_t state_out[216]) {
  const size_t n = ell + nb;
  if (!ell || (n & (n - 1))) return -1;
  const size_t L = log2_of(n);
  Transcript transcript = start(filler, filler_len);
  state_words(transcript, state_out);
  GrandProductProof pf;
  ByteReader r{proof, proof_len};
  pf.C = r.g1();
  pf.r_p = r.fr();
  pf.ipa_proof.B_c = r.g1();
  pf.ipa_proof.B_d = r.g1();
  pf.ipa_proof.vec_L_C = r.g1v(L);
  pf.ipa_proof.vec_R_C = r.g1v(L);
  pf.ipa_proof.vec_L_D = r.g1v(L);
  pf.ipa_proof.vec_R_D = r.g1v(L);
  pf.ipa_proof.c_final = r.fr();
  pf.ipa_proof.d_final = r.fr();
  if (!r.ok || r.left) return 2;
  Replayer rp{factors, 2};
  FrDraw draw = [&rp]() { return rp(); };
  MsmAccumulator acc;
  const bool ok = gprod_verify(pf, affs_from_wire(G, ell), affs_from_wire(H, nb), jac_from_wire(crs_U), aff_from_wire(g_sum), aff_from_wire(h_sum), jac_from_wire(B),
                               fr_from_wire(result), nb, transcript, acc, draw) &&
                  acc.verify();
  state_words(transcript, state_out);
  return ok ? 0 : 1;
}

}  // extern "C"
