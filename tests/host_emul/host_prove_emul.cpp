// TEST-ONLY: the host-driven prover's steps (curdleproofs_amd/csrc/host_prove.hpp) compiled for the CPU and run in the order
// Engine::batch_prove_tables runs them, one proof.  The group side is the caller's: every point a step hashes arrives as the compressed
// bytes of its slot (`comp`), and each phase's results are handed over the way the engine does — in request order, through take.
// stdin: `name value` lines (hex but for ell and perm); stdout: `name hex` lines, scalars in wire form (Montgomery residues).
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "../../curdleproofs_amd/csrc/host_prove.hpp"

using namespace cpx;
typedef std::vector<uint8_t> Bytes;

static Bytes unhex(const std::string& h) {
  Bytes b(h.size() / 2);
  for (size_t i = 0; i < b.size(); i++) b[i] = (uint8_t)std::stoi(h.substr(2 * i, 2), nullptr, 16);
  return b;
}
static void put(const char* name, const void* p, size_t len) {
  printf("%s ", name);
  for (size_t i = 0; i < len; i++) printf("%02x", static_cast<const uint8_t*>(p)[i]);
  printf("\n");
}
static void put(const char* name, const host::SVec& v) { put(name, v.data(), v.size() * sizeof(host::S)); }
static void put(const char* name, const std::vector<Fr>& v) { put(name, v.data(), v.size() * sizeof(Fr)); }

int main() {
  std::map<std::string, std::string> in;
  std::string line;
  while (std::getline(std::cin, line)) {
    const size_t sp = line.find(' ');
    if (sp != std::string::npos) in[line.substr(0, sp)] = line.substr(sp + 1);
  }
  const size_t ell = std::stoul(in.at("ell")), n = ell + N_BLINDERS;
  size_t L = 0;
  while ((size_t(1) << L) < n) L++;
  const int ni = (int)n, Li = (int)L;
  const SlotMap sm(L);
  const ProofLayout pl(L);
  std::vector<uint32_t> perm;
  {
    std::istringstream is(in.at("perm"));
    for (uint32_t x; is >> x;) perm.push_back(x);
  }
  const Bytes rand = unhex(in.at("rand")), k = unhex(in.at("k")), mbl = unhex(in.at("m_blinders")), ic = unhex(in.at("ic")), mcomp = unhex(in.at("mcomp")),
              h_comp = unhex(in.at("h_comp")), comp = unhex(in.at("comp")), fin = unhex(in.at("final"));   // final: c | d | x, canonical
  if (perm.size() != ell || rand.size() != (size_t)RandIdx(ni).count() * 32 || k.size() != 32 || mbl.size() != 4 * 32 || ic.size() != 4 * ell * 48 || mcomp.size() != 48 ||
      h_comp.size() != 48 || comp.size() != (size_t)sm.count() * 48 || fin.size() != 3 * 32) {
    fprintf(stderr, "malformed case\n");
    return 2;
  }
  // a phase's results as the engine receives them: the compressed points of its requests, in request order
  auto results = [&](const ReqList& l) {
    Bytes r((size_t)l.n * 48, 0xee);
    for (int i = 0; i < l.n; i++)
      if (l.r[i].out >= 0) memcpy(&r[(size_t)i * 48], &comp[(size_t)l.r[i].out * 48], 48);
    return r;
  };
  host::ProveState s;
  host::prove_begin(s, ell, L, rand.data(), k.data(), perm.data(), ic.data(), mcomp.data());
  put("vec_a", s.vec_a);
  put("V_APERM", s.vec[V_APERM]);
  std::vector<Fr> side(3 * ell);
  host::prove_side_scalars(s, ell, side.data(), side.data() + ell, side.data() + 2 * ell);
  put("side", side);

  const ReqList p1 = prove_phase1b(ni, Li).then(prove_phase1(ni, Li));
  host::take(s, p1, results(p1).data());
  host::prove_after_phase1(s, ell, perm.data());
  put("V_C", s.vec[V_C]);

  const ReqList p2 = prove_phase2(ni, Li, false);
  host::take(s, p2, results(p2).data());
  host::prove_after_phase2(s, ell, mbl.data());
  put("V_U", s.vec[V_U]);
  put("V_D", s.vec[V_D]);
  put("V_ZZU", s.vec[V_ZZU]);

  const ReqList p3 = prove_phase3(ni, Li);
  host::take(s, p3, results(p3).data());
  std::vector<Fr> row(4 * n), gam(2 * L), beta(1);
  host::prove_ipa_setup(s, ell, L, row.data(), beta.data());
  put("ipa_row", row);
  put("ipa_beta", beta);
  for (size_t j = 0; j < L; j++) {
    const ReqList rd = cpx::prove_ipa_round(ni, Li, (int)j, false);
    host::take(s, rd, results(rd).data());
    host::prove_ipa_round(s, L, (int)j, &gam[2 * j]);
  }
  put("ipa_gamma", gam);

  const ReqList p1t = prove_phase1t(ni, Li);
  host::take(s, p1t, results(p1t).data());
  int side_slots[6];
  side_stream_slots(Li, side_slots);
  const int first = SL_CMT1;   // the window of slots the engine compresses on its side stream: cm_T.T_1 .. cm_B.T_2
  host::take(s, side_slots, 6, &comp[(size_t)first * 48], first);
  host::S c_fin, d_fin, x_fin;
  if (!host::S::from_le_bytes(&fin[0], &c_fin) || !host::S::from_le_bytes(&fin[32], &d_fin) || !host::S::from_le_bytes(&fin[64], &x_fin)) return 2;
  row.assign(2 * n, Fr::zero());
  host::prove_smsm_setup(s, ell, L, c_fin.f, d_fin.f, ic.data(), h_comp.data(), row.data());
  put("smsm_row", row);
  for (size_t j = 0; j < L; j++) {
    const ReqList rd = cpx::prove_smsm_round(ni, Li, (int)j);
    host::take(s, rd, results(rd).data());
    host::prove_smsm_round(s, L, (int)j, &gam[2 * j]);
  }
  put("smsm_gamma", gam);

  Bytes proof(pl.size(), 0xee);
  host::prove_serialize(s, L, x_fin.f, proof.data());
  put("proof", proof.data(), proof.size());
  put("sc", s.sc, sizeof(s.sc));
  return 0;
}
