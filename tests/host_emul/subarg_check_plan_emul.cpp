// g++ program over curdleproofs_amd/csrc/subarg_check_plan.hpp (tests/test_subarg_verify_cpu.py): the layout of cpx_ipa_verify /
// cpx_same_msm_verify exactly as Engine::subarg_verify and k_subarg_scalars use it, and an item's row of weights computed the way the
// kernel computes it (over Fr, every s_i and 1 / s_i from its index, the challenges inverted by fr_inv_divsteps), printed as plain
// "key value..." lines.  The test builds it twice, the second time with -fsanitize=address,undefined.
//   subarg_check_plan_emul plan <kind: 0 = IPA, 1 = SameMSM> <count> <n>     the whole plan, index words included
//   subarg_check_plan_emul limit <kind> <count> <n>                          the verdict of the limits alone
//   subarg_check_plan_emul row <kind> <n> <hex>...                           the row of one item; scalars as canonical hexadecimal integers:
//                           factors (2 | 3), alpha, (beta,) gamma_1..L, finals (c, d | x), then for the IPA z and u_0..u_{n-1}
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/modinv30.hpp"
#include "../../curdleproofs_amd/csrc/subarg_check_plan.hpp"

using namespace cpx;

static Fr from_hex(const char* s) {   // canonical integer -> Montgomery
  Fr c = Fr::zero();
  const size_t len = strlen(s);
  for (size_t i = 0; i < len && i < 64; i++) {
    const char ch = s[len - 1 - i];
    const uint32_t d = ch >= '0' && ch <= '9' ? (uint32_t)(ch - '0') : (uint32_t)((ch | 0x20) - 'a' + 10);
    c.v[i / 8] |= (d & 15u) << (4 * (i % 8));
  }
  return fe_to_mont(c);
}
static void print_hex(const Fr& mont) {
  const Fr c = fe_from_mont(mont);
  printf(" ");
  for (int j = 7; j >= 0; j--) printf("%08x", c.v[j]);
}

int main(int argc, char** argv) {
  const bool row = argc >= 4 && !strcmp(argv[1], "row");
  if (!row && (argc != 5 || (strcmp(argv[1], "plan") && strcmp(argv[1], "limit")))) {
    fprintf(stderr, "usage: subarg_check_plan_emul plan|limit <kind> <count> <n> | row <kind> <n> <hex>...\n");
    return 2;
  }
  const bool ipa = atoi(argv[2]) == 0;
  SubargCheckPlan sp;
  if (row) {
    const size_t n = (size_t)strtoull(argv[3], nullptr, 10);
    if (subarg_check_plan(ipa, 1, n, sp) != SUBARG_OK) return 2;
    const size_t L = sp.L, want = (size_t)sp.checks() + sp.challenges() + sp.proof_scalars() + (ipa ? 1 + n : 0);
    if ((size_t)argc != 4 + want) {
      fprintf(stderr, "row: %zu scalars expected\n", want);
      return 2;
    }
    std::vector<Fr> in(want);
    for (size_t i = 0; i < want; i++) in[i] = from_hex(argv[4 + i]);
    size_t at = 0;
    SubargTerms<Fr> w;
    w.a[2] = w.beta = w.z = w.fin[1] = w.h = w.af[2] = Fr::zero();   // (what one kind does not use)
    for (int k = 0; k < sp.checks(); k++) w.a[k] = in[at++];
    w.alpha = in[at++];
    if (ipa) w.beta = in[at++];
    std::vector<Fr> gam(2 * L + 1);
    for (size_t j = 0; j < L; j++) gam[j] = in[at++];
    for (size_t j = 0; j < L; j++) gam[L + j] = fr_inv_divsteps(gam[j]);
    for (size_t k = 0; k < sp.proof_scalars(); k++) w.fin[k] = in[at++];
    if (ipa) w.z = in[at++];
    const Fr* u = in.data() + at;
    w.gam = gam.data();
    w.gam_inv = gam.data() + L;
    w.set(ipa);
    std::vector<Fr> out(sp.points());
    for (size_t i = 0; i < n; i++) {
      const Fr s_i = verification_scalar(w.gam, (int)L, (int)i);
      if (ipa) out[i] = subarg_base_weight(w, true, 0, s_i, fe_mul(u[i], verification_scalar(w.gam_inv, (int)L, (int)i)));
      else
        for (int f = 0; f < 3; f++) out[sp.base_off(f) + i] = subarg_base_weight(w, false, f, s_i, s_i);
    }
    for (size_t s = 0; s < sp.proof_points(); s++) out[sp.proof_off() + s] = subarg_proof_weight(w, sp, (int)s);
    for (size_t k = 0; k < SubargCheckPlan::kStatement; k++) out[sp.statement_off() + k] = subarg_statement_weight(w, ipa, (int)k);
    printf("row");
    for (const Fr& x : out) print_hex(x);
    printf("\n");
    return 0;
  }
  const size_t count = (size_t)strtoull(argv[3], nullptr, 10), n = (size_t)strtoull(argv[4], nullptr, 10);
  const int status = (int)subarg_check_plan(ipa, count, n, sp);
  printf("status %d\n", status);
  if (status != SUBARG_OK || !strcmp(argv[1], "limit")) return 0;
  printf("L %zu\nchecks %d\nfamilies %d\nproof_points %zu\nproof_scalars %zu\nproof_bytes %zu\nchallenges %zu\nterms %d\npoints %zu\nproof_off %zu\nstatement_off %zu\n", sp.L,
         sp.checks(), sp.families(), sp.proof_points(), sp.proof_scalars(), sp.proof_bytes(), sp.challenges(), sp.terms(), sp.points(), sp.proof_off(), sp.statement_off());
  printf("fr %zu %zu %zu %zu %zu %zu\n", sp.fr_weights(), sp.fr_z(), sp.fr_u(), sp.fr_rand(), sp.fr_challenges(), sp.fr_total());
  printf("by %zu %zu %zu %zu\n", sp.by_proofs(), sp.by_statement(), sp.by_tu(), sp.by_total());
  printf("ix %zu %zu %zu %zu\n", sp.ix_src(), sp.ix_dst(), sp.ix_statement(), sp.ix_total());
  printf("st %zu %zu\njac %zu\naff %zu\n", sp.st_bad(), sp.st_total(), sp.jac_total(), sp.aff_total());
  const SubargTotals t = sp.totals();   // what the engine reserves at this depth, and what leads the proof
  printf("totals %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", t.fr, t.jac, t.aff, t.bytes, t.flags, t.ix, t.tasks, t.res, t.lead_bytes, t.lead_challenges);
  for (int f = 0; f < sp.families(); f++) printf("base_off %d %zu\n", f, sp.base_off(f));
  for (size_t i = 0; i < sp.proof_scalars(); i++) printf("scalar_byte %zu %zu\n", i, sp.scalar_byte(i));
  for (int b = 0; b < sp.terms(); b++) printf("block %d %d %d %zu\n", b, sp.block_is_right(b) ? 1 : 0, sp.block_check(b), sp.L ? sp.block_slot(b, 0) : 0);
  for (size_t j = 0; j < sp.L; j++) {
    printf("round %zu", j);
    for (int q = 0; q < sp.terms(); q++) printf(" %zu", sp.round_slot(j, q));
    printf("\n");
  }
  std::vector<uint32_t> ix;
  sp.fill_idx(ix);
  const char* names[3] = {"src", "dst", "statement"};
  const size_t first[4] = {sp.ix_src(), sp.ix_dst(), sp.ix_statement(), sp.ix_total()};
  for (int k = 0; k < 3; k++) {
    printf("idx_%s", names[k]);
    for (size_t t = first[k]; t < first[k + 1]; t++) printf(" %u", ix[t]);
    printf("\n");
  }
  Tier0MsmPlan pl;
  std::vector<uint32_t> lens;
  const bool ok = sp.msm(pl, lens);
  printf("msm %d %zu %zu %u\n", ok ? 1 : 0, pl.count, pl.points, pl.max_n);
  return 0;
}
