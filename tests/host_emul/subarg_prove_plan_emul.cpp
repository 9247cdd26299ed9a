// g++ program over curdleproofs_amd/csrc/subarg_prove_plan.hpp and blinder_algebra.hpp (tests/test_subarg_prove_cpu.py): the layout of
// cpx_ipa_prove / cpx_same_msm_prove exactly as Engine::subarg_prove and the kernels of subarg_prove.hip use it, and
// generate_ipa_blinders computed the way k_subarg_blinders computes it (partial sums of `workers` strided workers added up, then the
// solve), printed as plain "key value..." lines.  The test builds it twice, the second time with -fsanitize=address,undefined.
//   subarg_prove_plan_emul plan <kind: 0 = IPA, 1 = SameMSM> <count> <n>     the whole plan
//   subarg_prove_plan_emul limit <kind> <count> <n>                          the verdict of the limits alone
//   subarg_prove_plan_emul blinders <n> <workers> <hex>...                   c [n], d [n], r [n], z [n - 2] as canonical hexadecimal integers:
//                                                                             "singular 1", or "singular 0" and "rd" with the n entries of r_d
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/blinder_algebra.hpp"
#include "../../curdleproofs_amd/csrc/subarg_prove_plan.hpp"

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
  if (argc >= 4 && !strcmp(argv[1], "blinders")) {
    const int n = atoi(argv[2]), workers = atoi(argv[3]);
    if (n < 2 || workers < 1 || argc != 4 + 4 * n - 2) {
      fprintf(stderr, "blinders: n >= 2, workers >= 1 and 4 n - 2 scalars expected\n");
      return 2;
    }
    std::vector<Fr> in((size_t)(4 * n - 2));
    for (size_t i = 0; i < in.size(); i++) in[i] = from_hex(argv[4 + i]);
    const Fr *c = in.data(), *d = c + n, *r = d + n, *z = r + n;
    Fr omega = Fr::zero(), delta = Fr::zero();
    for (int w = 0; w < workers; w++) {   // the work-group's threads, then its reduction
      Fr om = Fr::zero(), de = Fr::zero();
      ipa_blinder_partial(r, z, c, d, n, w, workers, om, de);
      omega = fe_add(omega, om);
      delta = fe_add(delta, de);
    }
    const IpaBlinderTail t = ipa_blinder_solve(omega, delta, r[n - 2], r[n - 1], c[n - 2], c[n - 1]);
    printf("singular %d\n", t.singular ? 1 : 0);
    if (t.singular) return 0;
    printf("rd");
    for (int i = 0; i < n - 2; i++) print_hex(z[i]);
    print_hex(t.pen_z);
    print_hex(t.last_z);
    printf("\n");
    return 0;
  }
  if (argc != 5 || (strcmp(argv[1], "plan") && strcmp(argv[1], "limit"))) {
    fprintf(stderr, "usage: subarg_prove_plan_emul plan|limit <kind> <count> <n> | blinders <n> <workers> <hex>...\n");
    return 2;
  }
  const bool ipa = atoi(argv[2]) == 0;
  const size_t count = (size_t)strtoull(argv[3], nullptr, 10), n = (size_t)strtoull(argv[4], nullptr, 10);
  SubargProvePlan sp;
  const int status = (int)subarg_prove_plan(ipa, count, n, sp);
  printf("status %d\n", status);
  if (status != LOOP_OK || !strcmp(argv[1], "limit")) return 0;
  printf("L %zu\nfirst %zu\nnvec %zu\ndraws_each %zu\nab_each %zu\nchallenges %zu\nblocks %zu\nproof_points %zu\nproof_bytes %zu\npoints %zu\n", sp.L(), sp.first(), sp.nvec(),
         sp.draws_each(), sp.ab_each(), sp.challenges(), sp.blocks(), sp.proof_points(), sp.proof_bytes(), sp.points());
  printf("loop %zu %zu %zu\n", sp.lp.fr_total(), sp.lp.results(), sp.lp.L * sp.lp.tasks());
  printf("fr %zu %zu %zu %zu %zu %zu\n", sp.fr_wit(), sp.fr_draws(), sp.fr_rd(), sp.fr_z(), sp.fr_ab(), sp.fr_total());
  printf("by %zu %zu %zu %zu\n", sp.by_points(), sp.by_tu(), sp.by_rng(), sp.by_total());
  printf("aff %zu %zu\n", sp.aff_points(), sp.aff_total());
  printf("task %zu %zu\n", sp.task_first(), sp.task_total());
  const SubargTotals t = sp.totals();   // what the engine reserves at this depth, and what leads the proof
  printf("totals %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", t.fr, t.jac, t.aff, t.bytes, t.flags, t.ix, t.tasks, t.res, t.lead_bytes, t.lead_challenges);  if (count) printf("pt %zu %zu %zu %zu\n", sp.pt_first(0, 0), sp.pt_first(count - 1, sp.first() - 1), sp.pt_statement(0, 0), sp.pt_statement(count - 1, 2));
  for (size_t b = 0; b < sp.first(); b++) printf("first_family %zu %d\n", b, sp.first_family(b));
  for (size_t i = 0; i < sp.nvec(); i++) printf("scalar_byte %zu %zu\n", i, sp.scalar_byte(i));
  for (size_t b = 0; b < sp.blocks(); b++) {
    printf("block %zu %d", b, sp.block_term(b));
    for (size_t j = 0; j < sp.L(); j++) printf(" %zu", sp.round_slot(j, b));
    printf("\n");
  }
  Tier0MsmPlan pl;
  std::vector<uint32_t> lens;
  const bool ok = sp.first_msm(pl, lens);
  printf("msm %d %zu %zu %u\n", ok ? 1 : 0, pl.count, pl.points, pl.max_n);
  return 0;
}
