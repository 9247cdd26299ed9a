// g++ program over curdleproofs_amd/csrc/loop_plan.hpp (tests/test_loop_rounds_cpu.py): the layout of cpx_ipa_rounds /
// cpx_same_msm_rounds exactly as Engine::loop_rounds and k_loop_step use it, printed as plain "key value..." lines.  The test builds it
// twice, the second time with -fsanitize=address,undefined.
//   loop_plan_emul plan <kind: 0 = IPA, 1 = SameMSM> <count> <n>     the whole plan, index lists included
//   loop_plan_emul limit <kind> <count> <n>                          the verdict of the limits alone
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/loop_plan.hpp"

using cpx::LoopPlan;

int main(int argc, char** argv) {
  if (argc != 5 || (strcmp(argv[1], "plan") && strcmp(argv[1], "limit"))) {
    fprintf(stderr, "usage: loop_plan_emul plan|limit <kind> <count> <n>\n");
    return 2;
  }
  const bool ipa = atoi(argv[2]) == 0;
  const size_t count = (size_t)strtoull(argv[3], nullptr, 10), n = (size_t)strtoull(argv[4], nullptr, 10);
  LoopPlan lp;
  const int status = (int)cpx::loop_plan(ipa, count, n, lp);
  printf("status %d\n", status);
  if (status != cpx::LOOP_OK || !strcmp(argv[1], "limit")) return 0;
  printf("L %zu\nterms %d\ntasks %zu\nround_points %zu\nbase_stride %zu\nh_index %zu\nvec_words %zu\nrow_words %zu\nfinals_each %zu\n", lp.L, lp.terms(), lp.tasks(),
         lp.round_points(), lp.base_stride(), lp.h_index(), lp.vec_words(), lp.row_words(), lp.finals_each());
  printf("fr %zu %zu %zu %zu %zu %zu\n", lp.fr_vec(), lp.fr_rows(), lp.fr_ones(), lp.fr_gammas(), lp.fr_finals(), lp.fr_total());
  printf("idx_len %zu\nidx_total %zu\nresults %zu\n", lp.idx_len(), lp.idx_total(), lp.results());
  for (int q = 0; q < lp.terms(); q++)
    printf("term %d %d %zu %d %d %u %d %d %zu\n", q, lp.term_family(q), lp.family_off(lp.term_family(q)), lp.term_hi(q) ? 1 : 0, lp.term_has_h(q) ? 1 : 0, lp.term_len(q),
           lp.term_vec(q), lp.term_vec_right(q) ? 1 : 0, lp.scal_off(q));
  for (int f = 0; f < (ipa ? 2 : 3); f++) printf("family %d %d\n", f, lp.family_gamma_power(f));
  for (int v = 0; v < (ipa ? 2 : 1); v++) printf("vec %d %d\n", v, lp.vec_gamma_power(v));
  std::vector<uint32_t> idx;
  lp.fill_idx(idx);
  for (size_t j = 0; j < lp.L; j++)
    for (int hi = 0; hi < 2; hi++) {
      printf("list %zu %d", j, hi);
      for (size_t t = 0; t < lp.idx_len(); t++) printf(" %u", idx[lp.idx_off(j, hi != 0) + t]);
      printf("\n");
    }
  cpx::Tier0MsmPlan pl;
  std::vector<uint32_t> lens;
  const bool ok = lp.round_msm(pl, lens);
  printf("msm %d %zu %zu %u\n", ok ? 1 : 0, pl.count, pl.points, pl.max_n);
  if (count) printf("result_last %zu\n", lp.result_index(lp.L ? lp.L - 1 : 0, count - 1, lp.terms() - 1));
  return 0;
}
