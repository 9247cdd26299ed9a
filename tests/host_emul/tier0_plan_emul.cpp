// g++ program over curdleproofs_amd/csrc/tier0_plan.hpp (tests/test_tier0_rounds_cpu.py): the offset and size arithmetic of
// cpx_g1_msm_many / cpx_g1_fold_many exactly as Engine::msm_many / Engine::fold_many call it, printed as plain "key value..." lines.
// The test builds it twice, the second time with -fsanitize=address,undefined.
//   tier0_plan_emul msm <tbw_slices option> [len ...]     the plan of one call
//   tier0_plan_emul refuse <count>                        a call of `count` tasks whose lens pointer is NULL: refused before it is read
//   tier0_plan_emul points <len> <repeat>                 `repeat` tasks of `len` points: accepted or refused by the point limit
//   tier0_plan_emul fold <families> <half> <fold_quad_max> <plain>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/tier0_plan.hpp"

using cpx::Tier0MsmPlan;

static int run_msm(int argc, char** argv) {
  const long pinned = atol(argv[2]);
  std::vector<uint32_t> lens;
  for (int i = 3; i < argc; i++) lens.push_back((uint32_t)strtoul(argv[i], nullptr, 10));
  Tier0MsmPlan pl;
  if (!cpx::tier0_msm_plan(lens.size(), lens.data(), pl)) {
    printf("refused 1\n");
    return 0;
  }
  pl.slices = cpx::tbw_slices_rule(pinned, (int)pl.count, 2, (int)pl.max_n);
  printf("refused 0\ncount %zu\npoints %zu\nmax_n %u\nslices %d\n", pl.count, pl.points, pl.max_n, pl.slices);
  printf("conv_entries %zu\ndigit_words %zu\nsets %zu\ntail_dup %d\n", pl.conv_entries(), pl.digit_words(), pl.sets(), pl.tail_dup());
  for (size_t i = 0; i < pl.count; i++)
    printf("task %zu %u %zu %zu %zu %zu %zu\n", i, pl.conv_off[i], pl.conv_first(i), pl.digit_first(i), pl.part_first(i), pl.part_slot(i, 0, 0),
           pl.part_slot(i, 15, pl.tail_dup() - 1));
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 3 && !strcmp(argv[1], "msm")) return run_msm(argc, argv);
  if (argc == 3 && !strcmp(argv[1], "refuse")) {
    Tier0MsmPlan pl;
    printf("refused %d\n", cpx::tier0_msm_plan((size_t)strtoull(argv[2], nullptr, 10), nullptr, pl) ? 0 : 1);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "points")) {
    const std::vector<uint32_t> lens((size_t)strtoull(argv[3], nullptr, 10), (uint32_t)strtoul(argv[2], nullptr, 10));
    Tier0MsmPlan pl;
    const bool ok = cpx::tier0_msm_plan(lens.size(), lens.data(), pl);
    printf("refused %d\npoints %zu\n", ok ? 0 : 1, ok ? pl.points : (size_t)0);
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "fold")) {
    const size_t families = (size_t)strtoull(argv[2], nullptr, 10), half = (size_t)strtoull(argv[3], nullptr, 10);
    const bool fits = cpx::tier0_fold_fits(families, half);
    printf("fits %d\nquad_max %ld\n", fits ? 1 : 0, fits ? cpx::tier0_fold_quad_max(families * half, atol(argv[4]), atoi(argv[5]) != 0) : -1L);
    return 0;
  }
  fprintf(stderr, "usage: tier0_plan_emul msm|refuse|points|fold ...\n");
  return 2;
}
