// Stand-alone driver of curdleproofs_amd/csrc/locate_plan.hpp for tests/test_verify_grouped_cpu.py: compiled with g++ (once plain, once with
// -fsanitize=address,undefined), it prints the groups, the stage-2 list, the verdict map and the buffer sizes of one grouped verification.
//   locate_plan_emul B groups_max NPT n fix_parts1 fix_parts2 slices FLAGS GROUP_OK OWN_OK
// FLAGS: B characters '0'..'3' (the proofs' flag words), GROUP_OK: NT characters '0' / '1' (stage 1's results), OWN_OK: B characters
// '0' / '1' (what a proof's own check says, looked at for the proofs stage 2 rechecks only).  B = 0: the three strings are "-".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../../curdleproofs_amd/csrc/locate_plan.hpp"

using namespace cpx;

int main(int argc, char** argv) {
  if (argc != 11) {
    fprintf(stderr, "usage: %s B groups_max NPT n fix_parts1 fix_parts2 slices FLAGS GROUP_OK OWN_OK\n", argv[0]);
    return 2;
  }
  const size_t B = strtoull(argv[1], nullptr, 10);
  const long groups_max = atol(argv[2]);
  const size_t NPT = strtoull(argv[3], nullptr, 10), n = strtoull(argv[4], nullptr, 10), fp1 = strtoull(argv[5], nullptr, 10), fp2 = strtoull(argv[6], nullptr, 10),
               slices = strtoull(argv[7], nullptr, 10);
  const LocatePlan pl = locate_plan(B, groups_max);
  const std::string sf = B ? argv[8] : "", sg = B ? argv[9] : "", so = B ? argv[10] : "";
  if (sf.size() != B || sg.size() != pl.NT || so.size() != B) {
    fprintf(stderr, "FLAGS and OWN_OK take B = %zu characters, GROUP_OK NT = %zu\n", B, pl.NT);
    return 2;
  }
  std::vector<uint32_t> flags(B);
  std::vector<uint8_t> group_ok(pl.NT);
  for (size_t p = 0; p < B; p++) flags[p] = (uint32_t)(sf[p] - '0');
  for (size_t g = 0; g < pl.NT; g++) group_ok[g] = sg[g] == '1';
  printf("plan %zu %zu %zu %d\n", pl.B, pl.G, pl.NT, pl.per_proof() ? 1 : 0);
  for (size_t g = 0; g < pl.NT; g++)
    printf("group %zu %zu %zu %zu %zu %zu\n", g, pl.group_first(g), pl.group_count(g), pl.s1_task_off(g, NPT), pl.s1_task_n(g, NPT), pl.s1_out_first(g, fp1));
  printf("beyond %zu\n", pl.group_count(pl.NT));   // a group past the end holds nothing
  printf("sizes1 %zu %zu %zu %zu %zu %zu %zu %zu\n", pl.s1_max_n(NPT), pl.s1_points(NPT), pl.s1_crs_scalars(n), LocatePlan::conv_entries(pl.NT, pl.s1_max_n(NPT)),
         LocatePlan::digit_words(pl.NT, pl.s1_max_n(NPT)), LocatePlan::bucket_parts(pl.NT, slices), LocatePlan::fix_part_slots(pl.NT, fp1), LocatePlan::result_bytes(pl.NT));
  std::vector<uint32_t> list;
  locate_stage2(pl, group_ok.data(), flags.data(), list);
  std::vector<uint8_t> recheck_ok(list.size());
  for (size_t s = 0; s < list.size(); s++) {
    printf("stage2 %zu %u %zu %zu %zu\n", s, list[s], pl.group_of(list[s]), LocatePlan::s2_conv_off(s, NPT), LocatePlan::s2_out_first(s, fp2));
    recheck_ok[s] = so[list[s]] == '1';
  }
  const size_t S = list.size();
  printf("sizes2 %zu %zu %zu %zu %zu %zu\n", S, LocatePlan::conv_entries(S, NPT), LocatePlan::digit_words(S, NPT), LocatePlan::bucket_parts(S, slices),
         LocatePlan::fix_part_slots(S, fp2), LocatePlan::result_bytes(S));
  std::vector<int> verdict(B, CPX_ERR_INTERNAL);
  locate_verdicts(pl, group_ok.data(), flags.data(), list, recheck_ok.data(), verdict.data());
  printf("verdicts");
  for (size_t p = 0; p < B; p++) printf(" %d", verdict[p]);
  printf("\n");
  return 0;
}
