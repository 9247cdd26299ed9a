// Stand-alone driver of curdleproofs_amd/csrc/check_plan.hpp for tests/test_check_plan_cpu.py: compiled with g++ (once plain, once with
// -fsanitize=address,undefined), it prints the sizes, the gather list, the four task lists and the verdict rule of one accumulated check.
//   check_plan_emul B groups_max ell L fix_parts pp_stride SUSPECTS
// SUSPECTS: B characters '0' / '1' (the proofs of the stage-2 list).  The planner only offsets base pointers, so the "device" buffers
// are plain host arrays that nothing dereferences; every address is printed as a block letter and an offset from that block's base:
//   msm <list> k  bases_off  idx_block idx_off  scalars_off  n flags conv_off      (idx_block R: row-relative list, G: global list)
//   fix <list> k  idx_is_null  scal_block scal_off  off n flags out_first          (scal_block C: per-proof CRS scalars, S: summed rows)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "../../curdleproofs_amd/csrc/check_plan.hpp"

using namespace cpx;

template <class T>
static bool inside(const std::vector<T>& v, const T* p, size_t* off) {
  if (p < v.data() || p > v.data() + v.size()) return false;
  *off = (size_t)(p - v.data());
  return true;
}

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: %s B groups_max ell L fix_parts pp_stride SUSPECTS\n", argv[0]);
    return 2;
  }
  const size_t B = strtoull(argv[1], nullptr, 10);
  const long groups_max = atol(argv[2]);
  const size_t ell = strtoull(argv[3], nullptr, 10), L = strtoull(argv[4], nullptr, 10), fp = strtoull(argv[5], nullptr, 10), stride = strtoull(argv[6], nullptr, 10);
  const std::string sus = argv[7];
  const size_t n = ell + 4;
  if (sus.size() != B) {
    fprintf(stderr, "SUSPECTS takes B = %zu characters\n", B);
    return 2;
  }
  const LocatePlan lp = locate_plan(B, groups_max), fl = CheckPlan::fused_plan(B);
  CheckPlan cp(B, ell, L, n);
  if (stride < cp.NPT) {
    fprintf(stderr, "pp_stride must hold the %zu points of a proof\n", cp.NPT);
    return 2;
  }
  std::vector<Aff> points(B * stride);
  std::vector<uint32_t> row_idx(cp.NPT), gidx(cp.n_points());
  std::vector<Fr> s_pts(cp.n_points()), s_crs(B * n), s_sums(lp.s1_crs_scalars(n));
  cp.place(points.data(), stride, row_idx.data(), gidx.data(), s_pts.data(), s_crs.data(), s_sums.data());
  printf("sizes %zu %zu %zu %zu\n", cp.NI, cp.NM, cp.NPT, cp.n_points());
  printf("plans %zu %zu %zu %zu\n", lp.G, lp.NT, fl.G, fl.NT);
  cp.gather(gidx.data());
  printf("gather");
  for (uint32_t x : gidx) printf(" %u", x);
  printf("\n");

  int bad = 0;
  auto print = [&](const char* name, const std::vector<MsmTask>& mt, const std::vector<FixTask>& ft) {
    for (size_t k = 0; k < mt.size(); k++) {
      const MsmTask& t = mt[k];
      size_t b = 0, i = 0, s = 0;
      const bool rel = t.idx == row_idx.data();
      if (!inside(points, t.bases, &b) || !(rel || inside(gidx, t.idx, &i)) || !inside(s_pts, t.scalars, &s)) bad = 1;
      printf("msm %s %zu %zu %c %zu %zu %u %u %u\n", name, k, b, rel ? 'R' : 'G', i, s, t.n, t.flags, t.conv_off);
    }
    for (size_t k = 0; k < ft.size(); k++) {
      const FixTask& t = ft[k];
      size_t s = 0;
      const bool c = inside(s_crs, t.scalars, &s), m = !c && inside(s_sums, t.scalars, &s);
      if (!c && !m) bad = 1;
      printf("fix %s %zu %d %c %zu %u %u %u %u\n", name, k, t.idx == nullptr ? 1 : 0, c ? 'C' : 'S', s, t.off, t.n, t.flags, t.out_first);
    }
  };
  {
    std::vector<MsmTask> mt(B);
    std::vector<FixTask> ft(B);
    cp.proof_tasks(fp, mt.data(), ft.data());
    print("proof", mt, ft);
  }
  {
    std::vector<MsmTask> mt(lp.NT);
    std::vector<FixTask> ft(lp.NT);
    cp.group_tasks(lp, fp, mt.data(), ft.data());
    print("groups", mt, ft);
  }
  {
    std::vector<MsmTask> mt(fl.NT);
    std::vector<FixTask> ft(1);
    cp.fused_tasks(mt.data(), ft.data());
    print("fused", mt, ft);
  }
  {
    std::vector<uint32_t> list;
    for (size_t p = 0; p < B; p++)
      if (sus[p] == '1') list.push_back((uint32_t)p);
    std::vector<MsmTask> mt(list.size());
    std::vector<FixTask> ft(list.size());
    cp.suspect_tasks(list, fp, mt.data(), ft.data());
    print("suspects", mt, ft);
  }
  for (uint32_t f = 0; f < 4; f++)
    for (int passed = 0; passed < 2; passed++) printf("verdict %u %d %d\n", f, passed, check_verdict(f, passed != 0));
  if (bad) fprintf(stderr, "a task points outside the buffers it was given\n");
  return bad;
}
