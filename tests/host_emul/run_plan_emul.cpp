// g++ twin of curdleproofs_amd/csrc/run_plan.hpp (tests/test_whisk_run_cpu.py): the source list, the commit list, the index check and the
// lane layout of the Whisk shuffle run, run on the CPU exactly as whisk.cpp and run.hip call them.  A stand-alone program, so that it can be
// built with -fsanitize=address,undefined as it is: every array below has exactly the size the engine gives it.
//
//   stdin:  count ell n n_applied, then count * ell indices
//   stdout: valid 0|1; for a valid table  src <count*ell entries>  |  commit <len>  |  dst <len>  |  pos <len>  |  lanes <0|1>
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../curdleproofs_amd/csrc/run_plan.hpp"

using namespace cpx;

static void line(const char* key, const std::vector<uint32_t>& v, size_t len) {
  printf("%s", key);
  for (size_t i = 0; i < len; i++) printf(" %u", v[i]);
  printf("\n");
}

int main() {
  unsigned count = 0, ell = 0, n = 0, n_applied = 0;
  if (scanf("%u %u %u %u", &count, &ell, &n, &n_applied) != 4) return 2;
  const RunPlan rp(count, ell, n);
  const size_t pp = rp.reads();
  std::vector<uint32_t> indices(pp);
  for (size_t g = 0; g < pp; g++)
    if (scanf("%u", &indices[g]) != 1) return 2;
  const bool valid = rp.indices_valid(indices.data());
  printf("valid %d\n", valid ? 1 : 0);
  if (!valid) return 0;   // the engine refuses the call here: nothing below ever sees such a table
  std::vector<uint32_t> src(pp), last(n), dst((size_t)(n_applied < count ? n_applied : count) * ell), pos(dst.size());
  rp.resolve(indices.data(), src.data(), last.data());
  line("src", src, pp);
  const size_t len = rp.commit_list(indices.data(), n_applied, dst.data(), pos.data(), last.data());
  printf("commit %zu\n", len);
  line("dst", dst, len);
  line("pos", pos, len);
  // the copy kernels' grid: every (point, piece) of pp points is some lane's, exactly once, and a wave's lanes of one point are neighbours
  std::vector<uint8_t> hit(pp * RUN_POINT_CHUNKS);
  bool ok = true;
  for (size_t b = 0; b < run_copy_blocks(pp); b++)
    for (uint32_t t = 0; t < RUN_BLOCK_THREADS; t++) {
      const size_t g = run_lane_point(b, t);
      const uint32_t c = run_lane_chunk(t);
      if (g >= pp) continue;   // (the kernels' own bound)
      ok &= c < RUN_POINT_CHUNKS && hit[g * RUN_POINT_CHUNKS + c]++ == 0;
      if (c) ok &= run_lane_point(b, t - 1) == g && run_lane_chunk(t - 1) == c - 1;
    }
  for (uint8_t h : hit) ok &= h == 1;
  printf("lanes %d\n", ok ? 1 : 0);
  return 0;
}
