// g++ program over curdleproofs_amd/csrc/find_plan.hpp (tests/test_find_trackers_cpu.py): the plan of cpx_whisk_find_trackers exactly as
// Engine::whisk_find_trackers and launch_find_scan use it, printed as plain "key value..." lines.
//   find_plan_emul fits <n_trackers> <n_keys>                          the limits of a call
//   find_plan_emul plan <n_trackers> <n_keys> <min_keys> <table_mb>    path, chunks, bytes, grids, and the wave map walked over every chunk:
//                                                                      how often each (tracker, key) pair is taken by a lane
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/find_plan.hpp"

using cpx::FindPlan;

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "fits")) {
    printf("fits %d\n", cpx::find_fits((size_t)strtoull(argv[2], nullptr, 10), (size_t)strtoull(argv[3], nullptr, 10)) ? 1 : 0);
    return 0;
  }
  if (argc == 6 && !strcmp(argv[1], "plan")) {
    const size_t n = (size_t)strtoull(argv[2], nullptr, 10), nk = (size_t)strtoull(argv[3], nullptr, 10);
    const long mb = atol(argv[5]);
    const FindPlan pl = cpx::find_plan(n, nk, atol(argv[4]), mb);
    printf("table %d\nchunk_cols %zu\nn_chunks %zu\nfix_chunk %d\nbudget %zu\n", pl.table ? 1 : 0, pl.chunk_cols, pl.n_chunks, pl.fix_chunk, (size_t)mb << 20);
    if (!pl.table) return 0;
    printf("next_bytes %zu\n", FindPlan::chunk_bytes(pl.chunk_cols + 1, pl.fix_chunk));
    std::vector<uint8_t> taken(n * nk, 0);
    size_t lanes_out_of_range = 0, sum = 0;
    for (size_t c = 0; c < pl.n_chunks; c++) {
      const size_t first = pl.chunk_first(c), nc = pl.chunk_size(c), waves = pl.scan_waves(nc);
      printf("chunk %zu %zu %zu %zu %zu %zu %zu %zu\n", c, first, nc, FindPlan::chunk_bytes(nc, pl.fix_chunk), FindPlan::table_entries(nc), FindPlan::shift_entries(nc),
             FindPlan::tmp_entries(nc, pl.fix_chunk), waves);
      sum += nc;
      for (size_t g = 0; g < waves; g++) {
        const cpx::FindWave w = pl.wave(g);
        for (size_t lane = 0; lane < (size_t)cpx::FIND_WAVE_COLS; lane++) {
          const size_t col = w.col0 + lane;
          if (col >= nc) continue;   // a dead lane
          if (w.key >= nk || first + col >= n) {
            lanes_out_of_range++;
            continue;
          }
          if (taken[(first + col) * nk + w.key] < 255) taken[(first + col) * nk + w.key]++;
        }
      }
    }
    size_t once = 0;
    for (uint8_t t : taken) once += t == 1;
    printf("columns %zu\npairs %zu\npairs_taken_once %zu\nlanes_out_of_range %zu\n", sum, n * nk, once, lanes_out_of_range);
    return 0;
  }
  fprintf(stderr, "usage: find_plan_emul fits|plan ...\n");
  return 2;
}
