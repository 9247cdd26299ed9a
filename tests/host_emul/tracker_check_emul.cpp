// Stand-alone driver of curdleproofs_amd/csrc/tracker_check_plan.hpp for tests/test_tracker_grouped_cpu.py: the g++ build of the text that
// hipcc compiles into k_tracker_check_scalars and that Engine::tracker_check lays its tasks out by.
//   tracker_check_emul plan COUNT GROUPS_MAX            the plan, every group's task, the sizes
//   tracker_check_emul slots COUNT GROUPS_MAX P...      the five slots of the listed items
//   tracker_check_emul scalars                          stdin: lines "a b s c" (canonical integers, 64 hex digits each); stdout: per line the
//                                                       five terms (k_G, A, r_G, k_r_G, B) and the generator term, canonical hex
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../../curdleproofs_amd/csrc/tracker_check_plan.hpp"

using namespace cpx;

static bool parse_fr(const char* hex, Fr& out) {
  if (strlen(hex) != 64) return false;
  for (int i = 0; i < 8; i++) {
    char w[9];
    memcpy(w, hex + 8 * (7 - i), 8);   // most significant digits first in the text, little-endian limbs in memory
    w[8] = 0;
    char* end = nullptr;
    out.v[i] = (uint32_t)strtoul(w, &end, 16);
    if (*end) return false;
  }
  return true;
}
static void print_fr(const Fr& mont) {
  const Fr c = fe_from_mont(mont);
  for (int i = 7; i >= 0; i--) printf("%08x", c.v[i]);
}

int main(int argc, char** argv) {
  if (argc >= 4 && (!strcmp(argv[1], "plan") || !strcmp(argv[1], "slots"))) {
    const size_t count = strtoull(argv[2], nullptr, 10);
    const TrackerCheckPlan pl = tracker_check_plan(count, atol(argv[3]));
    if (!strcmp(argv[1], "plan")) {
      printf("plan %zu %zu %zu %d\n", pl.count(), pl.lp.G, pl.tasks(), tracker_check_fits(count) ? 1 : 0);
      for (size_t g = 0; g < pl.tasks(); g++) printf("group %zu %zu %zu %zu %zu %zu\n", g, pl.lp.group_first(g), pl.lp.group_count(g), pl.task_off(g), pl.task_n(g), pl.gen_slot(g));
      printf("sizes %zu %zu %zu %zu %zu %zu\n", pl.max_n(), pl.points(), pl.input_bytes(), pl.weight_scalars(), pl.result_points(), (size_t)kTrackerCheckMax);
      printf("planes %d %d %d %d %d\n", tck_plane(TCK_K_G), tck_plane(TCK_A), tck_plane(TCK_R_G), tck_plane(TCK_K_R_G), tck_plane(TCK_B));
      const TrackerInputLayout in = tracker_input_layout(count);
      printf("layout %zu %zu %zu %zu", in.trackers, in.k_commitments, in.proofs, in.bytes);
      for (int q = 0; q < TCK_PLANES; q++) printf(" %zu %zu", in.plane_off[q], in.plane_rec[q]);
      printf("\n");
      return 0;
    }
    for (int i = 4; i < argc; i++) {
      const size_t p = strtoull(argv[i], nullptr, 10);
      if (p >= count) return 2;
      printf("slots %zu", p);
      for (int j = 0; j < TCK_TERMS; j++) printf(" %zu", pl.slot(p, j));
      printf("\n");
    }
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "scalars")) {
    char a[80], b[80], s[80], c[80];
    while (scanf("%79s %79s %79s %79s", a, b, s, c) == 4) {
      Fr fa, fb, fs, fc;
      if (!parse_fr(a, fa) || !parse_fr(b, fb) || !parse_fr(s, fs) || !parse_fr(c, fc)) return 2;
      const TrackerCheckScalars sc = tracker_check_scalars(fe_to_mont(fa), fe_to_mont(fb), fe_to_mont(fs), fe_to_mont(fc));
      for (int j = 0; j < TCK_TERMS; j++) {
        print_fr(sc.term[j]);
        printf(" ");
      }
      print_fr(sc.gen);
      printf("\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: %s plan COUNT GROUPS_MAX | slots COUNT GROUPS_MAX P... | scalars < lines\n", argv[0]);
  return 2;
}
