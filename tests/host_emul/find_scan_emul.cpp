// TEST-ONLY: the table path of cpx_whisk_find_trackers on the CPU.  Layout, recoding and the per-pair body are the product's
// (curdleproofs_amd/csrc/find_plan.hpp, the body k_find_scan runs); the table is built here with the one-lane host build of the g1_28.hpp
// formulas: column c holds m * 256^w * base_c at entry (w * 128 + m - 1) * nc + c, as k_table_build + k_fix_build<8> leave it.
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/g1.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"
#include "../../curdleproofs_amd/csrc/find_plan.hpp"

using namespace cpx;

namespace {
std::vector<TFix> g_tab;
size_t g_nc = 0;
TAff normalise(const TJac& p) { return p.is_identity() ? TAff::identity() : t_to_affine(p, t_inv(p.z)); }
}  // namespace

extern "C" {
void emul_find_consts(int out[4]) {
  out[0] = FIND_WINDOWS;
  out[1] = FIND_MULT;
  out[2] = FIND_WAVE_COLS;
  out[3] = (int)sizeof(TFix);
}
// the 32 digits of n canonical keys (32 bytes little-endian each)
void emul_find_digits(int n, const uint8_t* keys, int* digits) {
  for (int j = 0; j < n; j++) {
    uint32_t k[8];
    memcpy(k, keys + 32 * j, 32);
    FindDigits dg;
    find_recode(k, dg);
    for (int w = 0; w < FIND_WINDOWS; w++) digits[j * FIND_WINDOWS + w] = find_digit(dg, w);
  }
}
long emul_find_entry(int w, int d, long nc, long col) { return (long)find_entry(w, d, (size_t)nc, (size_t)col); }
// bases: nc affine points, standard form (96 B each; 96 zero bytes = the identity)
void emul_find_build(int nc, const uint8_t* bases) {
  g_nc = (size_t)nc;
  g_tab.assign(FindPlan::table_entries(g_nc), TFix{TAff::identity()});
  for (int c = 0; c < nc; c++) {
    Aff b;
    memcpy(&b, bases + 96 * c, 96);
    TAff S = t_from_std(b);   // 256^w * base
    for (int w = 0; w < FIND_WINDOWS; w++) {
      TJac acc = TJac::identity();
      for (int m = 1; m <= FIND_MULT; m++) {
        acc = t_add_mixed(acc, S);
        g_tab[find_entry(w, m, g_nc, (size_t)c)].a = normalise(acc);
      }
      TJac sh = TJac::from_affine(S);
      for (int s = 0; s < 8; s++) sh = t_dbl(sh);
      S = normalise(sh);
    }
  }
}
void emul_find_table_entry(long e, uint8_t out96[96]) {
  const Aff a = t_to_std(g_tab[(size_t)e].a);
  memcpy(out96, &a, 96);
}
// match[j * nc + c] = does canonical key j open column c against the claimed point claimed[j * nc + c] (96 B, standard form)?  ok[c] = the
// column's tracker decoded
void emul_find_pairs(int n_keys, const uint8_t* keys, const uint8_t* claimed, const uint8_t* ok, int* match) {
  for (int j = 0; j < n_keys; j++) {
    uint32_t k[8];
    memcpy(k, keys + 32 * j, 32);
    FindDigits dg;
    find_recode(k, dg);
    for (size_t c = 0; c < g_nc; c++) {
      Aff cl;
      memcpy(&cl, claimed + 96 * ((size_t)j * g_nc + c), 96);
      match[(size_t)j * g_nc + c] = find_pair_matches<false>(dg, g_tab.data(), g_nc, c, true, t_from_std(cl), ok[c] != 0) ? 1 : 0;
    }
  }
}
}
