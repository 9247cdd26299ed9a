// TEST-ONLY: the fixed-base table of the G1 generator on the CPU.  Layout, window width and recoding are the product's
// (curdleproofs_amd/csrc/gen_table.hpp, the header k_gen_table / k_gen_mul walk); the point arithmetic is the one-lane host build of the
// g1_28.hpp formulas the kernels use.  The table is built and walked exactly as in genmul.hip.
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/g1.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"
#include "../../curdleproofs_amd/csrc/glv.hpp"
#include "../../curdleproofs_amd/csrc/gen_table.hpp"

using namespace cpx;

namespace {
std::vector<TAff> g_tab;
}

extern "C" {
// windows per half, largest digit magnitude below the top window, largest top digit, table entries, additions per scalar, bytes per entry
void emul_gen_consts(int out[6]) {
  out[0] = GEN_WINDOWS;
  out[1] = GEN_DIGIT_MAX;
  out[2] = GEN_TOP_DIGIT_MAX;
  out[3] = GEN_TABLE_ENTRIES;
  out[4] = GEN_MAX_ADDS;
  out[5] = (int)sizeof(TAff);
}
// entry e of the table is the multiple mult[e] * 256^window[e] of the generator; capacity[w] = gen_window_entries(w)
void emul_gen_layout(int* window, int* mult, int* capacity) {
  for (int e = 0; e < GEN_TABLE_ENTRIES; e++) {
    window[e] = gen_entry_window(e);
    mult[e] = gen_entry_multiple(e);
  }
  for (int w = 0; w < GEN_WINDOWS; w++) capacity[w] = gen_window_entries(w);
}
// n canonical scalars (32 bytes little-endian, < r).  Per scalar: halves = |t| (16 B LE) || q (16 B LE); signs = neg_k, neg_t (glv_split);
// index / neg [2][GEN_WINDOWS]: gen_pick of every (half, window), index -1 for a zero digit.
void emul_gen_recode(int n, const uint8_t* scalars, uint8_t* halves, int* signs, int* index, int* neg) {
  for (int c = 0; c < n; c++) {
    uint32_t k[8], t[4], q[4], nk, nt;
    memcpy(k, scalars + 32 * c, 32);
    glv_split(k, t, q, nk, nt);
    memcpy(halves + 32 * c, t, 16);
    memcpy(halves + 32 * c + 16, q, 16);
    signs[2 * c] = (int)nk;
    signs[2 * c + 1] = (int)nt;
    GenDigits d;
    gen_recode(k, d);
    for (int h = 0; h < 2; h++)
      for (int w = 0; w < GEN_WINDOWS; w++) {
        const GenPick p = gen_pick(d, h, w);
        index[(c * 2 + h) * GEN_WINDOWS + w] = p.index;
        neg[(c * 2 + h) * GEN_WINDOWS + w] = p.neg ? 1 : 0;
      }
  }
}
// k_gen_table: entry e = j 256^w G by an 8-step double-and-add and 8 w doublings (here one inversion per entry)
void emul_gen_table_build(const uint8_t gen96[96]) {
  Aff g;
  memcpy(&g, gen96, 96);
  const TAff G = t_from_std(g);
  g_tab.resize(GEN_TABLE_ENTRIES);
  for (int e = 0; e < GEN_TABLE_ENTRIES; e++) {
    const int j = gen_entry_multiple(e), w = gen_entry_window(e);
    TJac acc = TJac::identity();
    for (int b = GEN_WINDOW_BITS - 1; b >= 0; b--) {
      acc = t_dbl(acc);
      if ((j >> b) & 1) acc = t_add_mixed(acc, G);
    }
    for (int i = 0; i < GEN_WINDOW_BITS * w; i++) acc = t_dbl(acc);
    g_tab[e] = t_to_affine(acc, t_inv(acc.z));
  }
}
void emul_gen_table_entry(int e, uint8_t out96[96]) {
  const Aff a = t_to_std(g_tab[e]);
  memcpy(out96, &a, 96);
}
// k_gen_mul: out[i] = scalars[i] G (Jacobian, standard form, 144 B) for n canonical scalars; adds_out (optional): non-zero picks per scalar
void emul_gen_mul(int n, const uint8_t* scalars, uint8_t* out, int* adds_out) {
  for (int c = 0; c < n; c++) {
    uint32_t k[8];
    memcpy(k, scalars + 32 * c, 32);
    GenDigits dg;
    gen_recode(k, dg);
    TAcc acc = TAcc::identity();
    int adds = 0;
    for (int w = 0; w < GEN_WINDOWS; w++)
      for (int h = 0; h < 2; h++) {
        const GenPick pk = gen_pick(dg, h, w);
        const int idx = pk.index < 0 ? 0 : (pk.index < GEN_TABLE_ENTRIES ? pk.index : GEN_TABLE_ENTRIES - 1);
        TAff e = g_tab[idx];
        if (h) e.x = t_mul(e.x, t_beta());
        e = t_cneg(e, pk.neg != (h == 1));
        if (pk.index < 0) e = TAff::identity();
        else adds++;
        acc = t_acc_add_mixed(acc, e);
      }
    const Jac r = t_jac_to_std(t_acc_to_jac(acc));
    memcpy(out + 144 * c, &r, 144);
    if (adds_out) adds_out[c] = adds;
  }
}
}
