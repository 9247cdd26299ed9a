// TEST-ONLY: the two-base joint ladder of the batched tracker-proof verifier on the CPU.  The schedule is the product's
// (curdleproofs_amd/csrc/tracker_ladder.hpp, the header k_tracker_relations walks); the point arithmetic is the one-lane host build of the
// g1_28.hpp additions, where the kernel uses their quad-cooperative forms.  Tables, step order and the exceptional cases (the accumulator
// meeting a table entry equal or opposite to itself) are laid out exactly as in the kernel.
#include <cstring>
#include "../../curdleproofs_amd/csrc/g1.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"
#include "../../curdleproofs_amd/csrc/glv.hpp"
#include "../../curdleproofs_amd/csrc/recode.hpp"
#include "../../curdleproofs_amd/csrc/tracker_ladder.hpp"

using namespace cpx;

namespace {
TAcc neg_of(const TAcc& a) { return a.is_identity() ? a : TAcc{a.x, t_neg(a.y), a.zz, a.zzz}; }
void build_table(const Aff& p_std, TAcc* tab) {
  const TAff P = t_from_std(p_std);
  TAcc XP = TAcc::identity(), XN = TAcc::identity();
  if (!P.is_identity()) {
    XP = TAcc{P.x, P.y, t_one(), t_one()};
    XN = TAcc{t_mul(P.x, t_beta()), t_neg(P.y), t_one(), t_one()};
  }
  tab[0] = XP;
  tab[2] = XN;
  tab[4] = t_acc_add(XP, XN);
  tab[1] = neg_of(XP);
  tab[3] = neg_of(XN);
  tab[6] = t_acc_add(XP, tab[3]);
  tab[5] = neg_of(tab[4]);
  tab[7] = neg_of(tab[6]);
}
}  // namespace

extern "C" {
// n cases: out[i] = a[i] * p1[i] + b[i] * p2[i] (Jacobian, standard form, 144 B).  Points: affine wire form (96 B, identity = zeros);
// scalars: 32 bytes little-endian canonical (< r).  adds_out (optional): how many table additions the schedule asked for, per case.
void emul_tracker_ladder(int n, const uint8_t* p1, const uint8_t* p2, const uint8_t* a, const uint8_t* b, uint8_t* out, int* adds_out) {
  for (int c = 0; c < n; c++) {
    Aff P[2];
    memcpy(&P[0], p1 + 96 * c, 96);
    memcpy(&P[1], p2 + 96 * c, 96);
    uint32_t ka[8], kb[8];
    memcpy(ka, a + 32 * c, 32);
    memcpy(kb, b + 32 * c, 32);
    SmulNaf ra, rb;
    recode_smul_glv(ka, ra);
    recode_smul_glv(kb, rb);
    TAcc slot[TL_PER_REL];
    slot[TL_ACC] = TAcc::identity();
    for (int base = 0; base < 2; base++) build_table(P[base], slot + TL_TAB + TRACKER_TABLE_ENTRIES * base);
    int adds = 0;
    for (int i = TRACKER_LADDER_TOP; i >= 0; i--) {
      slot[TL_ACC] = t_acc_dbl(slot[TL_ACC]);
      const TrackerStep st = tracker_ladder_step(ra, rb, i);
      for (int base = 0; base < 2; base++) {
        if (st.e[base] < 0) continue;
        slot[TL_ACC] = t_acc_add(slot[TL_ACC], slot[TL_TAB + TRACKER_TABLE_ENTRIES * base + st.e[base]]);
        adds++;
      }
    }
    const Jac r = t_jac_to_std(t_acc_to_jac(slot[TL_ACC]));
    memcpy(out + 144 * c, &r, 144);
    if (adds_out) adds_out[c] = adds;
  }
}
}
