// TEST-ONLY: the request lists of the protocol (curdleproofs_amd/csrc/prove_reqs.hpp) compiled for the CPU and flattened into integer
// arrays; the assertions are in tests/test_prove_reqs_cpu.py.  The names of layout.hpp and protocol.h the assertions are written in
// come from pr_consts.
#include <cstdint>
#include "../../curdleproofs_amd/csrc/prove_reqs.hpp"

using namespace cpx;

extern "C" {

// phase: 0 = 1b, 1 = 1, 2 = 1t, 3 = 2, 4 = 2 with B in commitment form, 5 = 3, 6 = IPA round j, 7 = the same, fused, 8 = SameMSM round j,
// 9 = the verifier's.  out: 17 ints per request — seg0 {kind, gather, off, n, arg}, seg1 {..}, scalars {kind, at}, keep, out, add[3].
// Returns the number of requests; *round_stride: the entries of a proof's row of round scalars.
int pr_list(int phase, int n, int L, int j, int32_t* out, int32_t* round_stride) {
  ReqList l;
  switch (phase) {
    case 0: l = prove_phase1b(n, L); break;
    case 1: l = prove_phase1(n, L); break;
    case 2: l = prove_phase1t(n, L); break;
    case 3: l = prove_phase2(n, L, false); break;
    case 4: l = prove_phase2(n, L, true); break;
    case 5: l = prove_phase3(n, L); break;
    case 6: l = prove_ipa_round(n, L, j, false); break;
    case 7: l = prove_ipa_round(n, L, j, true); break;
    case 8: l = prove_smsm_round(n, L, j); break;
    case 9: l = verify_requests(n, L); break;
    default: return -1;
  }
  for (int i = 0; i < l.n; i++) {
    const ReqDesc& d = l.r[i];
    const int32_t v[17] = {d.seg0.kind, d.seg0.gather, d.seg0.off, d.seg0.n, d.seg0.arg, d.seg1.kind, d.seg1.gather, d.seg1.off, d.seg1.n, d.seg1.arg,
                           d.scal.kind, d.scal.at,     d.keep,     d.out,    d.add[0],   d.add[1],    d.add[2]};
    for (int k = 0; k < 17; k++) out[17 * i + k] = v[k];
  }
  *round_stride = l.round_stride;
  return l.n;
}

// the list phase 1b then phase 1, as both paths issue it when A leads the phase: the number of requests and their `out` slots
int pr_then(int n, int L, int32_t* outs) {
  const ReqList l = prove_phase1b(n, L).then(prove_phase1(n, L));
  for (int i = 0; i < l.n; i++) outs[i] = l.r[i].out;
  return l.n;
}

int pr_gather(int n, int gather, int arg, uint32_t* out) { return gather_list(n, gather, arg, out); }
void pr_side_slots(int L, int32_t* q) { side_stream_slots(L, q); }
void pr_basis(int n, uint32_t* cols) { CtabCols(n).same_msm_basis(cols); }
int pr_slot_round(int L, int which, int j) {   // LC RC LD RD LA LT LU RA RT RU
  const SlotMap sm(L);
  const int s[10] = {sm.LC(j), sm.RC(j), sm.LD(j), sm.RD(j), sm.LA(j), sm.LT(j), sm.LU(j), sm.RA(j), sm.RT(j), sm.RU(j)};
  return s[which];
}

// the names the tables of the request lists are written in (layout.hpp, protocol.h, prove_reqs.hpp), in the order of NAMES in the test
int pr_consts(int n, int L, int32_t* o) {
  const SlotMap sm(L);
  const RandIdx ri(n);
  const PtabRow row(n);
  const CtabCols cc(n);
  const int32_t v[] = {SL_A, SL_CMT1, SL_CMT2, SL_CMU1, SL_CMU2, SL_R, SL_S, SL_B, SL_C, SL_BC, SL_BD, sm.CMA1(), sm.CMA2(), sm.CMB1(), sm.CMB2(), sm.BA(), sm.BT(), sm.BU(),
                       sm.D(), sm.APRIME(), sm.TMP(0), sm.count(), ProofLayout(L).n_points(),
                       ri.VR(), ri.IR(), ri.RT(), ri.RU(), ri.RA(), ri.RB(), ri.count(),
                       row.M(), row.T(), row.U(), cc.H(), cc.G_t(), cc.G_u(), cc.G_sum(), cc.H_sum(),
                       V_APERM, V_FACT, V_C, V_ZZU, V_COUNT, SC_BETA_SP, SC_ALPHA_SP, SC_NEG_BETA_G_INV, SC_ALPHA_G, SC_COUNT, VSC_NEG_BETA_G_INV, VSC_ALPHA_G, VSC_COUNT,
                       SEG_NONE, SEG_CRS, SEG_PTAB, GA_NONE, GA_BASIS, GA_HI, GA_LO, GA_BASIS_HI, GA_BASIS_LO, GA_COL, GA_HI_H, GA_LO_H,
                       SCAL_NONE, SCAL_RAND, SCAL_VEC, SCAL_SC, SCAL_ROUND};
  const int cnt = (int)(sizeof v / sizeof v[0]);
  for (int i = 0; i < cnt; i++) o[i] = v[i];
  return cnt;
}
}
