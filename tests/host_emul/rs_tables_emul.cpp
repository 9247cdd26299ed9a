// TEST-ONLY: the two request lists that take the prover's R and S from the per-proof tables (curdleproofs_amd/csrc/prove_reqs.hpp:
// prove_rs_tables, prove_rs_sums) compiled for the CPU and flattened into integers; the assertions are in tests/test_rs_tables_cpu.py.
#include <cstdint>
#include "../../curdleproofs_amd/csrc/prove_reqs.hpp"

using namespace cpx;

extern "C" {

// which: 0 = prove_rs_tables, 1 = prove_rs_sums, 2 = prove_phase1t, 3 = prove_phase1.  out: 17 ints per request — seg0 {kind, gather, off,
// n, arg}, seg1 {..}, scalars {kind, at}, keep, out, add[3].  Returns the number of requests.
int rs_list(int which, int n, int L, int32_t* out) {
  const ReqList l = which == 0 ? prove_rs_tables(n, L) : which == 1 ? prove_rs_sums(n, L) : which == 2 ? prove_phase1t(n, L) : prove_phase1(n, L);
  for (int i = 0; i < l.n; i++) {
    const ReqDesc& d = l.r[i];
    const int32_t v[17] = {d.seg0.kind, d.seg0.gather, d.seg0.off, d.seg0.n, d.seg0.arg, d.seg1.kind, d.seg1.gather, d.seg1.off, d.seg1.n, d.seg1.arg,
                           d.scal.kind, d.scal.at,     d.keep,     d.out,    d.add[0],   d.add[1],    d.add[2]};
    for (int k = 0; k < 17; k++) out[17 * i + k] = v[k];
  }
  return l.n;
}

// the names the assertions are written in, in the order of NAMES in the test
int rs_consts(int n, int L, int32_t* o) {
  const SlotMap sm(L);
  const PtabRow row(n);
  const RandIdx ri(n);
  const int32_t v[] = {SL_R,      SL_S,     SL_CMT2,  SL_CMU2,  sm.CMA2(),   sm.CMB2(),  sm.TMP(0), sm.count(), sm.D(),     row.T(),  row.U(),    row.count(), V_APERM, V_COUNT,
                       SEG_NONE,  SEG_PTAB, GA_NONE,  SCAL_NONE, SCAL_VEC,   SC_K_INV,   SC_RK_K_INV, SC_XFIN,  SC_COUNT,   ri.RK(),  rs_tables_slot(L, 0), rs_tables_slot(L, 1),
                       (int32_t)N_BLINDERS};
  const int cnt = (int)(sizeof v / sizeof v[0]);
  for (int i = 0; i < cnt; i++) o[i] = v[i];
  return cnt;
}
void rs_side_slots(int L, int32_t* q) { side_stream_slots(L, q); }
}
