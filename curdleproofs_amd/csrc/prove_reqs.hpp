// The table-backed MSM requests of the protocol, phase by phase — the "all-MSM" formulation (engine.cpp, above create_masked_stream)
// written down ONCE, in protocol terms: which CRS columns or per-proof table row a request reads and through which gather list, which
// scalars it uses, which points of earlier phases it adds, where its affine point is kept and which slot receives its compressed
// bytes.  Host code without a HIP call and without a pointer: Engine::make_reqs turns a list into the TblReq of tbl_plan.hpp for the
// host-driven prover / verifier (engine.cpp) and for the device-resident plans (engine_device.cpp), which differ only in where a
// request's scalars live.  tests/test_prove_reqs_cpu.py compiles it for the CPU.
#pragma once
#include <stdint.h>
#include "layout.hpp"
#include "protocol.h"

namespace cpx {

// ---- a base segment: `n` points from column / row entry `off` on, or — with a gather list — the list's n entries (off stays 0) ----
enum SegKind : uint8_t { SEG_NONE = 0, SEG_CRS, SEG_PTAB };   // nothing | columns of the CRS tables (CtabCols) | a proof's table row (PtabRow)
// the closed set of gather lists; `arg` is the column of GA_COL and the bit `half` = n >> (j + 1) of round j for the others that take one.
// "hi": the indices k < n with k & half set, "lo": the rest; BASIS: CtabCols::same_msm_basis (alone, or applied to hi / lo);
// GA_HI_H / GA_LO_H: hi / lo followed by the column H — the fused form of an IPA round
enum Gather : uint8_t { GA_NONE = 0, GA_BASIS, GA_HI, GA_LO, GA_BASIS_HI, GA_BASIS_LO, GA_COL, GA_HI_H, GA_LO_H };
struct ReqSeg {
  uint8_t kind = SEG_NONE, gather = GA_NONE;
  int off = 0, n = 0, arg = 0;
};
// the entries of a gather list (at most n + 1) into `out`; returns their number (0: GA_NONE)
inline int gather_list(int n, int gather, int arg, uint32_t* out) {
  const CtabCols cc(n);
  int cnt = 0;
  if (gather == GA_COL) out[cnt++] = (uint32_t)arg;
  if (gather == GA_BASIS) cc.same_msm_basis(out), cnt = n;
  if (gather == GA_HI || gather == GA_LO || gather == GA_HI_H || gather == GA_LO_H || gather == GA_BASIS_HI || gather == GA_BASIS_LO) {
    const bool hi = gather == GA_HI || gather == GA_HI_H || gather == GA_BASIS_HI;
    for (int k = 0; k < n; k++)
      if (((k & arg) != 0) == hi) out[cnt++] = (uint32_t)k;
    if (gather == GA_BASIS_HI || gather == GA_BASIS_LO)   // (the basis is the identity below n - 2)
      for (int i = 0; i < cnt; i++) out[i] = out[i] == (uint32_t)n - 2 ? (uint32_t)cc.G_t() : out[i] == (uint32_t)n - 1 ? (uint32_t)cc.G_u() : out[i];
    if (gather == GA_HI_H || gather == GA_LO_H) out[cnt++] = (uint32_t)cc.H();
  }
  return cnt;
}

// ---- where the seg0.n + seg1.n scalars of a request are (seg1's follow seg0's), named as protocol.h and layout.hpp name them ----
enum ScalKind : uint8_t {
  SCAL_NONE = 0,
  SCAL_RAND,    // from draw `at` of the RandIdx row on
  SCAL_VEC,     // vector V_* = at
  SCAL_SC,      // from small scalar SC_* (the verifier: VSC_*) = at on
  SCAL_ROUND    // from entry `at` of the proof's row of round scalars on (ReqList::round_stride entries per proof)
};
struct ReqScal {
  uint8_t kind = SCAL_NONE;
  int at = 0;
};

struct ReqDesc {
  ReqSeg seg0, seg1;
  ReqScal scal;
  int keep = -1;             // SlotMap slot that keeps the affine point, or none
  int out = -1;              // slot that receives the compressed bytes, or none
  int add[3] = {-1, -1, -1};   // slots of kept points of earlier phases, added with coefficient 1
};

// the requests of one proof in one phase, in the order both paths issue them
struct ReqList {
  enum { MAX = 12 };
  int n = 0;
  int round_stride = 0;      // SCAL_ROUND: entries of a proof's row
  ReqDesc r[MAX];
  ReqDesc& push(ReqSeg s0, ReqScal sc, int out, int keep = -1) {
    ReqDesc& d = r[n++];
    d.seg0 = s0, d.scal = sc, d.out = out, d.keep = keep;
    return d;
  }
  ReqList then(const ReqList& o) const {   // this list's requests, then o's
    ReqList l = *this;
    for (int i = 0; i < o.n; i++) l.r[l.n++] = o.r[i];
    return l;
  }
};

namespace rq {
inline ReqSeg crs(int off, int n) { return ReqSeg{SEG_CRS, GA_NONE, off, n, 0}; }
inline ReqSeg crs_col(int col) { return ReqSeg{SEG_CRS, GA_COL, 0, 1, col}; }
inline ReqSeg crs_gather(int gather, int n, int arg = 0) { return ReqSeg{SEG_CRS, (uint8_t)gather, 0, n, arg}; }
inline ReqSeg ptab(int off, int n, int gather = GA_NONE, int arg = 0) { return ReqSeg{SEG_PTAB, (uint8_t)gather, off, n, arg}; }
inline ReqScal rand(int i) { return ReqScal{SCAL_RAND, i}; }
inline ReqScal vec(int v) { return ReqScal{SCAL_VEC, v}; }
inline ReqScal sc(int i) { return ReqScal{SCAL_SC, i}; }
inline ReqScal round(int at) { return ReqScal{SCAL_ROUND, at}; }
inline void add3(ReqDesc& d, int a, int b = -1, int c = -1) { d.add[0] = a, d.add[1] = b, d.add[2] = c; }
}  // namespace rq

// ---- the prover (n = ell + 4 bases, L = log2 n rounds) ----
// phase 1b: A = msm(G | Hvec, a_sigma | blinders) (curdleproofs.rs:93) — the one commitment of phase 1 that needs vec_a; kept: B and A' add it
inline ReqList prove_phase1b(int n, int) {
  ReqList l;
  l.push(rq::crs(0, n), rq::vec(V_APERM), SL_A, SL_A);
  return l;
}
// phase 1: what depends on the prover's randomness only (curdleproofs.rs:110-116, same_multiscalar_argument.rs:80,
// inner_product_argument.rs:126, same_scalar_argument.rs:60-61)
inline ReqList prove_phase1(int n, int L) {
  const SlotMap sm(L);
  const RandIdx ri(n);
  const CtabCols cc(n);
  ReqList l;
  l.push(rq::crs_gather(GA_BASIS, n), rq::rand(ri.VR()), sm.BA());          // B_a
  l.push(rq::crs(0, n), rq::rand(ri.IR()), SL_BC);                          // B_c = msm(G | Hvec, r_c)
  l.push(rq::crs_col(cc.G_t()), rq::rand(ri.RT()), SL_CMT1, SL_CMT1);       // cm_T.T_1 = r_t G_t (kept: A' adds it)
  l.push(rq::crs_col(cc.G_u()), rq::rand(ri.RU()), SL_CMU1, SL_CMU1);       // cm_U.T_1
  l.push(rq::crs_col(cc.G_t()), rq::rand(ri.RA()), sm.CMA1());              // cm_A.T_1
  l.push(rq::crs_col(cc.G_u()), rq::rand(ri.RB()), sm.CMB1());              // cm_B.T_1
  const int rs[4] = {ri.RT(), ri.RU(), ri.RA(), ri.RB()};                       // r * H halves of the four T_2 commitments, kept as affine
  for (int q = 0; q < 4; q++) l.push(rq::crs_col(cc.H()), rq::rand(rs[q]), -1, sm.TMP(q));   // points for the side stream
  return l;
}
// phase 1t: B_t = msm(T_b, r), B_u = msm(U_b, r) (same_multiscalar_argument.rs:81-82) over the per-proof tables
inline ReqList prove_phase1t(int n, int L) {
  const SlotMap sm(L);
  const PtabRow row(n);
  ReqList l;
  l.push(rq::ptab(row.T(), n), rq::rand(RandIdx(n).VR()), sm.BT());
  l.push(rq::ptab(row.U(), n), rq::rand(RandIdx(n).VR()), sm.BU());
  return l;
}
// phase 2: B = A + alpha M + beta sum(G) (same_permutation_argument.rs:75-76) as two points and an addend or — commitment_form — as
// the commitment the reference computes, msm(G | Hvec, V_FACT); A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.rs:134), a sum of three
// points of phase 1; C = msm(G | Hvec, c) (grand_product_argument.rs:76)
inline ReqList prove_phase2(int n, int L, bool commitment_form) {
  const SlotMap sm(L);
  ReqList l;
  if (commitment_form) l.push(rq::crs(0, n), rq::vec(V_FACT), SL_B, SL_B);
  else {
    ReqDesc& b = l.push(rq::crs(CtabCols(n).G_sum(), 1), rq::sc(SC_BETA_SP), SL_B, SL_B);   // scalars [beta | alpha]
    b.seg1 = rq::ptab(PtabRow(n).M(), 1);
    rq::add3(b, SL_A);
  }
  rq::add3(l.push(ReqSeg{}, ReqScal{}, sm.APRIME()), SL_A, SL_CMT1, SL_CMU1);
  l.push(rq::crs(0, n), rq::vec(V_C), SL_C);
  return l;
}
// phase 3: D = B - beta^-1 sum(G) + alpha sum(H) (grand_product_argument.rs:132; G_sum, H_sum: adjacent columns),
// B_d = msm(G', r_d) = msm(G, r_d o u)
inline ReqList prove_phase3(int n, int L) {
  ReqList l;
  rq::add3(l.push(rq::crs(CtabCols(n).G_sum(), 2), rq::sc(SC_NEG_BETA_G_INV), SlotMap(L).D()), SL_B);
  l.push(rq::crs(0, n), rq::vec(V_ZZU), SL_BD);
  return l;
}
// IPA round j as MSMs over the original bases (inner_product_argument.rs:150-163); a proof's scalar row, as k_ipa_round_scalars leaves
// it: [L_C (hn), beta <c_L, d_R> | L_D (hn) | R_C (hn), beta <c_R, d_L> | R_D (hn)].  The H term of L_C / R_C is a second segment or —
// fused — one more column at the end of the gather list (its scalar follows the hn cross-term scalars either way)
inline ReqList prove_ipa_round(int n, int L, int j, bool fused) {
  const SlotMap sm(L);
  const int hn = n / 2, half = n >> (j + 1);
  ReqList l;
  l.round_stride = 4 * hn + 2;
  const int out[4] = {sm.LC(j), sm.LD(j), sm.RC(j), sm.RD(j)}, at[4] = {0, hn + 1, 2 * hn + 1, 3 * hn + 2};
  for (int q = 0; q < 4; q++) {
    const bool hi = q == 0 || q == 3, with_h = q == 0 || q == 2;
    if (with_h && fused) l.push(rq::crs_gather(hi ? GA_HI_H : GA_LO_H, hn + 1, half), rq::round(at[q]), out[q]);
    else l.push(rq::crs_gather(hi ? GA_HI : GA_LO, hn, half), rq::round(at[q]), out[q]);
    if (with_h && !fused) l.r[l.n - 1].seg1 = rq::crs_col(CtabCols(n).H());
  }
  return l;
}
// SameMSM round j (same_multiscalar_argument.rs:104-112): L_A, L_T, L_U = <x_L, {G_b, T_b, U_b}_R>, R_* = <x_R, {..}_L>; a proof's
// scalar row: [L_* scalars (hn) | R_* scalars (hn)]
inline ReqList prove_smsm_round(int n, int L, int j) {
  const SlotMap sm(L);
  const PtabRow row(n);
  const int hn = n / 2, half = n >> (j + 1);
  ReqList l;
  l.round_stride = 2 * hn;
  int out[6];
  sm.same_msm_round(j, out);
  for (int q = 0; q < 6; q++) {
    const bool left = q < 3;
    const ReqSeg s = q % 3 == 0 ? rq::crs_gather(left ? GA_BASIS_HI : GA_BASIS_LO, hn, half) : rq::ptab(q % 3 == 1 ? row.T() : row.U(), hn, left ? GA_HI : GA_LO, half);
    l.push(s, rq::round(left ? 0 : hn), out[q]);
  }
  return l;
}
// the six proof points the side stream computes outside the table-backed requests: R = a x vec_R, S = a x vec_S (curdleproofs.rs:112-113)
// and the four T_2 = s * {R, S} + r * H (curdleproofs.rs:115-116, same_scalar_argument.rs:60-61), on top of TMP(0..3) of phase 1
// (with R and S from the tables, below: the same six slots from k R and k S — prove_rs_tables, prove_rs_sums)
inline void side_stream_slots(int L, int q[6]) {
  const SlotMap sm(L);
  const int s[6] = {SL_R, SL_S, SL_CMT2, SL_CMU2, sm.CMA2(), sm.CMB2()};
  for (int i = 0; i < 6; i++) q[i] = s[i];
}

// R and S from the per-proof tables (option rs_from_tables, the device-resident prover): the witness says T_j = k R_sigma(j) and
// U_j = k S_sigma(j) (util.rs:94-95), and V_APERM is a_sigma(j), the same permutation applied to vec_a (curdleproofs.rs:93).  Hence
//     Rk = msm(T, a_sigma) = sum_j a_sigma(j) k R_sigma(j) = k msm(vec_R, a) = k R   and likewise   Sk = msm(U, a_sigma) = k S,
// over bases whose shifted tables the SameMSM rounds need anyway — in place of the one-off bucket MSMs R = msm(vec_R, a),
// S = msm(vec_S, a) (curdleproofs.rs:112-113).  The first ell entries of the rows only: the last four are the blinder slots
// (0, 0, H, 0 / 0, 0, 0, H), which V_APERM pairs with vec_a_blinders.  T and U in their given order — the permutation is in the
// scalars.  The two points stay in scratch slots no other request writes; no proof bytes come from them directly.
inline int rs_tables_slot(int L, int which) { return SlotMap(L).TMP(which ? 6 : 4); }   // Rk | Sk (TMP(5), TMP(7): the plans' write-only slots)
inline ReqList prove_rs_tables(int n, int L) {
  const PtabRow row(n);
  const int ell = n - (int)N_BLINDERS;
  ReqList l;
  l.push(rq::ptab(row.T(), ell), rq::vec(V_APERM), -1, rs_tables_slot(L, 0));
  l.push(rq::ptab(row.U(), ell), rq::vec(V_APERM), -1, rs_tables_slot(L, 1));
  return l;
}
// ... and the two commitments that need no scalar multiplication then: cm_T.T_2 = k R + r_t H = Rk + TMP(0), cm_U.T_2 = k S + r_u H =
// Sk + TMP(1) (curdleproofs.rs:115-116) — sums of kept points.  (R = k^-1 Rk, S = k^-1 Sk and cm_A.T_2 = r_k R + r_a H = (r_k k^-1) Rk +
// TMP(2), cm_B.T_2 likewise (same_scalar_argument.rs:60-61) are the side stream's four scalar multiplications.)
inline ReqList prove_rs_sums(int, int L) {
  const SlotMap sm(L);
  ReqList l;
  rq::add3(l.push(ReqSeg{}, ReqScal{}, SL_CMT2, SL_CMT2), rs_tables_slot(L, 0), sm.TMP(0));
  rq::add3(l.push(ReqSeg{}, ReqScal{}, SL_CMU2, SL_CMU2), rs_tables_slot(L, 1), sm.TMP(1));
  return l;
}

// ---- the verifier: D = B - beta^-1 sum(G) + alpha sum(H) (grand_product_argument.rs:223) and A' = A + cm_T.T_1 + cm_U.T_1
//      (curdleproofs.rs:258) over the decompressed proof points; both are hashed (bytes) and enter the accumulated check (points) ----
inline ReqList verify_requests(int n, int L) {
  const SlotMap sm(L);
  ReqList l;
  rq::add3(l.push(rq::crs(CtabCols(n).G_sum(), 2), rq::sc(VSC_NEG_BETA_G_INV), sm.D(), sm.D()), SL_B);
  rq::add3(l.push(ReqSeg{}, ReqScal{}, sm.APRIME(), sm.APRIME()), SL_A, SL_CMT1, SL_CMU1);
  return l;
}

}  // namespace cpx
