// Index layouts shared by the host-driven protocol (engine.cpp), the device-resident one (engine_device.cpp, protocol.hip) and
// the host-only test build: the per-proof point registry, the wire format of a proof, the prover's random draws, the row of a
// proof's point table, the columns of the CRS tables and the verifier's random factors.  Plain index arithmetic, no HIP.
// prove_reqs.hpp states the protocol's MSM requests in these names.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mont32.hpp"

namespace cpx {

static constexpr size_t N_BLINDERS = 4;   // lib.rs:35: n = ell + N_BLINDERS bases, the last four carry the blinders

// ---- per-proof point registry ("slots") that follows the 4*ell instance points in d_pp_ ----
// CRS singles, M, then every proof point in serialisation order (curdleproofs.rs:300-310), then scratch.
enum { SL_H = 0, SL_GT, SL_GU, SL_GSUM, SL_HSUM, SL_M, SL_A, SL_CMT1, SL_CMT2, SL_CMU1, SL_CMU2, SL_R, SL_S, SL_B, SL_C, SL_BC, SL_BD, SL_IPA0 };
// The "misc" points of the verifier's accumulated check are the slots 0 .. SL_A + n_points(): slot s is misc point s.
static_assert(SL_A == SL_M + 1, "the proof points must follow the CRS singles and M without a gap");
static constexpr uint8_t kCompIdentity = 0xc0;   // first byte of the compressed identity (the other 47 are zero)
struct SlotMap {
  int L;
  CPX_HD explicit SlotMap(size_t l) : L((int)l) {}
  CPX_HD int LC(int j) const { return SL_IPA0 + j; }
  CPX_HD int RC(int j) const { return SL_IPA0 + L + j; }
  CPX_HD int LD(int j) const { return SL_IPA0 + 2 * L + j; }
  CPX_HD int RD(int j) const { return SL_IPA0 + 3 * L + j; }
  CPX_HD int CMA1() const { return SL_IPA0 + 4 * L; }
  CPX_HD int CMA2() const { return CMA1() + 1; }
  CPX_HD int CMB1() const { return CMA1() + 2; }
  CPX_HD int CMB2() const { return CMA1() + 3; }
  CPX_HD int BA() const { return CMA1() + 4; }
  CPX_HD int BT() const { return CMA1() + 5; }
  CPX_HD int BU() const { return CMA1() + 6; }
  CPX_HD int LA(int j) const { return CMA1() + 7 + j; }
  CPX_HD int LT(int j) const { return CMA1() + 7 + L + j; }
  CPX_HD int LU(int j) const { return CMA1() + 7 + 2 * L + j; }
  CPX_HD int RA(int j) const { return CMA1() + 7 + 3 * L + j; }
  CPX_HD int RT(int j) const { return CMA1() + 7 + 4 * L + j; }
  CPX_HD int RU(int j) const { return CMA1() + 7 + 5 * L + j; }
  CPX_HD int D() const { return CMA1() + 7 + 6 * L; }
  CPX_HD int APRIME() const { return D() + 1; }
  CPX_HD int TMP(int i) const { return D() + 2 + i; }   // 8 scratch results
  CPX_HD int count() const { return D() + 2 + 8; }
  // the points the transcripts absorb together, in the order they are hashed (the proof-byte known answers pin it):
  // same_scalar_argument.rs:112-118, and one round of inner_product_argument.rs:164-170 / same_multiscalar_argument.rs:114-122
  CPX_HD void sameexp_points(int q[10]) const {
    const int pts[10] = {SL_R, SL_S, SL_CMT1, SL_CMT2, SL_CMU1, SL_CMU2, CMA1(), CMA2(), CMB1(), CMB2()};
    for (int i = 0; i < 10; i++) q[i] = pts[i];
  }
  CPX_HD void ipa_round(int j, int q[4]) const {
    const int pts[4] = {LC(j), LD(j), RC(j), RD(j)};
    for (int i = 0; i < 4; i++) q[i] = pts[i];
  }
  CPX_HD void same_msm_round(int j, int q[6]) const {
    const int pts[6] = {LA(j), LT(j), LU(j), RA(j), RT(j), RU(j)};
    for (int i = 0; i < 6; i++) q[i] = pts[i];
  }
};

// ---- wire format of a proof (CurdleproofsProof::serialize, curdleproofs.rs:300-310): the proof points in slot order from SL_A,
//      the seven scalars interleaved — r_p after C, c and d after the IPA's R_D, the z's after cm_B.T_2, x at the end ----
struct ProofLayout {
  enum Scalar { r_p = 0, c, d, z_k, z_t, z_u, x, N_SCALARS };
  int L;
  CPX_HD explicit ProofLayout(size_t l) : L((int)l) {}
  CPX_HD int n_points() const { return SlotMap(L).D() - SL_A; }   // SL_A .. RU(L-1), contiguous: 18 + 10 L
  // proof points serialised before scalar i
  CPX_HD int points_before(int i) const {
    const SlotMap sm(L);
    return (i == r_p ? SL_C + 1 : i <= d ? sm.CMA1() : i <= z_u ? sm.BA() : sm.D()) - SL_A;
  }
  // byte offset of proof point q (slot SL_A + q)
  CPX_HD size_t point_offset(int q) const {
    return 48 * (size_t)q + (q >= points_before(r_p) ? 32 : 0) + (q >= points_before(c) ? 64 : 0) + (q >= points_before(z_k) ? 96 : 0);
  }
  CPX_HD size_t scalar_offset(int i) const { return 48 * (size_t)points_before(i) + 32 * (size_t)i; }
  CPX_HD size_t size() const { return 48 * (size_t)n_points() + 32 * N_SCALARS; }
};

// ---- the prover's 3n+9 random draws (SURVEY 8b RNG contract), as indices into a proof's `rand` row ----
struct RandIdx {
  int n;
  CPX_HD explicit RandIdx(int n_) : n(n_) {}
  CPX_HD int AB() const { return 0; }              // vec_a_blinders[2]     curdleproofs.rs:86
  CPX_HD int CB() const { return 2; }              // vec_c_blinders[4]     grand_product_argument.rs:75
  CPX_HD int IR() const { return 6; }              // IPA r[n]              inner_product_argument.rs:46
  CPX_HD int IZ() const { return 6 + n; }          // IPA z[n-2]            inner_product_argument.rs:47
  CPX_HD int RT() const { return 2 * n + 4; }      // r_t, r_u              curdleproofs.rs:110-111
  CPX_HD int RU() const { return 2 * n + 5; }
  CPX_HD int RA() const { return 2 * n + 6; }      // r_a, r_b, r_k         same_scalar_argument.rs:56-58
  CPX_HD int RB() const { return 2 * n + 7; }
  CPX_HD int RK() const { return 2 * n + 8; }
  CPX_HD int VR() const { return 2 * n + 9; }      // SameMSM vec_r[n]      same_multiscalar_argument.rs:78
  CPX_HD int count() const { return 3 * n + 9; }
};

// ---- row of a proof's point table (ptab): M, then T_b and U_b, the instance vectors T, U with their four blinder points ----
struct PtabRow {
  int n;
  CPX_HD explicit PtabRow(size_t n_) : n((int)n_) {}
  CPX_HD int M() const { return 0; }
  CPX_HD int T() const { return 1; }
  CPX_HD int U() const { return 1 + n; }
  CPX_HD int count() const { return 1 + 2 * n; }   // (R and S are used once: no table)
};

// ---- columns of the CRS tables (ctab, fixtab): G | Hvec, then the single points.  Columns 0 .. G_u coincide with the
//      CurdleproofsCrs::from_points input (crs.rs:37-58); G_sum, H_sum (crs.rs:46-47) are computed ----
struct CtabCols {
  int n;
  CPX_HD explicit CtabCols(size_t n_) : n((int)n_) {}
  CPX_HD int H() const { return n; }
  CPX_HD int G_t() const { return n + 1; }
  CPX_HD int G_u() const { return n + 2; }
  CPX_HD int G_sum() const { return n + 3; }
  CPX_HD int H_sum() const { return n + 4; }
  CPX_HD int count() const { return n + 5; }
  // the SameMSM basis G | Hvec[0..2) | G_t | G_u (curdleproofs.rs:136-139) as n column indices
  CPX_HD void same_msm_basis(uint32_t* cols) const {
    for (int i = 0; i < n - 2; i++) cols[i] = (uint32_t)i;
    cols[n - 2] = (uint32_t)G_t();
    cols[n - 1] = (uint32_t)G_u();
  }
};

// ---- the verifier's random factors (msm_accumulator.rs:44), as indices into a proof's `rand` row.  a1 .. a8 weight the accumulated
//      checks: SamePermutation, the IPA over C and over D, SameMultiscalar over A', cm_T.T_2 and cm_U.T_2, R and S against vec_a
//      (curdleproofs.rs:293-294).  The fused verifier takes four more, w1 .. w4, for the SameScalar equalities of cm_A.T_1, cm_A.T_2,
//      cm_B.T_1 and cm_B.T_2 (same_scalar_argument.rs:127-137) ----
enum { VF_SAMEPERM = 0, VF_IPA_C, VF_IPA_D, VF_SMSM_A, VF_SMSM_T, VF_SMSM_U, VF_R, VF_S, VF_COUNT,   // 8: per-proof verdicts
       VF_SS_A1 = VF_COUNT, VF_SS_A2, VF_SS_B1, VF_SS_B2, VF_FUSED_COUNT };                       // 12: fused batch

}  // namespace cpx
