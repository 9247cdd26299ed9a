// Schedule of the two-base joint ladder of the batched tracker-proof verifier (tracker.hip: k_tracker_relations) — host + device.
//
// One relation of a tracker proof (whisk.rs:219-223) is  a P1 + b P2 == C  with two 255-bit scalars.  Both scalars are split by the
// endomorphism and recoded as k_smul does (recode.hpp recode_smul_glv): four signed digit streams of 129 steps,
//     a P1 + b P2 = sum_{i=0}^{128} 2^i (e_i P1 + f_i N P1 + g_i P2 + h_i N P2),   e, f, g, h in {-1, 0, 1},   N P = -phi(P) (glv.hpp).
// A step is one doubling and at most one addition per base: the pair (e_i, f_i) names one entry of P1's table, (g_i, h_i) one of P2's.
// A table holds the eight non-zero combinations d P + d' N P in the order k_smul_quad uses:
//     0 +P   1 -P   2 +NP   3 -NP   4 +(P + NP)   5 -(P + NP)   6 +(P - NP)   7 -(P - NP)
// This header decides WHICH entry each base contributes at step i; the kernel (quad-cooperative additions, operands in LDS) and the
// CPU emulation of the tests (tests/host_emul/tracker_ladder_emul.cpp, one-lane additions) both walk it.
#pragma once
#include "recode.hpp"

namespace cpx {

constexpr int TRACKER_LADDER_TOP = 128;    // steps run from this bit down to 0
constexpr int TRACKER_TABLE_ENTRIES = 8;   // per base
// LDS / array slots of one relation: the accumulator, then the two tables
constexpr int TL_ACC = 0, TL_TAB = 1, TL_PER_REL = 1 + 2 * TRACKER_TABLE_ENTRIES;

// table entry of  d P + d' N P  for the digits (d, d') of step i of one recoded scalar; -1: both digits are zero
CPX_HD int glv_table_entry(const SmulNaf& rn, int i) {
  const int wd = i >> 5, bt = i & 31;
  const int dt = ((rn.nz[0][wd] >> bt) & 1u) ? (((rn.ng[0][wd] >> bt) & 1u) ? -1 : 1) : 0;
  const int dq = ((rn.nz[1][wd] >> bt) & 1u) ? (((rn.ng[1][wd] >> bt) & 1u) ? -1 : 1) : 0;
  if (dt && !dq) return dt > 0 ? 0 : 1;
  if (!dt && dq) return dq > 0 ? 2 : 3;
  if (dt && dq) return dt == dq ? (dt > 0 ? 4 : 5) : (dt > 0 ? 6 : 7);
  return -1;
}

struct TrackerStep {
  int e[2];   // entry of base 0 / base 1 added after the doubling of this step, -1 = none
};
CPX_HD TrackerStep tracker_ladder_step(const SmulNaf& a, const SmulNaf& b, int i) { return TrackerStep{{glv_table_entry(a, i), glv_table_entry(b, i)}}; }

}  // namespace cpx
