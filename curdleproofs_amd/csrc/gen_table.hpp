// Fixed-base table of the G1 generator: layout, window width and the recoding of a scalar into table picks — host + device.
//
// Every multiple of the generator G the Whisk input side needs (r G, k G, k (r G) = (k r) G) has the same base, so the doublings of a
// double-and-add chain can be done once, in a table.  A scalar is split by the endomorphism as everywhere else (glv.hpp, the ONE split):
//     k = sk (st |t| + q N)  (mod r),   N = z^2,   |t|, q < 2^127,   N P = -phi(P) = (beta x, -y),
// and both halves are written in the signed radix-256 digits of glv_biased_bytes:  v = sum_w d_w 256^w,  d_w in [-128, 127],  16 digits.
// That recoding needs NO carry window: |t| <= N / 2 and q <= r / (2 N) + 1 have a top byte of at most 0x56, so the bias of the top digit
// never overflows and the top digit lies in [0, GEN_TOP_DIGIT_MAX].  The table therefore holds
//     T[w][j - 1] = j 256^w G,   j = 1 .. 128 for the windows w < 15,   j = 1 .. GEN_TOP_DIGIT_MAX for w = 15:
// GEN_TABLE_ENTRIES = 15 * 128 + 86 = 2006 affine points in the table form (TAff, 112 bytes): 224 672 bytes — every one of them can be
// asked for, nothing else can.  The endomorphism half is not stored: its entries are (beta x, -y) of the same points, one field product
// per pick.  k G is then at most 32 mixed additions (one per window and half) and no doubling.
// This header decides WHICH entry, with which sign, each (half, window) contributes; the kernels (genmul.hip) and the CPU twin of the tests
// (tests/host_emul/gen_table_emul.cpp) both walk it.
#pragma once
#include "glv.hpp"

namespace cpx {

constexpr int GEN_WINDOW_BITS = 8;
constexpr int GEN_WINDOWS = 16;            // per half
constexpr int GEN_DIGIT_MAX = 128;         // largest digit magnitude of the windows below the top one (digit -128)
constexpr int GEN_TOP_DIGIT_MAX = 0x56;    // largest digit of window 15 (never negative): the top byte of floor(N / 2)
constexpr int GEN_TABLE_ENTRIES = (GEN_WINDOWS - 1) * GEN_DIGIT_MAX + GEN_TOP_DIGIT_MAX;
constexpr int GEN_MAX_ADDS = 2 * GEN_WINDOWS;   // mixed additions per scalar

// digit magnitudes 1 .. gen_window_entries(w) of window w have an entry
CPX_HD constexpr int gen_window_entries(int w) { return w == GEN_WINDOWS - 1 ? GEN_TOP_DIGIT_MAX : GEN_DIGIT_MAX; }
CPX_HD constexpr int gen_table_index(int w, int mag) { return w * GEN_DIGIT_MAX + mag - 1; }   // mag >= 1
// entry e = (w, j): the multiple j 256^w
CPX_HD constexpr int gen_entry_window(int e) { return e / GEN_DIGIT_MAX; }
CPX_HD constexpr int gen_entry_multiple(int e) { return e % GEN_DIGIT_MAX + 1; }

// a recoded scalar: the biased digit bytes of |t| (half 0) and q (half 1), and the sign of each half's sum
struct GenDigits {
  uint32_t bytes[2][4];
  uint32_t neg[2];
};
// k: canonical scalar (8 words, < r)
CPX_HD void gen_recode(const uint32_t* k, GenDigits& o) {
  uint32_t t[4], q[4], nk, nt;
  glv_split(k, t, q, nk, nt);
  glv_biased_bytes(t, o.bytes[0]);
  glv_biased_bytes(q, o.bytes[1]);
  o.neg[0] = nk ^ nt;
  o.neg[1] = nk;
}

// What window w of half h contributes:  (neg ? -1 : 1) * E,  E = T[index] for half 0 and N T[index] = (beta x, -y) of it for half 1;
// index < 0: nothing (a zero digit).
struct GenPick {
  int index;
  bool neg;
};
CPX_HD GenPick gen_pick(const GenDigits& d, int half, int w) {
  const int digit = (int)((d.bytes[half][w >> 2] >> (8 * (w & 3))) & 0xffu) - 128;
  const int mag = digit < 0 ? -digit : digit;
  return GenPick{mag ? gen_table_index(w, mag) : -1, ((digit < 0) != (d.neg[half] != 0))};
}

}  // namespace cpx
