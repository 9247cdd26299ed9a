// TEST-ONLY: the host side of the shifted-table recoding compiled for the CPU — the endomorphism split (glv.hpp), the signed radix-256
// digits of a half (glv_biased_bytes) and the window -> (copy, weight class) map of the one- and two-segment tables (recode.hpp
// tbl_window), exactly as k_msm_tblw and k_late_uniform use them, and the partial-slot layout of the bucket-list waves (tbw_parts,
// tbw_part_slot), as the waves and the planner of a table phase use it.
#include <cstdint>
#include "../../curdleproofs_amd/csrc/recode.hpp"

using namespace cpx;

// digits[w], copy[w], cls[w] for the 16 windows of the half v (4 words; at most 0x7f7f...7f, the domain of glv_biased_bytes), as
// windows first .. first + 15 (first = 0: the |t| half, 16: the q half) of a table with `real` shifted copies per half
extern "C" void emul_half_windows(const uint32_t* v, uint32_t real, uint32_t first, int32_t* digits, uint32_t* copy, uint32_t* cls) {
  uint32_t bytes[4];
  glv_biased_bytes(v, bytes);
  for (uint32_t w = 0; w < 16; w++) {
    digits[w] = (int32_t)((bytes[w >> 2] >> (8 * (w & 3))) & 255u) - 128;
    const TblWindow tw = tbl_window(first + w, real);
    copy[w] = tw.copy;
    cls[w] = tw.cls;
  }
}

// k (canonical, 8 words) -> |t|, q (4 words each), the signs of k and t, and the 32 windows of both halves
extern "C" void emul_scalar_windows(const uint32_t* k, uint32_t real, uint32_t* t_abs, uint32_t* q, uint32_t* neg, int32_t* digits, uint32_t* copy, uint32_t* cls) {
  glv_split(k, t_abs, q, neg[0], neg[1]);   // neg[0]: k was negated, neg[1]: t is negative
  emul_half_windows(t_abs, real, 0, digits, copy, cls);
  emul_half_windows(q, real, 16, digits + 16, copy + 16, cls + 16);
}

extern "C" uint32_t emul_tbw_parts(uint32_t wpw, uint32_t segs) { return tbw_parts(wpw, segs); }
extern "C" uint32_t emul_tbw_parts_hi(uint32_t wpw, uint32_t segs) { return tbw_parts_hi(wpw, segs); }
extern "C" uint32_t emul_tbw_part_slot(uint32_t wpw, uint32_t segs, uint32_t waves, uint32_t slices, uint32_t wv, uint32_t slice, uint32_t set) {
  return tbw_part_slot(wpw, segs, waves, slices, wv, slice, set);
}
