// Plan of cpx_whisk_find_trackers (whisk.cpp, find.hip) — host + device, no HIP call: which of the two paths a call takes, how the table
// path cuts the trackers into chunks that fit a memory budget, which (key, columns) a scan wave owns, the limits of a call, and the
// per-pair body of the scan (digits -> picks -> accumulate -> compare).  One definition for Engine::whisk_find_trackers, for k_find_scan and
// for tests/host_emul/find_plan_emul.cpp / find_scan_emul.cpp, which compile it for the CPU (tests/test_find_trackers_cpu.py).
//
// The relation tested for every (tracker i, key j) pair is  k_j * r_G_i == k_r_G_i  (whisk.rs:36-55).
//   ladder path  one k_smul element per pair (129 doublings, about 1.85 k field products), then k_find_compare
//   table path   per chunk of nc trackers the CRS table layout at fix_bits = 8 with one tracker per column,
//                tab[(w * 128 + (m - 1)) * nc + col] = m * 256^w * r_G_col  (w < 32, m = 1..128; kernels.h "fixed-base MSM"), built by
//                k_table_build (32 shifted copies) and k_fix_build<8>; a pair then costs at most 32 mixed additions (about 0.35 k products),
//                no doubling and no inversion.  A column costs about 85 k products to build (4096 entries at about 20 products each with the
//                normalisation, plus the shifted copies), so the table pays from about 57 keys on — operation counts, estimates; the
//                measured crossover is in profiles/find_trackers.md.
#pragma once
#include <cstddef>
#include <cstdint>
#include "g1_28.hpp"
#include "recode.hpp"

namespace cpx {

constexpr size_t kFindMaxTrackers = (size_t)1 << 23;   // 32-bit byte offsets into the uploaded trackers (96 B each), int grids
constexpr size_t kFindMaxKeys = (size_t)1 << 20;
constexpr uint64_t kFindMaxPairs = (uint64_t)1 << 32;  // n_trackers * n_keys
constexpr long kFindMinKeysMax = ((long)1 << 20) + 1;  // option find_table_min_keys: 1 = always the table, 2^20 + 1 = never
constexpr long kFindTableMbMax = 65536;                // option find_table_mb

constexpr int FIND_WINDOWS = 32;     // radix-256 windows of a whole scalar (FixWin<8>::W)
constexpr int FIND_MULT = 128;       // multiples per window: m = 1..128
constexpr int FIND_WAVE_COLS = 64;   // consecutive columns of a scan wave, one per lane

// bytes of the device types the chunking counts (find.hip asserts them against sizeof)
constexpr size_t kFindEntryBytes = 128;   // TFix
constexpr size_t kFindShiftBytes = 112;   // TAff
constexpr size_t kFindTmpBytes = 224;     // TblTmp

// false: beyond what one call takes (checked before any input is read)
inline bool find_fits(size_t n_trackers, size_t n_keys) {
  return n_trackers <= kFindMaxTrackers && n_keys <= kFindMaxKeys && (uint64_t)n_trackers * (uint64_t)n_keys <= kFindMaxPairs;
}

struct FindWave {
  size_t key, col0;   // the wave's key and its first column inside the chunk; lane l takes column col0 + l
};

struct FindPlan {
  size_t n_trackers = 0, n_keys = 0;
  bool table = false;       // false: the ladder path (k_smul + k_find_compare)
  size_t chunk_cols = 0;    // columns (trackers) per chunk of the table path; the last chunk may be short
  size_t n_chunks = 0;
  int fix_chunk = 1;        // k_fix_build normalises this many multiples per inversion round (a power of two dividing FIND_MULT)

  size_t chunk_first(size_t c) const { return c * chunk_cols; }
  size_t chunk_size(size_t c) const { return c + 1 < n_chunks ? chunk_cols : n_trackers - c * chunk_cols; }
  // device memory of a chunk of nc columns: the table, the 32 shifted copies it is built from, and ONE scratch buffer that serves
  // k_table_build (31 Jacobian copies per column) and then k_fix_build (fix_chunk entries per (window, column) thread, threads rounded
  // up to whole waves)
  static size_t table_entries(size_t nc) { return (size_t)FIND_WINDOWS * FIND_MULT * nc; }
  static size_t shift_entries(size_t nc) { return (size_t)FIND_WINDOWS * nc; }
  static size_t tmp_entries(size_t nc, int fix_chunk) {
    const size_t build = (size_t)(FIND_WINDOWS - 1) * nc, fix = ((size_t)FIND_WINDOWS * nc + 63) / 64 * 64 * (size_t)fix_chunk;
    return build > fix ? build : fix;
  }
  static size_t chunk_bytes(size_t nc, int fix_chunk) {
    return table_entries(nc) * kFindEntryBytes + shift_entries(nc) * kFindShiftBytes + tmp_entries(nc, fix_chunk) * kFindTmpBytes;
  }
  // Wave map of a chunk of nc columns: n_keys waves per block of 64 columns, the waves of a block next to each other — the waves in flight
  // at any time read the same 8 KB rows of a few column blocks (32 windows x 128 multiples x 8 KB = 32 MB per block).
  static size_t col_blocks(size_t nc) { return (nc + FIND_WAVE_COLS - 1) / FIND_WAVE_COLS; }
  size_t scan_waves(size_t nc) const { return n_keys * col_blocks(nc); }   // the scan's grid: single-wave work-groups
  FindWave wave(size_t g) const { return FindWave{g % n_keys, g / n_keys * FIND_WAVE_COLS}; }
};

// the largest normalisation chunk whose scratch stays below an eighth of the table it serves (32 threads x fix_chunk entries against
// 32 x 128 table entries per column): 8
inline int find_fix_chunk() {
  int c = FIND_MULT;
  while (c > 1 && (size_t)FIND_WINDOWS * c * kFindTmpBytes * 8 > (size_t)FIND_WINDOWS * FIND_MULT * kFindEntryBytes) c >>= 1;
  return c;
}

// min_keys = option find_table_min_keys, table_mb = option find_table_mb (MiB).  The caller has checked find_fits.
inline FindPlan find_plan(size_t n_trackers, size_t n_keys, long min_keys, long table_mb) {
  FindPlan pl;
  pl.n_trackers = n_trackers;
  pl.n_keys = n_keys;
  pl.table = n_trackers && n_keys && (long)n_keys >= min_keys;
  if (!pl.table) return pl;
  pl.fix_chunk = find_fix_chunk();
  const size_t budget = (size_t)(table_mb < 1 ? 1 : table_mb) << 20;
  size_t nc = budget / FindPlan::chunk_bytes(1, pl.fix_chunk);   // (an estimate from above: the scratch of one column is rounded up to a wave)
  while (nc > 1 && FindPlan::chunk_bytes(nc, pl.fix_chunk) > budget) nc--;
  while (FindPlan::chunk_bytes(nc + 1, pl.fix_chunk) <= budget) nc++;
  if (nc < 1) nc = 1;                                            // a budget below one column: one column per chunk all the same
  if (nc > FIND_WAVE_COLS) nc -= nc % FIND_WAVE_COLS;            // whole waves wherever a chunk holds more than one
  if (nc > n_trackers) nc = n_trackers;
  pl.chunk_cols = nc;
  pl.n_chunks = (n_trackers + nc - 1) / nc;
  return pl;
}

// ---- the per-pair body of the scan ----
// The 32 signed radix-256 digits of a canonical key (fix_window_digits<8, 32>: d_w in [-128, 127], no carry leaves the top window),
// packed four to a word: what a scan wave holds in scalar registers.
struct FindDigits {
  uint32_t w[8];
};
CPX_HD void find_recode(const uint32_t* k /*canonical, 8 words*/, FindDigits& o) {
  int16_t d[FIND_WINDOWS];
  fix_window_digits<8, FIND_WINDOWS>(k, 0, d, 1);
  CPX_UNROLL for (int j = 0; j < 8; j++) o.w[j] = 0;
  CPX_UNROLL for (int j = 0; j < FIND_WINDOWS; j++) o.w[j >> 2] |= ((uint32_t)d[j] & 0xffu) << (8 * (j & 3));
}
CPX_HD int find_digit(const FindDigits& dg, int w) {
  uint32_t word = dg.w[0];
  CPX_UNROLL for (int j = 1; j < 8; j++) word = (w >> 2) == j ? dg.w[j] : word;   // (selects, not a dynamically indexed register array)
  return (int)(int8_t)(word >> (8 * (w & 3)));
}
// which entry of a chunk's table digit d != 0 of window w reads for column col
CPX_HD size_t find_entry(int w, int d, size_t nc, size_t col) { return ((size_t)w * FIND_MULT + (size_t)((d < 0 ? -d : d) - 1)) * nc + col; }

// Does key (digits dg) open the tracker of column col?  acc = sum_w d_w * 256^w * r_G from the table, the entry of the next window in flight
// while the current one is added; then - k_r_G as an affine addend: the pair matches iff the sum is the identity and the tracker decoded
// (`ok`: k_decompress leaves the identity for a point that fails to decode, and such an identity must never match).  A dead lane
// (live = false) and a masked tracker run on the identity and read nothing.  No inversion anywhere.  INL: the products of the 32 additions
// inlined (the device loop) or called (the CPU twin).
template <bool INL> CPX_HD bool find_pair_matches(const FindDigits& dg, const TFix* tab, size_t nc, size_t col, bool live, const TAff& claimed, bool ok) {
  const bool walk = live && ok;
  auto fetch = [&](int w, int& d) {
    d = find_digit(dg, w);
    return d && walk ? tab[find_entry(w, d, nc, col)].a : TAff::identity();
  };
  TAcc acc = TAcc::identity();
  int dn;
  TAff pn = fetch(0, dn);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = 0; w < FIND_WINDOWS; w++) {
    const int d = dn;
    const TAff p = pn;
    if (w + 1 < FIND_WINDOWS) pn = fetch(w + 1, dn);
    if (d) acc = INL ? t_acc_add_mixed_inl(acc, t_cneg_lazy(p, d < 0)) : t_acc_add_mixed(acc, t_cneg(p, d < 0));   // (d is the same for the whole wave)
  }
  TAff c = TAff::identity();
  if (walk && !claimed.is_identity()) c = t_cneg(claimed, true);
  acc = t_acc_add_mixed(acc, c);
  return walk && acc.is_identity();
}

}  // namespace cpx
