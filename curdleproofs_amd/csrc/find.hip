// gfx950 kernels of cpx_whisk_find_trackers: which of `n_keys` keys opens each of `n_trackers` trackers, k * r_G == k_r_G
// (whisk.rs:36-55 for every (tracker, key) pair; whisk.cpp drives them, find_plan.hpp holds the plan and the per-pair body).
//
//  k_find_scan      table path.  One lane per pair, one wave per (key, 64 consecutive tracker columns of the chunk).  The chunk's table is
//                   the CRS table layout at fix_bits = 8 with one tracker per column (k_table_build + k_fix_build<8>, unchanged), so a wave
//                   reads one contiguous 8 KB row per window.  The key's 32 digits are the same for the whole wave: recoded once, held in
//                   scalar registers, and a zero digit is skipped by the wave as a whole.  At most 32 mixed additions per pair, no doubling;
//                   - k_r_G is added at the end and the accumulator tested for the identity (as k_tracker_relations does): no inversion.
//                   Matching lanes take the smallest key index with a vector atomicMin.  Dead lanes and trackers that did not decode run on
//                   the identity and read nothing from the table.
//  k_find_compare   ladder path.  k_smul has written k_j * r_G_i for every pair (one task per key); one lane per tracker scans the keys in
//                   ascending order and compares the affine results with the decoded k_r_G.  The first match wins.
// Decoding and the table build are the existing kernels (k_decompress, k_table_build, k_fix_build).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "../../include/cpx.h"
#include "g1.hpp"
#include "g1_28.hpp"
#include "recode.hpp"
#include "find_plan.hpp"
#include "kernels.h"

namespace cpx {

static_assert(sizeof(TFix) == kFindEntryBytes && sizeof(TAff) == kFindShiftBytes && sizeof(TblTmp) == kFindTmpBytes, "find_plan.hpp counts these bytes");
static_assert(FIND_WINDOWS == FixWin<8>::W && FIND_MULT == (int)FixWin<8>::HALF, "the table of k_fix_build<8>");

// tab: the chunk's table of nc columns, column c = tracker col_first + c.  keys: n_keys Fr in Montgomery form (limbs that are not a reduced
// field element stand for limbs / 2^256 mod r, the way k_smul reads its scalars).  claimed: the decoded k_r_G of ALL trackers; status: the
// decoder's verdicts, r_G plane then k_r_G plane, n_trackers each.  owner: pre-filled with CPX_NO_OWNER.
__global__ __launch_bounds__(64) void k_find_scan(const TFix* __restrict__ tab, uint32_t nc, uint32_t col_first, const Fr* __restrict__ keys, uint32_t n_keys,
                                                  const Aff* __restrict__ claimed, const uint8_t* __restrict__ status, uint32_t n_trackers,
                                                  uint32_t* __restrict__ owner) {
  const uint32_t g = blockIdx.x, lane = threadIdx.x;
  const uint32_t key = g % n_keys, col = g / n_keys * FIND_WAVE_COLS + lane;   // FindPlan::wave
  const bool live = col < nc;
  const uint32_t trk = col_first + (live ? col : 0);
  FindDigits dg;
  find_recode(fe_from_mont(keys[key]).v, dg);
  CPX_UNROLL for (int j = 0; j < 8; j++) dg.w[j] = (uint32_t)__builtin_amdgcn_readfirstlane((int)dg.w[j]);   // (every lane computed the same words)
  const bool ok = live && status[trk] == 0 && status[(size_t)n_trackers + trk] == 0;
  const TAff c = ok ? t_from_std(claimed[trk]) : TAff::identity();
  if (find_pair_matches<true>(dg, tab, nc, col, live, c, ok)) atomicMin(&owner[trk], key);
}

// prod[j * n_trackers + i] = k_j * r_G_i (affine, standard form: k_smul's output); claimed / status as above
__global__ __launch_bounds__(64) void k_find_compare(const Aff* __restrict__ prod, const Aff* __restrict__ claimed, const uint8_t* __restrict__ status,
                                                     uint32_t n_trackers, uint32_t n_keys, uint32_t* __restrict__ owner) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_trackers) return;
  uint32_t own = CPX_NO_OWNER;
  if (status[i] == 0 && status[(size_t)n_trackers + i] == 0) {
    const Aff c = claimed[i];
    for (uint32_t j = 0; j < n_keys && own == CPX_NO_OWNER; j++) {
      const Aff p = prod[(size_t)j * n_trackers + i];
      bool same = true;
      CPX_UNROLL for (int l = 0; l < 12; l++) same = same && p.x.v[l] == c.x.v[l] && p.y.v[l] == c.y.v[l];
      if (same) own = j;
    }
  }
  owner[i] = own;
}

#define FIND_LAUNCH(kern, grid, block, lds, stream, ...)                                            \
  do {                                                                                                \
    hipEvent_t _a = nullptr, _b = nullptr;                                                            \
    take_launch_events(&_a, &_b);                                                                     \
    if (_a || _b) hipExtLaunchKernelGGL(kern, grid, block, lds, stream, _a, _b, 0, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                             \
  } while (0)

void launch_find_scan(const FindPlan& pl, const TFix* d_tab, size_t nc, size_t col_first, const Fr* d_keys, const Aff* d_claimed, const uint8_t* d_status,
                      uint32_t* d_owner, hipStream_t s) {
  const size_t waves = pl.scan_waves(nc);
  if (!waves) return;
  FIND_LAUNCH(k_find_scan, dim3((unsigned)waves), dim3(64), 0, s, d_tab, (uint32_t)nc, (uint32_t)col_first, d_keys, (uint32_t)pl.n_keys, d_claimed, d_status,
              (uint32_t)pl.n_trackers, d_owner);
}
void launch_find_compare(const Aff* d_prod, const Aff* d_claimed, const uint8_t* d_status, size_t n_trackers, size_t n_keys, uint32_t* d_owner, hipStream_t s) {
  if (!n_trackers) return;
  FIND_LAUNCH(k_find_compare, dim3((unsigned)((n_trackers + 63) / 64)), dim3(64), 0, s, d_prod, d_claimed, d_status, (uint32_t)n_trackers, (uint32_t)n_keys, d_owner);
}

}  // namespace cpx
