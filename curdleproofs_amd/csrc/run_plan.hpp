// Index bookkeeping of a run of Whisk shuffles against the resident candidate list (cpx_whisk_verify_shuffle_run; whisk.cpp, run.hip) —
// plain integers, no HIP: one definition for the host that builds the lists, the kernels that walk them, and the g++ twin
// tests/host_emul/run_plan_emul.cpp.
//
// Item b of a run reads the candidates at indices[b][0..ell) and writes its post trackers back to the same indices, slot by slot in rising
// j.  The post trackers of all items are decoded once into the planes T | U of the call ([count][ell] each, shuffle_plan.hpp); position
// p = b * ell + j names post tracker j of item b in them.
//
//   source list   for every (b, j) where the pre tracker comes from: a candidate index of the list as loaded, or, flagged RUN_SRC_POST,
//                 the position of the last write to that index by an EARLIER item (an item reads before it writes; every earlier item counts,
//                 whatever its verdict: the as-if list of include/cpx.h).
//   commit list   for the first n_applied items, one (candidate index, position) pair per touched index: the position that ends up there.
//                 The destinations are pairwise different, so the device write-back has no two lanes on one candidate.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mont32.hpp"

namespace cpx {

// count * ell < 2^28 (ShufflePlan::fits) and n <= 2^24: bit 31 is free in both kinds of entry
constexpr uint32_t RUN_SRC_POST = 0x80000000u;
constexpr uint32_t RUN_NO_WRITER = 0xffffffffu;
constexpr size_t RUN_MAX_CANDIDATES = (size_t)1 << 24;

CPX_HD bool run_src_is_post(uint32_t s) { return (s & RUN_SRC_POST) != 0; }
CPX_HD uint32_t run_src_index(uint32_t s) { return s & ~RUN_SRC_POST; }   // a candidate index, or a position in the post planes

struct RunPlan {
  uint32_t count, ell, n;   // items, trackers per item, candidates in the list
  CPX_HD RunPlan(size_t count_, size_t ell_, size_t n_) : count((uint32_t)count_), ell((uint32_t)ell_), n((uint32_t)n_) {}
  CPX_HD size_t reads() const { return (size_t)count * ell; }
  // every index names a candidate
  CPX_HD bool indices_valid(const uint32_t* indices) const {
    for (size_t g = 0; g < reads(); g++)
      if (indices[g] >= n) return false;
    return true;
  }
  // src[b * ell + j] for all items; last_writer: n entries of scratch (left holding the last position written to every index, RUN_NO_WRITER
  // where none was).  The indices must be valid.
  CPX_HD void resolve(const uint32_t* indices, uint32_t* src, uint32_t* last_writer) const {
    for (uint32_t i = 0; i < n; i++) last_writer[i] = RUN_NO_WRITER;
    for (uint32_t b = 0; b < count; b++) {
      const size_t row = (size_t)b * ell;
      for (uint32_t j = 0; j < ell; j++) {   // the reads of an item come before its own writes
        const uint32_t w = last_writer[indices[row + j]];
        src[row + j] = w == RUN_NO_WRITER ? indices[row + j] : (RUN_SRC_POST | w);
      }
      for (uint32_t j = 0; j < ell; j++) last_writer[indices[row + j]] = (uint32_t)(row + j);   // rising j: the highest slot wins
    }
  }
  // The write-back of items 0 .. n_applied-1: dst[t] = a candidate index, pos[t] = the post position that ends up there, t < the returned
  // length (at most n_applied * ell; every dst once).  last_writer: n entries of scratch.
  CPX_HD size_t commit_list(const uint32_t* indices, uint32_t n_applied, uint32_t* dst, uint32_t* pos, uint32_t* last_writer) const {
    if (n_applied > count) n_applied = count;
    const size_t writes = (size_t)n_applied * ell;
    for (uint32_t i = 0; i < n; i++) last_writer[i] = RUN_NO_WRITER;
    for (size_t g = 0; g < writes; g++) last_writer[indices[g]] = (uint32_t)g;
    size_t len = 0;
    for (size_t g = 0; g < writes; g++)
      if (last_writer[indices[g]] == (uint32_t)g) {   // the one write that is not overwritten
        dst[len] = indices[g];
        pos[len] = (uint32_t)g;
        len++;
      }
    return len;
  }
};

// ---- lane layout of the two copy kernels (run.hip): a decoded point is RUN_POINT_CHUNKS 16-byte pieces, one lane each, the lanes of one
// point side by side, so a wave's loads and stores of a point are one contiguous 96-byte stretch ----
constexpr uint32_t RUN_POINT_CHUNKS = 6;
constexpr uint32_t RUN_BLOCK_POINTS = 32;                                  // points per work-group
constexpr uint32_t RUN_BLOCK_THREADS = RUN_BLOCK_POINTS * RUN_POINT_CHUNKS;   // 192 = 3 waves
CPX_HD size_t run_copy_blocks(size_t points) { return (points + RUN_BLOCK_POINTS - 1) / RUN_BLOCK_POINTS; }
CPX_HD size_t run_lane_point(size_t block, uint32_t thread) { return block * RUN_BLOCK_POINTS + thread / RUN_POINT_CHUNKS; }
CPX_HD uint32_t run_lane_chunk(uint32_t thread) { return thread % RUN_POINT_CHUNKS; }

}  // namespace cpx
