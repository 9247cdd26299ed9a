// gfx950 kernels of the Whisk shuffle run against the resident candidate list (cpx_whisk_verify_shuffle_run; whisk.cpp drives them,
// run_plan.hpp holds the source / commit lists and the lane layout they share with the host).
//
//  k_run_gather   fills the planes R | S of the call and their status bytes: pre tracker g = b * ell + j is a candidate of the resident
//                 list (planes cand_R | cand_S of n points) or, flagged, a post tracker of an earlier item of the same call (planes T | U,
//                 just decoded).  It runs after the decoder and before k_shuffle_status, so the status fold and the placeholder
//                 substitution see a run like a call with explicit pre trackers.
//  k_run_commit   the write-back: the winning post trackers of the applied items, points and status, into the candidate planes.  The
//                 destinations of the commit list are pairwise different (RunPlan::commit_list).
// Both are copies: a point is six 16-byte pieces, one lane each, the six lanes of a point side by side (run_plan.hpp).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "g1.hpp"
#include "kernels.h"
#include "run_plan.hpp"

namespace cpx {

static_assert(sizeof(Aff) == RUN_POINT_CHUNKS * sizeof(uint4), "a decoded point is six 16-byte pieces");

// src [pp]: the source list.  cand / cand_status: cand_R | cand_S, n points each.  pts / status: R | S | T | U of pp points each (T, U read; R, S written).
__global__ __launch_bounds__(RUN_BLOCK_THREADS) void k_run_gather(uint32_t pp, uint32_t n, const uint32_t* __restrict__ src, const Aff* __restrict__ cand,
                                                                  const uint8_t* __restrict__ cand_status, Aff* pts, uint8_t* status) {
  const size_t g = run_lane_point(blockIdx.x, threadIdx.x);
  if (g >= pp) return;
  const uint32_t c = run_lane_chunk(threadIdx.x), s = src[g], at = run_src_index(s);
  const bool post = run_src_is_post(s);
  if (at >= (post ? pp : n)) return;   // (the host refuses such a list before anything is launched: the kernel stays inside its buffers)
  const Aff* from_r = post ? pts + 2 * (size_t)pp + at : cand + at;
  const Aff* from_s = post ? pts + 3 * (size_t)pp + at : cand + (size_t)n + at;
  const uint4 r = reinterpret_cast<const uint4*>(from_r)[c], u = reinterpret_cast<const uint4*>(from_s)[c];
  reinterpret_cast<uint4*>(pts + g)[c] = r;
  reinterpret_cast<uint4*>(pts + (size_t)pp + g)[c] = u;
  if (c == 0) {
    const uint8_t* st = post ? status + 2 * (size_t)pp : cand_status;
    const size_t plane = post ? pp : n;
    status[g] = st[at];
    status[(size_t)pp + g] = st[plane + at];
  }
}

// len pairs (dst[t], pos[t]): candidate dst[t] becomes post tracker pos[t] of the call (planes T | U of pts)
__global__ __launch_bounds__(RUN_BLOCK_THREADS) void k_run_commit(uint32_t len, uint32_t pp, uint32_t n, const uint32_t* __restrict__ dst, const uint32_t* __restrict__ pos,
                                                                  const Aff* __restrict__ pts, const uint8_t* __restrict__ status, Aff* __restrict__ cand,
                                                                  uint8_t* __restrict__ cand_status) {
  const size_t t = run_lane_point(blockIdx.x, threadIdx.x);
  if (t >= len) return;
  const uint32_t c = run_lane_chunk(threadIdx.x), d = dst[t], p = pos[t];
  if (d >= n || p >= pp) return;   // (as above)
  reinterpret_cast<uint4*>(cand + d)[c] = reinterpret_cast<const uint4*>(pts + 2 * (size_t)pp + p)[c];
  reinterpret_cast<uint4*>(cand + (size_t)n + d)[c] = reinterpret_cast<const uint4*>(pts + 3 * (size_t)pp + p)[c];
  if (c == 0) {
    cand_status[d] = status[2 * (size_t)pp + p];
    cand_status[(size_t)n + d] = status[3 * (size_t)pp + p];
  }
}

#define RUN_LAUNCH(kern, grid, block, stream, ...)                                                \
  do {                                                                                              \
    hipEvent_t _a = nullptr, _b = nullptr;                                                          \
    take_launch_events(&_a, &_b);                                                                   \
    if (_a || _b) hipExtLaunchKernelGGL(kern, grid, block, 0, stream, _a, _b, 0, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);                             \
  } while (0)

void launch_run_gather(uint32_t pp, uint32_t n, const uint32_t* d_src, const Aff* d_cand, const uint8_t* d_cand_status, Aff* d_pts, uint8_t* d_status, hipStream_t s) {
  if (!pp) return;
  RUN_LAUNCH(k_run_gather, dim3((unsigned)run_copy_blocks(pp)), dim3(RUN_BLOCK_THREADS), s, pp, n, d_src, d_cand, d_cand_status, d_pts, d_status);
}
void launch_run_commit(uint32_t len, uint32_t pp, uint32_t n, const uint32_t* d_dst, const uint32_t* d_pos, const Aff* d_pts, const uint8_t* d_status, Aff* d_cand,
                       uint8_t* d_cand_status, hipStream_t s) {
  if (!len) return;
  RUN_LAUNCH(k_run_commit, dim3((unsigned)run_copy_blocks(len)), dim3(RUN_BLOCK_THREADS), s, len, pp, n, d_dst, d_pos, d_pts, d_status, d_cand, d_cand_status);
}

}  // namespace cpx
