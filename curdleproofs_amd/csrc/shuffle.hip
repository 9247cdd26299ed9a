// gfx950 kernels of the batched Whisk shuffle calls (whisk.rs:106-179 and util.rs:83-106 for `count` independent shuffles per call;
// whisk.cpp drives them, shuffle_plan.hpp holds the index arithmetic they share with the host).
//
//  k_shuffle_status   one wave per item: folds the decoding statuses of the item's points into one flag, puts the placeholder
//                     instance (every point the generator) into the rows of an item that did not decode, and — prover form — turns the
//                     item's permutation and its four blinders into the n Montgomery scalars of  M = msm(vec_G, sigma) + msm(vec_H,
//                     blinders)  (util.rs:99-104); verifier form: the decoded M as the Jacobian point the engine loads.
//  k_shuffle_gather   one lane per (item, j):  T[i][j] = (k R)[i][perm[i][j]],  U likewise (util.rs:96-97), written dense for the
//                     engine's instance rows and interleaved (T_j, U_j) for the compression into post trackers (whisk.rs:279-293).
//  k_shuffle_commit   one lane per item: the affine M the fixed-base phase left in the item's slot, as the Jacobian point the engine loads.
// Decoding, the scalar multiplications k R / k S, the MSM behind M and the compression are the existing kernels (k_decompress,
// k_smul, k_msm_fix + k_reduce_sets + k_finalize_ranges, k_compress).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "g1.hpp"
#include "kernels.h"
#include "shuffle_plan.hpp"

namespace cpx {

// status: the decoder's verdicts, indexed like pts (nullptr: the points came in decoded — cpx_batch_shuffle); pts: the decoded planes.
template <bool VERIFIER>
__global__ __launch_bounds__(64) void k_shuffle_status(ShufflePlan pl, const uint8_t* __restrict__ status, Aff* __restrict__ pts, Aff gen,
                                                       const uint32_t* __restrict__ perm, const Fr* __restrict__ blinders, Fr* __restrict__ msc,
                                                       Jac* __restrict__ mjac, uint8_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x, lane = threadIdx.x;
  if (i >= pl.count) return;
  const bool is_bad = status && __any(pl.item_bad(status, i, lane, 64) ? 1 : 0);   // (uniform over the wave)
  if (lane == 0) bad[i] = is_bad ? 1 : 0;
  if (is_bad)
    for (uint32_t p = 0; p < pl.planes(); p++)
      for (uint32_t e = lane; e < pl.ell; e += 64) pts[pl.point_index(p, i, e)] = shuffle_row_point(true, pts[pl.point_index(p, i, e)], gen);
  if (VERIFIER) {
    if (lane == 0) mjac[i] = Jac::from_affine(shuffle_row_point(is_bad, pts[pl.m_index(i)], gen));
    return;
  }
  // sigma as field elements, then the blinders (already Montgomery limbs)
  const uint32_t n = pl.ell + 4;
  for (uint32_t e = lane; e < n; e += 64) {
    Fr s;
    if (e < pl.ell) {
      CPX_UNROLL for (int w = 0; w < 8; w++) s.v[w] = 0;
      s.v[0] = perm[(size_t)i * pl.ell + e];
      s = fe_to_mont(s);
    } else {
      s = blinders[(size_t)i * 4 + (e - pl.ell)];
    }
    msc[(size_t)i * n + e] = s;
  }
}

__global__ __launch_bounds__(256) void k_shuffle_gather(ShufflePlan pl, const uint32_t* __restrict__ perm, const Aff* __restrict__ kr, const Aff* __restrict__ ks,
                                                        Aff* __restrict__ vec_t, Aff* __restrict__ vec_u, Aff* __restrict__ zipped) {
  const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= pl.plane_points()) return;
  const uint32_t j = (uint32_t)(g % pl.ell);
  const size_t src = g - j + pl.gather_src(perm[g], j);
  const Aff t = kr[src], u = ks[src];
  vec_t[pl.dense_dst(g)] = t;
  vec_u[pl.dense_dst(g)] = u;
  zipped[pl.zip_dst(g, 0)] = t;
  zipped[pl.zip_dst(g, 1)] = u;
}

// pp: the engine's per-proof rows (stride pp_stride points); m_slot: where the row keeps its affine M
__global__ __launch_bounds__(256) void k_shuffle_commit(const Aff* __restrict__ pp, size_t pp_stride, uint32_t m_slot, uint32_t count, Jac* __restrict__ mjac) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  mjac[i] = Jac::from_affine(pp[(size_t)i * pp_stride + m_slot]);
}

#define SHF_LAUNCH(kern, grid, block, stream, ...)                                                \
  do {                                                                                              \
    hipEvent_t _a = nullptr, _b = nullptr;                                                          \
    take_launch_events(&_a, &_b);                                                                   \
    if (_a || _b) hipExtLaunchKernelGGL(kern, grid, block, 0, stream, _a, _b, 0, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kern, grid, block, 0, stream, __VA_ARGS__);                             \
  } while (0)

void launch_shuffle_status(const ShufflePlan& pl, const uint8_t* d_status, Aff* d_pts, const Aff& gen, const uint32_t* d_perm, const Fr* d_blinders, Fr* d_msc,
                           Jac* d_mjac, uint8_t* d_bad, hipStream_t s) {
  if (!pl.count) return;
  if (pl.verifier) SHF_LAUNCH(k_shuffle_status<true>, dim3(pl.count), dim3(64), s, pl, d_status, d_pts, gen, d_perm, d_blinders, d_msc, d_mjac, d_bad);
  else SHF_LAUNCH(k_shuffle_status<false>, dim3(pl.count), dim3(64), s, pl, d_status, d_pts, gen, d_perm, d_blinders, d_msc, d_mjac, d_bad);
}
void launch_shuffle_gather(const ShufflePlan& pl, const uint32_t* d_perm, const Aff* d_kr, const Aff* d_ks, Aff* d_t, Aff* d_u, Aff* d_zipped, hipStream_t s) {
  if (!pl.count) return;
  SHF_LAUNCH(k_shuffle_gather, dim3((unsigned)((pl.plane_points() + 255) / 256)), dim3(256), s, pl, d_perm, d_kr, d_ks, d_t, d_u, d_zipped);
}
void launch_shuffle_commit(const Aff* d_pp, size_t pp_stride, uint32_t m_slot, uint32_t count, Jac* d_mjac, hipStream_t s) {
  if (!count) return;
  SHF_LAUNCH(k_shuffle_commit, dim3((count + 255) / 256), dim3(256), s, d_pp, pp_stride, m_slot, count, d_mjac);
}

}  // namespace cpx
