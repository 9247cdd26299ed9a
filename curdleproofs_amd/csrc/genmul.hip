// gfx950 kernels of the fixed-base multiplication by the G1 generator (whisk.rs:45-55 WhiskTracker::from_k_r, :370 get_k_commitment for
// `count` items per call; whisk.cpp drives them).  Layout, window width and recoding are gen_table.hpp's.
//
//  k_gen_table   one lane per table entry j 256^w G: j G by an 8-step double-and-add, 8 w doublings, one batch inversion per work-group
//                (block_inverse.hpp).  One launch, once per context.
//  k_gen_mul     one lane per scalar: the scalar (for a tracker's second point the Fr product k r, formed in the same lane) is split and
//                recoded once, then 16 windows x 2 halves = 32 mixed additions on an extended-Jacobian accumulator, no doubling.  Every lane
//                of a wave walks the same 32 steps: a zero digit adds the identity (the complete addition returns its other operand), a dead
//                lane multiplies by zero.  An accumulator that meets a table entry equal or opposite to itself takes the doubling / identity
//                branch of the complete mixed addition (g1_28.hpp xyzz28_add_mixed; tests/device/field_check.hip pins those branches).  One
//                batch inversion per work-group normalises the results; compression is the existing k_compress.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "g1.hpp"
#include "g1_28.hpp"
#include "glv.hpp"
#include "gen_table.hpp"
#include "kernels.h"
#include "block_inverse.hpp"

namespace cpx {

constexpr int GEN_THREADS = 64;   // single-wave groups, as k_smul

__global__ __launch_bounds__(GEN_THREADS) void k_gen_table(Aff gen, TAff* __restrict__ tab) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);   // 2 * GEN_THREADS field elements
  const int e = blockIdx.x * GEN_THREADS + threadIdx.x;
  const bool live = e < GEN_TABLE_ENTRIES;
  TJac acc = TJac::identity();
  if (live) {
    const TAff G = t_from_std(gen);
    const int j = gen_entry_multiple(e), w = gen_entry_window(e);
    for (int b = GEN_WINDOW_BITS - 1; b >= 0; b--) {   // j <= 128: 8 bits
      acc = t_dbl(acc);
      if ((j >> b) & 1) acc = t_add_mixed(acc, G);
    }
    for (int i = 0; i < GEN_WINDOW_BITS * w; i++) acc = t_dbl(acc);
  }
  const TF zinv = t_block_batch_inverse(acc.z, buf);
  if (live) tab[e] = t_to_affine(acc, zinv);   // (j 256^w < r: never the identity)
}

// mode GEN_MUL_PLAIN:     n = count lanes,      out[g] = a[g] G
// mode GEN_MUL_TRACKERS:  n = 2 count lanes,    out[2 i] = r_i G, out[2 i + 1] = (k_i r_i) G             (a = k, b = r)
// mode GEN_MUL_BOTH:      n = 3 count lanes,    the trackers as above, then out[2 count + i] = k_i G
// Scalars are Fr in Montgomery form.  Limbs that are not a reduced field element are not rejected: they stand for limbs / 2^256 mod r, the
// way k_smul reads its scalars.
__global__ __launch_bounds__(GEN_THREADS) void k_gen_mul(const Fr* __restrict__ a, const Fr* __restrict__ b, int count, int mode, const TAff* __restrict__ tab,
                                                         Aff* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);
  const long g = (long)blockIdx.x * GEN_THREADS + threadIdx.x;
  const long n = (long)count * (mode == GEN_MUL_PLAIN ? 1 : mode == GEN_MUL_TRACKERS ? 2 : 3);
  const bool live = g < n;
  Fr s = Fr::zero();
  if (live) {
    if (mode == GEN_MUL_PLAIN || g >= 2L * count) {
      s = fe_from_mont(a[mode == GEN_MUL_PLAIN ? g : g - 2L * count]);
    } else {
      const long i = g >> 1;
      s = fe_from_mont(b[i]);
      if (g & 1) s = fe_mul(s, a[i]);   // canonical r times the Montgomery limbs of k: the canonical product k r
    }
  }
  GenDigits dg;
  gen_recode(s.v, dg);
  TAcc acc = TAcc::identity();
#pragma unroll 1
  for (int w = 0; w < GEN_WINDOWS; w++) {
#pragma unroll 1
    for (int h = 0; h < 2; h++) {
      const GenPick pk = gen_pick(dg, h, w);
      const int idx = pk.index < 0 ? 0 : (pk.index < GEN_TABLE_ENTRIES ? pk.index : GEN_TABLE_ENTRIES - 1);
      TAff e = tab[idx];
      if (h) e.x = t_mul(e.x, t_beta());        // N P = -phi(P) = (beta x, -y)  (glv.hpp)
      e = t_cneg(e, pk.neg != (h == 1));
      if (pk.index < 0) e = TAff::identity();   // a zero digit runs on the identity
      acc = t_acc_add_mixed(acc, e);
    }
  }
  const TJac res = t_acc_to_jac(acc);
  const bool inf = res.is_identity();
  const TF zinv = t_block_batch_inverse(res.z, buf);
  if (!live) return;
  out[g] = inf ? Aff::identity() : t_to_std(t_to_affine(res, zinv));
}

#define GEN_LAUNCH(kern, grid, block, lds, stream, ...)                                             \
  do {                                                                                                \
    hipEvent_t _a = nullptr, _b = nullptr;                                                            \
    take_launch_events(&_a, &_b);                                                                     \
    if (_a || _b) hipExtLaunchKernelGGL(kern, grid, block, lds, stream, _a, _b, 0, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                             \
  } while (0)

size_t gen_table_entries() { return GEN_TABLE_ENTRIES; }
void launch_gen_table(const Aff& gen, TAff* d_tab, hipStream_t s) {
  GEN_LAUNCH(k_gen_table, dim3((GEN_TABLE_ENTRIES + GEN_THREADS - 1) / GEN_THREADS), dim3(GEN_THREADS), 2 * GEN_THREADS * sizeof(TF), s, gen, d_tab);
}
void launch_gen_mul(const Fr* d_a, const Fr* d_b, int count, int mode, const TAff* d_tab, Aff* d_out, hipStream_t s) {
  if (count <= 0) return;
  const long n = (long)count * (mode == GEN_MUL_PLAIN ? 1 : mode == GEN_MUL_TRACKERS ? 2 : 3);
  GEN_LAUNCH(k_gen_mul, dim3((unsigned)((n + GEN_THREADS - 1) / GEN_THREADS)), dim3(GEN_THREADS), 2 * GEN_THREADS * sizeof(TF), s, d_a, d_b, count, mode, d_tab, d_out);
}

}  // namespace cpx
