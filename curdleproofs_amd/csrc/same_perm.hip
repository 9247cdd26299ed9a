// The same-permutation layer of cpx_same_perm_prove / cpx_same_perm_verify ahead of the grand-product layer (gfx950) — product code.
//
// SamePermutationProof::new (same_permutation_argument.rs:40-99) for a lone statement on the caller's bases is step 1 of the transcript,
// the permuted factors with their product, vec_b_blinders and B = A + alpha M + beta sum G, then GrandProductProof::new.  Around the
// kernels of this file the call runs k_finalize over A | M (their encodings for step 1, M's affine form into the item's row), the tier-0
// MSM chain over the B tasks — beta on the ell positions of G, alpha on M —, and then the steps of cpx_gprod_prove (gprod.hip) on the same
// device memory, whose k_finalize over B adds A.  Layouts: same_perm_plan.hpp on top of gprod_plan.hpp; the algebra: same_perm_algebra.hpp.
//
//  k_same_perm_step          one work-group per item.  Step 1 (:60-63) on the item's transcript state (wave 0, wave_strobe.hpp): A, M, then
//                            vec_a as ONE message — the u64 length, then the canonical scalars, which the whole work-group converts into
//                            LDS SAME_PERM_PIECE at a time and wave 0 absorbs piece by piece, so ell is not bounded by LDS —, alpha, beta.
//                            All lanes: the factors through the permutation into the grand product's vec_b, vec_b_blinders, B's scalars;
//                            the product of the factors by the chunk products and log steps of k_gprod_products (gprod_algebra.hpp).
//  k_same_perm_verify_step   the verifier's twin (:134-145): step 1, the index factors' product into the grand-product check's gprod_result.
//  k_same_perm_weights       behind k_subarg_scalars: the relation of :149 with the item's factor a_0 joins the row of weights.
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "kernels.h"
#include "gprod_algebra.hpp"
#include "same_perm_algebra.hpp"

namespace cpx {

#define LBL(s) s, (sizeof(s) - 1)

// step 1 for one item, called by the whole work-group (it holds barriers); t is wave 0's.  alpha, beta: valid in wave 0
__device__ static void same_perm_step1(WaveStrobe& t, int tid, const uint8_t* enc_A, const uint8_t* enc_M, const Fr* a, int ell, uint32_t* piece, uint8_t* scratch, Fr& alpha,
                                       Fr& beta) {
  const bool w0 = tid < 64;   // (uniform over each wave)
  if (w0) {
    t.append_message(LBL("same_perm_step1"), enc_A, 48, scratch);   // :60
    t.append_message(LBL("same_perm_step1"), enc_M, 48, scratch);
    t.append_begin(LBL("same_perm_step1"), 8 + 32 * (size_t)ell, scratch);   // :61, vec_a as Vec<Fr>
    t.absorb(nullptr, 0, (uint32_t)ell, 4);
    t.absorb(nullptr, 0, 0, 4);
  }
  for (int base = 0; base < ell; base += SAME_PERM_PIECE) {
    const int cnt = ell - base < SAME_PERM_PIECE ? ell - base : SAME_PERM_PIECE;
    for (int i = tid; i < cnt; i += GPROD_THREADS) same_perm_canonical(a[base + i], piece + 8 * i);
    __syncthreads();
    if (w0) t.absorb(reinterpret_cast<const uint8_t*>(piece), 32 * (size_t)cnt);
    __syncthreads();
  }
  if (w0) {
    alpha = t.challenge_scalar(LBL("same_perm_alpha"), scratch);   // :62-63
    beta = t.challenge_scalar(LBL("same_perm_beta"), scratch);
  }
}

// the product of the work-group's chunk products part[0][*]: the log steps of k_gprod_products; the last thread holds the total
__device__ static Fr same_perm_total(Fr (*part)[GPROD_THREADS], int tid) {
  int cur = 0;
  for (int off = 1; off < GPROD_THREADS; off <<= 1, cur ^= 1) {
    part[cur ^ 1][tid] = gprod_scan_step(part[cur], tid, off);
    __syncthreads();
  }
  return part[cur][tid];
}

__global__ __launch_bounds__(GPROD_THREADS) void k_same_perm_step(const SamePermDev d) {
  __shared__ Fr part[2][GPROD_THREADS];
  __shared__ __attribute__((aligned(16))) uint32_t piece[SAME_PERM_PIECE * 8];
  __shared__ Fr sh[2];   // alpha, beta
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const SamePermProvePlan& pl = d.pl;
  const GprodProvePlan& gp = pl.gp;
  const size_t item = blockIdx.x;
  const int ell = (int)pl.ell(), nb = (int)pl.nb(), tid = threadIdx.x;
  const Fr* a = d.fr + pl.fr_a() + item * pl.ell();
  const uint32_t* perm = d.perm + item * pl.ell();
  uint64_t* st = d.states + item * 27;
  WaveStrobe t;
  if (tid < 64) t.load(st, tid);
  Fr alpha, beta;
  same_perm_step1(t, tid, d.bytes + pl.by_A() + item * 48, d.bytes + pl.by_M() + item * 48, a, ell, piece, scratch, alpha, beta);
  if (tid < 64) {
    t.store(st);
    if (tid == 0) {
      sh[0] = d.fr[pl.fr_chal() + 2 * item] = alpha;
      sh[1] = d.fr[pl.fr_chal() + 2 * item + 1] = beta;
    }
  }
  __syncthreads();
  alpha = sh[0];
  beta = sh[1];
  Fr* b = d.fr + gp.fr_b() + item * pl.ell();
  Fr* bsc = d.fr + pl.fr_bsc() + item * (pl.ell() + 1);
  int lo, hi;
  gprod_chunk(ell, GPROD_THREADS, tid, lo, hi);
  part[0][tid] = same_perm_fill_chunk(a, perm, lo, hi, alpha, beta, b);   // :66-72
  for (int i = lo; i < hi; i++) bsc[i] = beta;                             // :75-76
  if (tid == 0) bsc[ell] = alpha;
  const Fr *ra = d.fr + pl.fr_ra() + item * pl.nb(), *rm = d.fr + pl.fr_rm() + item * pl.nb();
  Fr* rb = d.fr + gp.fr_rb() + item * pl.nb();
  for (int k = tid; k < nb; k += GPROD_THREADS) rb[k] = same_perm_blinder(ra[k], rm[k], alpha);   // :78-81
  __syncthreads();
  const Fr total = same_perm_total(part, tid);   // :73
  if (tid == GPROD_THREADS - 1) d.fr[gp.fr_result() + item] = total;
}

__global__ __launch_bounds__(GPROD_THREADS) void k_same_perm_verify_step(const SamePermVerifyDev d) {
  __shared__ Fr part[2][GPROD_THREADS];
  __shared__ __attribute__((aligned(16))) uint32_t piece[SAME_PERM_PIECE * 8];
  __shared__ Fr sh[2];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const SamePermCheckPlan& pl = d.pl;
  const size_t item = blockIdx.x;
  const int ell = (int)pl.ell(), tid = threadIdx.x;
  const Fr* a = d.fr + pl.fr_a() + item * pl.ell();
  uint64_t* st = d.states + item * 27;
  WaveStrobe t;
  if (tid < 64) t.load(st, tid);
  Fr alpha, beta;
  same_perm_step1(t, tid, d.bytes + pl.by_A() + item * 48, d.bytes + pl.by_M() + item * 48, a, ell, piece, scratch, alpha, beta);   // :134-137
  if (tid < 64) {
    t.store(st);
    if (tid == 0) {
      sh[0] = d.fr[pl.fr_chal() + 2 * item] = alpha;
      sh[1] = d.fr[pl.fr_chal() + 2 * item + 1] = beta;
    }
  }
  __syncthreads();
  int lo, hi;
  gprod_chunk(ell, GPROD_THREADS, tid, lo, hi);
  part[0][tid] = same_perm_fill_chunk<Fr>(a, nullptr, lo, hi, sh[0], sh[1], nullptr);   // :140-145
  __syncthreads();
  const Fr total = same_perm_total(part, tid);
  if (tid == GPROD_THREADS - 1) d.fr[pl.gp.fr_result() + item] = total;
}

__global__ __launch_bounds__(GPROD_THREADS) void k_same_perm_weights(const SamePermVerifyDev d) {
  const SamePermCheckPlan& pl = d.pl;
  const size_t item = blockIdx.x;
  const int ell = (int)pl.ell(), tid = threadIdx.x;
  Fr* row = d.fr + pl.gp.sp.fr_weights() + item * pl.gp.sp.points();
  const SamePermWeights<Fr> w = same_perm_weights(d.fr[pl.fr_a0() + item], d.fr[pl.fr_chal() + 2 * item], d.fr[pl.fr_chal() + 2 * item + 1]);   // :149
  for (int i = tid; i < ell; i += GPROD_THREADS) row[i] = fe_add(row[i], w.g_add);
  if (tid == 0) {
    row[pl.row_B()] = w.B;
    row[pl.row_A()] = w.A;
    row[pl.row_M()] = w.M;
  }
}

void launch_same_perm_step(const SamePermDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_same_perm_step, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}
void launch_same_perm_verify_step(const SamePermVerifyDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_same_perm_verify_step, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}
void launch_same_perm_weights(const SamePermVerifyDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_same_perm_weights, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}

}  // namespace cpx
