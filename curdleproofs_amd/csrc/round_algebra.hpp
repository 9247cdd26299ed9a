// Fr algebra of one log round of the all-MSM form for ONE item on the threads of its work-group — device code.
// The bodies of k_ipa_round_scalars / k_ipa_round_fold / k_smsm_round_scalars / k_smsm_round_fold (kernels.hip: the batch prover's
// stand-alone launches) and of k_loop_step (loop.hip: the whole tail of a round of cpx_ipa_rounds / cpx_same_msm_rounds), written once.
// At the end load_scalar, a proof's scalar off the wire, for the verifier kernels (protocol.hip k_vs_prefix, subarg.hip k_subarg_scalars).
//
// Round j of n = 2^L elements: half = n >> (j+1); original base k has bit `half` set (hi) or clear (lo); the t-th lo index is
// kl = (t / half) * 2 half + t % half, the t-th hi index kh = kl + half (t < n/2) — the lists loop_plan.hpp hands the MSM tasks.
// Every function is called by all threads of the work-group (blockDim.x of them) and orders nothing: the caller puts a barrier
// between a fold and the scalars that read it.
#pragma once
#include <hip/hip_runtime.h>
#include "mont32.hpp"

namespace cpx {

// IPA (inner_product_argument.rs:150-163).  c | d | SG | SGp of n elements each;
// o = [ L_C scalars (n/2), beta<c_L,d_R> | L_D (n/2) | R_C (n/2), beta<c_R,d_L> | R_D (n/2) ];  red: 2 blockDim.x entries of LDS
__device__ __forceinline__ void ipa_round_scalars_body(const Fr* __restrict__ c, const Fr* __restrict__ d, const Fr* __restrict__ SG, const Fr* __restrict__ SGp, int n,
                                                       int half, const Fr& beta, Fr* __restrict__ o, Fr* red) {
  const int hn = n / 2, nt = blockDim.x;
  Fr* red0 = red;
  Fr* red1 = red + nt;
  Fr ip1 = Fr::zero(), ip2 = Fr::zero();
  for (int t = threadIdx.x; t < hn; t += nt) {
    const int kl = (t / half) * 2 * half + (t % half), kh = kl + half;
    const int ih = kh & (half - 1), il = kl & (half - 1);
    o[t] = fe_mul(c[ih], SG[kh]);                          // L_C : right-half bases with c_L
    o[hn + 1 + t] = fe_mul(d[half + il], SGp[kl]);         // L_D : left-half bases (rescaled) with d_R
    o[2 * hn + 1 + t] = fe_mul(c[half + il], SG[kl]);      // R_C : left-half bases with c_R
    o[3 * hn + 2 + t] = fe_mul(d[ih], SGp[kh]);            // R_D : right-half bases with d_L
  }
  for (int i = threadIdx.x; i < half; i += nt) {
    ip1 = fe_add(ip1, fe_mul(c[i], d[half + i]));
    ip2 = fe_add(ip2, fe_mul(c[half + i], d[i]));
  }
  red0[threadIdx.x] = ip1;
  red1[threadIdx.x] = ip2;
  __syncthreads();
  for (int sft = nt / 2; sft >= 1; sft >>= 1) {
    if ((int)threadIdx.x < sft) {
      red0[threadIdx.x] = fe_add(red0[threadIdx.x], red0[threadIdx.x + sft]);
      red1[threadIdx.x] = fe_add(red1[threadIdx.x], red1[threadIdx.x + sft]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    o[hn] = fe_mul(beta, red0[0]);
    o[3 * hn + 1] = fe_mul(beta, red1[0]);
  }
}
// c_L += gamma^-1 c_R, d_L += gamma d_R, SG[hi] *= gamma, SGp[hi] *= gamma^-1 (inner_product_argument.rs:174-184 on the scalar side)
__device__ __forceinline__ void ipa_round_fold_body(Fr* __restrict__ c, Fr* __restrict__ d, Fr* __restrict__ SG, Fr* __restrict__ SGp, int n, int half, const Fr& g,
                                                    const Fr& gi) {
  const int hn = n / 2, nt = blockDim.x;
  for (int i = threadIdx.x; i < half; i += nt) {
    c[i] = fe_add(c[i], fe_mul(gi, c[half + i]));
    d[i] = fe_add(d[i], fe_mul(g, d[half + i]));
  }
  for (int t = threadIdx.x; t < hn; t += nt) {
    const int kh = (t / half) * 2 * half + (t % half) + half;
    SG[kh] = fe_mul(SG[kh], g);
    SGp[kh] = fe_mul(SGp[kh], gi);
  }
}
// SameMSM (same_multiscalar_argument.rs:104-112).  x | SM;  o = [ L_* scalars (n/2) | R_* scalars (n/2) ]
__device__ __forceinline__ void smsm_round_scalars_body(const Fr* __restrict__ x, const Fr* __restrict__ SM, int n, int half, Fr* __restrict__ o) {
  const int hn = n / 2, nt = blockDim.x;
  for (int t = threadIdx.x; t < hn; t += nt) {
    const int kl = (t / half) * 2 * half + (t % half), kh = kl + half;
    o[t] = fe_mul(x[kh & (half - 1)], SM[kh]);                    // L_* : right-half bases with x_L
    o[hn + t] = fe_mul(x[(kl & (half - 1)) + half], SM[kl]);      // R_* : left-half bases with x_R
  }
}
// x_L += gamma^-1 x_R, SM[hi] *= gamma (same_multiscalar_argument.rs:126-134)
__device__ __forceinline__ void smsm_round_fold_body(Fr* __restrict__ x, Fr* __restrict__ SM, int n, int half, const Fr& g, const Fr& gi) {
  const int hn = n / 2, nt = blockDim.x;
  for (int i = threadIdx.x; i < half; i += nt) x[i] = fe_add(x[i], fe_mul(gi, x[half + i]));
  for (int t = threadIdx.x; t < hn; t += nt) {
    const int kh = (t / half) * 2 * half + (t % half) + half;
    SM[kh] = fe_mul(SM[kh], g);
  }
}

// ---- a scalar of a proof off the wire ----
// canonical little-endian scalar -> Montgomery; false (and zero) if >= r  (Fr::deserialize_compressed)
__device__ inline bool load_scalar(const uint8_t* b, Fr& out) {
  Fr c;
  CPX_UNROLL for (int j = 0; j < 8; j++) c.v[j] = (uint32_t)b[4 * j] | ((uint32_t)b[4 * j + 1] << 8) | ((uint32_t)b[4 * j + 2] << 16) | ((uint32_t)b[4 * j + 3] << 24);
  bool lt = false;
  for (int j = 7; j >= 0; j--) {
    if (c.v[j] != FrCfg::P[j]) {
      lt = c.v[j] < FrCfg::P[j];
      break;
    }
  }
  out = lt ? fe_to_mont(c) : Fr::zero();
  return lt;
}

}  // namespace cpx
