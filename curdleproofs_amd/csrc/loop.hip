// The tail of one log round of cpx_ipa_rounds / cpx_same_msm_rounds (gfx950) — product code.
//
// A round of the loops inner_product_argument.rs:150-186 / same_multiscalar_argument.rs:99-136 in the all-MSM form is the MSM chain of
// cpx_g1_msm_many over the round's 4 / 6 cross terms of every item, k_finalize for their 48-byte encodings, and ONE launch of
// k_loop_step, which does for every item what the host did between two tier-0 calls: the transcript step on the item's own state, the
// challenge's inverse, the folds of the scalar vectors and fold coefficients, and the scalars of the next round's cross terms — so that
// nothing returns to the host between the call's upload and its download.  Layouts: loop_plan.hpp; the Fr algebra: round_algebra.hpp,
// shared with the batch prover's k_*_round_* kernels.
//
// One work-group of two waves per item.  Wave 0 carries the transcript (wave_strobe.hpp: one wave per transcript, the retry loop of
// get_and_append_challenge is uniform over it), then hands gamma and its inverse to both waves through LDS.
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "modinv30.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "kernels.h"
#include "round_algebra.hpp"

namespace cpx {

#define LBL(s) s, (sizeof(s) - 1)

constexpr int LOOP_THREADS = 128;

template <bool IPA> __global__ __launch_bounds__(LOOP_THREADS) void k_loop_step(const LoopDev d, int j) {
  __shared__ Fr red[2 * LOOP_THREADS];
  __shared__ Fr gam[2];
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  constexpr int TERMS = IPA ? 4 : 6;
  const size_t item = blockIdx.x;
  const int n = d.n, half = n >> (j + 1);
  if (threadIdx.x < 64) {   // (uniform over each wave)
    uint64_t* st = d.states + item * 27;
    const uint8_t* pts = d.comp + ((size_t)j * d.count + item) * TERMS * 48;
    WaveStrobe t;
    t.load(st, threadIdx.x);
    for (int q = 0; q < TERMS; q++) {
      if (IPA) t.append_message(LBL("ipa_loop"), pts + 48 * q, 48, scratch);
      else t.append_message(LBL("same_msm_loop"), pts + 48 * q, 48, scratch);
    }
    const Fr gamma = IPA ? t.challenge_scalar(LBL("ipa_gamma"), scratch) : t.challenge_scalar(LBL("same_msm_gamma"), scratch);
    t.store(st);
    const Fr gi = fr_inv_divsteps(gamma);
    if (threadIdx.x == 0) {
      gam[0] = gamma;
      gam[1] = gi;
      d.gammas[item * d.L + j] = gamma;
    }
  }
  __syncthreads();
  const Fr g = gam[0], gi = gam[1];
  Fr* vec = d.vec + item * (IPA ? 4 : 2) * (size_t)n;
  Fr* row = d.rows + item * (IPA ? 2 * (size_t)n + 2 : (size_t)n);
  if (IPA) ipa_round_fold_body(vec, vec + n, vec + 2 * (size_t)n, vec + 3 * (size_t)n, n, half, g, gi);
  else smsm_round_fold_body(vec, vec + n, n, half, g, gi);
  __threadfence_block();
  __syncthreads();
  if (half > 1) {   // the scalars of the next round's cross terms
    if (IPA) ipa_round_scalars_body(vec, vec + n, vec + 2 * (size_t)n, vec + 3 * (size_t)n, n, half / 2, Fr::one(), row, red);
    else smsm_round_scalars_body(vec, vec + n, n, half / 2, row);
  } else if (threadIdx.x == 0) {   // the last round: c[0], d[0] / x[0]
    d.finals[item * (IPA ? 2 : 1)] = vec[0];
    if (IPA) d.finals[item * 2 + 1] = vec[n];
  }
}

void launch_loop_step(bool ipa, const LoopDev& d, int j, hipStream_t s) {
  if (d.count <= 0) return;
  if (ipa) hipLaunchKernelGGL(k_loop_step<true>, dim3(d.count), dim3(LOOP_THREADS), 0, s, d, j);
  else hipLaunchKernelGGL(k_loop_step<false>, dim3(d.count), dim3(LOOP_THREADS), 0, s, d, j);
}

}  // namespace cpx
