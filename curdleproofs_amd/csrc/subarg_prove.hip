// The steps of cpx_ipa_prove / cpx_same_msm_prove before the log-round loop (gfx950) — product code.
//
// InnerProductProof::new (inner_product_argument.rs:98-199) and SameMultiscalarProof::new (same_multiscalar_argument.rs:69-150) for a lone
// statement on the caller's bases are the blinders, the B points, step 1 of the transcript, the rewrite of the witness by alpha and (IPA)
// H = beta crs_H, then the loop of cpx_ipa_rounds / cpx_same_msm_rounds (loop.hip) on the same device memory.  Around the two kernels of
// this file the call runs the tier-0 MSM chain over the B points, k_finalize over them and the statement points, for SameMSM k_compress
// over T | U, and for the IPA k_smul for H.  Layouts: subarg_prove_plan.hpp on top of loop_plan.hpp.
//
//  k_subarg_blinders      IPA only: generate_ipa_blinders (blinder_algebra.hpp) per item — omega and delta as sums over the work-group,
//                         the one inversion both inverses come from on thread 0, r_d = the z draws with the two solved entries, and the item's flag where the
//                         reference panics (r_d is zero then).
//  k_subarg_prove_setup   step 1 on the item's own transcript state (wave 0; wave_strobe.hpp), then all lanes write r + alpha v into the
//                         loop's vectors with unit fold coefficients.  A flagged item keeps its state and enters the loop with zeros.
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "modinv30.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "kernels.h"
#include "blinder_algebra.hpp"

namespace cpx {

#define LBL(s) s, (sizeof(s) - 1)

constexpr int SPROVE_THREADS = 128;

__global__ __launch_bounds__(SPROVE_THREADS) void k_subarg_blinders(const SubargProveDev d) {
  __shared__ Fr red[2 * SPROVE_THREADS];
  const SubargProvePlan pl = d.pl;
  const size_t item = blockIdx.x;
  const int n = (int)pl.n(), tid = threadIdx.x;
  const Fr* c = d.fr + pl.fr_wit() + item * 2 * (size_t)n;
  const Fr* dd = c + n;
  const Fr* r = d.fr + pl.fr_draws() + item * pl.draws_each();
  const Fr* z = r + n;   // n - 2 draws
  Fr* rd = d.fr + pl.fr_rd() + item * (size_t)n;
  Fr om = Fr::zero(), de = Fr::zero();
  ipa_blinder_partial(r, z, c, dd, n, tid, SPROVE_THREADS, om, de);
  red[tid] = om;
  red[SPROVE_THREADS + tid] = de;
  __syncthreads();
  for (int sft = SPROVE_THREADS / 2; sft >= 1; sft >>= 1) {
    if (tid < sft) {
      red[tid] = fe_add(red[tid], red[tid + sft]);
      red[SPROVE_THREADS + tid] = fe_add(red[SPROVE_THREADS + tid], red[SPROVE_THREADS + tid + sft]);
    }
    __syncthreads();
  }
  for (int i = tid; i < n - 2; i += SPROVE_THREADS) rd[i] = z[i];
  if (tid == 0) {
    const IpaBlinderTail t = ipa_blinder_solve(red[0], red[SPROVE_THREADS], r[n - 2], r[n - 1], c[n - 2], c[n - 1]);
    rd[n - 2] = t.pen_z;
    rd[n - 1] = t.last_z;
    d.flags[item] = t.singular ? 1 : 0;
  }
}

template <bool IPA> __global__ __launch_bounds__(SPROVE_THREADS) void k_subarg_prove_setup(const SubargProveDev d) {
  __shared__ Fr ab[2];   // alpha, beta
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const SubargProvePlan pl = d.pl;
  const size_t item = blockIdx.x;
  const int n = (int)pl.n(), tid = threadIdx.x;
  const bool flagged = IPA && d.flags[item] != 0;   // (uniform over the work-group)
  Fr* chal = d.fr + pl.fr_ab() + item * (IPA ? 2 : 1);
  if (tid < 64 && !flagged) {   // (uniform over each wave)
    uint64_t* st = d.states + item * 27;
    const uint8_t* pts = d.bytes + pl.by_points();
    const uint8_t* stmt = pts + pl.pt_statement(item, 0) * 48;   // crs_H C D resp. A Z_t Z_u
    const uint8_t* first = pts + pl.pt_first(item, 0) * 48;      // B_c B_d resp. B_a B_t B_u
    WaveStrobe t;
    t.load(st, tid);
    Fr alpha, beta = Fr::zero();
    if (IPA) {   // inner_product_argument.rs:129-134
      t.append_message(LBL("ipa_step1"), stmt + 48, 48, scratch);
      t.append_message(LBL("ipa_step1"), stmt + 96, 48, scratch);
      t.append_scalar(LBL("ipa_step1"), d.fr[pl.fr_z() + item], scratch);
      t.append_message(LBL("ipa_step1"), first, 48, scratch);
      t.append_message(LBL("ipa_step1"), first + 48, 48, scratch);
      alpha = t.challenge_scalar(LBL("ipa_alpha"), scratch);
      beta = t.challenge_scalar(LBL("ipa_beta"), scratch);
    } else {     // same_multiscalar_argument.rs:84-91
      for (int k = 0; k < 3; k++) t.append_message(LBL("same_msm_step1"), stmt + 48 * k, 48, scratch);
      const uint8_t* tu = d.bytes + pl.by_tu() + item * 2 * (size_t)n * 48;
      for (int which = 0; which < 2; which++) {   // vec_T, vec_U as Vec<G1Affine>: the length as u64, then the encodings
        t.append_begin(LBL("same_msm_step1"), 8 + 48 * (size_t)n, scratch);
        t.absorb(nullptr, 0, (uint32_t)n, 4);
        t.absorb(nullptr, 0, 0, 4);
        t.absorb(tu + (size_t)which * n * 48, 48 * (size_t)n);
      }
      for (int k = 0; k < 3; k++) t.append_message(LBL("same_msm_step1"), first + 48 * k, 48, scratch);
      alpha = t.challenge_scalar(LBL("same_msm_alpha"), scratch);
    }
    t.store(st);
    if (tid == 0) {
      ab[0] = chal[0] = alpha;
      if (IPA) ab[1] = chal[1] = beta;
    }
  }
  if (flagged && tid == 0) {
    ab[0] = chal[0] = Fr::zero();
    ab[1] = chal[1] = Fr::zero();
  }
  __syncthreads();
  // the loop's vectors: r + alpha v (inner_product_argument.rs:136-139, same_multiscalar_argument.rs:93-95), fold coefficients 1
  const Fr alpha = ab[0], one = Fr::one();
  const Fr* wit = d.fr + pl.fr_wit() + item * (IPA ? 2 : 1) * (size_t)n;
  const Fr* r = d.fr + pl.fr_draws() + item * pl.draws_each();
  Fr* vec = d.vec + item * (IPA ? 4 : 2) * (size_t)n;
  if (IPA) {
    const Fr* rd = d.fr + pl.fr_rd() + item * (size_t)n;
    const Fr* seed = d.sgp_seed ? d.sgp_seed + item * (size_t)n : nullptr;   // (uniform over the launch)
    for (int i = tid; i < n; i += SPROVE_THREADS) {
      vec[i] = flagged ? Fr::zero() : fe_add(r[i], fe_mul(alpha, wit[i]));
      vec[n + i] = flagged ? Fr::zero() : fe_add(rd[i], fe_mul(alpha, wit[n + i]));
      vec[2 * (size_t)n + i] = one;
      vec[3 * (size_t)n + i] = seed ? seed[i] : one;
    }
    if (tid == 0) d.ones[item] = one;   // (H is beta crs_H already: the rounds' shared formulas multiply by 1)
  } else {
    for (int i = tid; i < n; i += SPROVE_THREADS) {
      vec[i] = fe_add(r[i], fe_mul(alpha, wit[i]));
      vec[n + i] = one;
    }
    if (n == 1 && tid == 0) d.finals[item] = fe_add(r[0], fe_mul(alpha, wit[0]));   // L = 0: no round writes x_final
  }
}

void launch_subarg_blinders(const SubargProveDev& d, hipStream_t s) {
  if (!d.pl.count() || !d.pl.ipa()) return;
  hipLaunchKernelGGL(k_subarg_blinders, dim3(d.pl.count()), dim3(SPROVE_THREADS), 0, s, d);
}
void launch_subarg_prove_setup(const SubargProveDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  if (d.pl.ipa()) hipLaunchKernelGGL(k_subarg_prove_setup<true>, dim3(d.pl.count()), dim3(SPROVE_THREADS), 0, s, d);
  else hipLaunchKernelGGL(k_subarg_prove_setup<false>, dim3(d.pl.count()), dim3(SPROVE_THREADS), 0, s, d);
}

}  // namespace cpx
