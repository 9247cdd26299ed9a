// The grand-product layer of cpx_gprod_prove ahead of the inner-product prover (gfx950) — product code.
//
// GrandProductProof::new (grand_product_argument.rs:43-166) for a lone statement on the caller's bases is the prefix products, C, r_p, the
// challenges alpha and beta, vec_d and D, then InnerProductProof::new on G | H and G' = u o (G | H).  Around the kernels of this file the
// call runs k_finalize over B, the tier-0 MSM chain over the C tasks and the D tasks, k_finalize over C, and then the steps of
// cpx_ipa_prove (subarg_prove.hip, loop.hip) on the same device memory with u as the fold coefficients of G'.  Layouts: gprod_plan.hpp on
// top of subarg_prove_plan.hpp; the algebra: gprod_algebra.hpp.
//
//  k_gprod_products   vec_c = 1, b_0, b_0 b_1, ... (:69-73) as a work-group scan over Fr products — a chunk of consecutive factors per
//                     thread, the chunks' products combined in seven steps across the work-group, every thread then writes its positions —, vec_c_blinders behind it:
//                     the IPA's witness c, and the scalars of the C task.
//  k_gprod_setup      wave 0: gprod_step1 (B, gprod_result), alpha, r_p, gprod_step2 (C, r_p), beta on the item's transcript state
//                     (wave_strobe.hpp), the one inversion for beta^-1, inner_prod into the IPA's z.  All lanes: u, vec_d | vec_d_blinders
//                     (the IPA's witness d) and the D task's scalars.
//  k_gprod_rdu        r_d o u: the scalars of B_d = <r_d, G'> over the points of G | H themselves.
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "modinv30.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "kernels.h"
#include "round_algebra.hpp"
#include "gprod_algebra.hpp"

namespace cpx {

#define LBL(s) s, (sizeof(s) - 1)

__global__ __launch_bounds__(GPROD_THREADS) void k_gprod_products(const GprodDev d) {
  __shared__ Fr part[2][GPROD_THREADS];   // the log-step combination reads one half and writes the other
  const GprodProvePlan& pl = d.pl;
  const size_t item = blockIdx.x;
  const int ell = (int)pl.ell(), nb = (int)pl.nb(), tid = threadIdx.x;
  const Fr* b = d.fr + pl.fr_b() + item * pl.ell();
  const Fr* cbl = d.fr + pl.fr_cbl() + item * pl.nb();
  Fr* c = d.fr + pl.sp.fr_wit() + item * 2 * pl.n();
  int lo, hi;
  gprod_chunk(ell, GPROD_THREADS, tid, lo, hi);
  part[0][tid] = gprod_chunk_product(b, lo, hi);
  __syncthreads();
  int cur = 0;
  for (int off = 1; off < GPROD_THREADS; off <<= 1, cur ^= 1) {
    part[cur ^ 1][tid] = gprod_scan_step(part[cur], tid, off);
    __syncthreads();
  }
  gprod_chunk_fixup(b, lo, hi, tid ? part[cur][tid - 1] : Fr::one(), c);
  for (int k = tid; k < nb; k += GPROD_THREADS) c[ell + k] = cbl[k];
}

__global__ __launch_bounds__(GPROD_THREADS) void k_gprod_setup(const GprodDev d) {
  __shared__ Fr sh[5];   // alpha, beta, beta^-1, beta^(ell+1), beta^-(ell+1)
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const GprodProvePlan& pl = d.pl;
  const size_t item = blockIdx.x;
  const int ell = (int)pl.ell(), nb = (int)pl.nb(), tid = threadIdx.x;
  const Fr* b = d.fr + pl.fr_b() + item * pl.ell();
  const Fr* rb = d.fr + pl.fr_rb() + item * pl.nb();
  if (tid < 64) {   // (uniform over each wave)
    uint64_t* st = d.states + item * 27;
    const Fr* cbl = d.fr + pl.fr_cbl() + item * pl.nb();
    const Fr result = d.fr[pl.fr_result() + item];
    WaveStrobe t;
    t.load(st, tid);
    t.append_message(LBL("gprod_step1"), d.bytes + pl.by_B() + item * 48, 48, scratch);   // grand_product_argument.rs:63-65
    t.append_scalar(LBL("gprod_step1"), result, scratch);
    const Fr alpha = t.challenge_scalar(LBL("gprod_alpha"), scratch);
    const Fr r_p = gprod_r_p(rb, cbl, nb, alpha);                                         // :79-81 (every lane: the transcript takes it uniform)
    t.append_message(LBL("gprod_step2"), d.bytes + pl.by_C() + item * 48, 48, scratch);   // :83-85
    t.append_scalar(LBL("gprod_step2"), r_p, scratch);
    const Fr beta = t.challenge_scalar(LBL("gprod_beta"), scratch);
    t.store(st);
    if (tid == 0) {
      const bool no_inverse = beta.is_zero();                                             // :86
      const Fr beta_inv = no_inverse ? Fr::zero() : fr_inv_divsteps(beta);
      const Fr beta_l = gprod_pow(beta, (uint64_t)ell);
      sh[0] = alpha;
      sh[1] = beta;
      sh[2] = beta_inv;
      sh[3] = fe_mul(beta_l, beta);
      sh[4] = gprod_pow(beta_inv, (uint64_t)ell + 1);
      d.fr[pl.fr_chal() + 2 * item] = alpha;
      d.fr[pl.fr_chal() + 2 * item + 1] = beta;
      d.fr[pl.fr_rp() + item] = r_p;
      d.fr[pl.sp.fr_z() + item] = gprod_inner_prod(r_p, result, beta_l, beta);            // :141-142
      d.flags[pl.flag_beta() + item] = no_inverse ? 1 : 0;
    }
  }
  __syncthreads();
  Fr* u = d.fr + pl.fr_u() + item * pl.n();
  Fr* dsc = d.fr + pl.fr_dsc() + item * pl.n();
  Fr* vd = d.fr + pl.sp.fr_wit() + item * 2 * pl.n() + pl.n();
  int lo, hi;
  gprod_chunk(ell, GPROD_THREADS, tid, lo, hi);
  gprod_fill_chunk(b, lo, hi, sh[1], sh[2], u, vd, dsc);
  gprod_fill_blinders(rb, ell, nb, tid, GPROD_THREADS, sh[0], sh[3], sh[4], u, vd, dsc);
}

__global__ __launch_bounds__(GPROD_THREADS) void k_gprod_rdu(const GprodDev d) {
  const GprodProvePlan& pl = d.pl;
  const size_t item = blockIdx.x, n = pl.n();
  const Fr* rd = d.fr + pl.sp.fr_rd() + item * n;
  const Fr* u = d.fr + pl.fr_u() + item * n;
  Fr* out = d.fr + pl.fr_rdu() + item * n;
  for (size_t i = threadIdx.x; i < n; i += GPROD_THREADS) out[i] = fe_mul(rd[i], u[i]);
}

// The verifier's steps ahead of InnerProductProof::verify (grand_product_argument.rs:201-231) for one item per work-group: the
// deserialisation verdict of C (the decoder's status) and r_p (canonical), gprod_step1 / gprod_step2 with alpha and beta on the item's
// transcript state (wave 0), the one inversion, and what cpx_ipa_verify's steps take from here: z = inner_prod, vec_u, and the two scalars
// -beta^-1 and alpha of D = B - beta^-1 crs_G_sum + alpha crs_H_sum.  An item that does not deserialise gets zeros.
__global__ __launch_bounds__(GPROD_THREADS) void k_gprod_verify_steps(const GprodVerifyDev d) {
  __shared__ Fr sh[2];   // beta^-1, beta^-(ell+1)
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const size_t item = blockIdx.x;
  const GprodCheckPlan& pl = d.pl;
  const int n = (int)pl.sp.n, ell = (int)pl.ell, tid = threadIdx.x;
  const uint8_t* head = d.bytes + pl.by_heads() + item * GprodCheckPlan::kHead;   // C, r_p
  Fr* u = d.fr + pl.sp.fr_u() + item * pl.sp.n;
  Fr& z = d.fr[pl.sp.fr_z() + item];
  Fr &neg_beta_inv = d.fr[pl.fr_neg_beta_inv() + item], &alpha_out = d.fr[pl.fr_alpha() + item];
  Fr* chal = d.fr + pl.fr_chal() + 2 * item;
  Fr r_p;
  const bool bad = !load_scalar(head + pl.rp_byte(), r_p) || d.status[pl.st_C() + item] != 0;   // (uniform over the work-group)
  if (bad) {
    for (int i = tid; i < n; i += GPROD_THREADS) u[i] = Fr::zero();
    if (tid == 0) {
      d.status[pl.st_bad() + item] = 1;
      z = neg_beta_inv = alpha_out = chal[0] = chal[1] = Fr::zero();
    }
    return;
  }
  if (tid < 64) {   // (uniform over each wave)
    uint64_t* st = d.states + item * 27;
    const Fr result = d.fr[pl.fr_result() + item];
    WaveStrobe t;
    t.load(st, tid);
    t.append_message(LBL("gprod_step1"), d.bytes + pl.by_B() + item * 48, 48, scratch);   // :202-204
    t.append_scalar(LBL("gprod_step1"), result, scratch);
    const Fr alpha = t.challenge_scalar(LBL("gprod_alpha"), scratch);
    t.append_message(LBL("gprod_step2"), head, 48, scratch);                   // :207-209
    t.append_scalar(LBL("gprod_step2"), r_p, scratch);
    const Fr beta = t.challenge_scalar(LBL("gprod_beta"), scratch);
    t.store(st);
    if (tid == 0) {
      const Fr beta_inv = beta.is_zero() ? Fr::zero() : fr_inv_divsteps(beta);   // (:210; a challenge is never zero)
      sh[0] = beta_inv;
      sh[1] = gprod_pow(beta_inv, (uint64_t)ell + 1);
      d.status[pl.st_bad() + item] = 0;
      z = gprod_inner_prod(r_p, result, gprod_pow(beta, (uint64_t)ell), beta);   // :230-231
      neg_beta_inv = fe_neg(beta_inv);
      alpha_out = chal[0] = alpha;
      chal[1] = beta;
    }
  }
  __syncthreads();
  int lo, hi;
  gprod_chunk(n, GPROD_THREADS, tid, lo, hi);   // :214-220: beta^-(i+1), i < ell, then beta^-(ell+1)
  gprod_fill_u(lo, hi, ell, sh[0], sh[1], u);
}

void launch_gprod_verify_steps(const GprodVerifyDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_gprod_verify_steps, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}
void launch_gprod_products(const GprodDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_gprod_products, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}
void launch_gprod_setup(const GprodDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_gprod_setup, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}
void launch_gprod_rdu(const GprodDev& d, hipStream_t s) {
  if (!d.pl.count()) return;
  hipLaunchKernelGGL(k_gprod_rdu, dim3(d.pl.count()), dim3(GPROD_THREADS), 0, s, d);
}

}  // namespace cpx
