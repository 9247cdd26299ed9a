// The transcript and scalar step of cpx_ipa_verify / cpx_same_msm_verify (gfx950) — product code.
//
// InnerProductProof::verify (inner_product_argument.rs:202-326) and SameMultiscalarProof::verify (same_multiscalar_argument.rs:153-261)
// for a lone proof on the caller's bases are, flattened (subarg_check_plan.hpp), one MSM per item over a row of points.  Around this
// kernel the call decodes the proof's points (k_decompress), normalises the statement points (k_finalize), for SameMSM encodes T and U
// (k_compress), and after it runs the tier-0 MSM chain with one task per item.  k_subarg_scalars does for every item what stands between:
// the deserialisation verdict, the whole transcript of `verify` on the item's own state — step 1 and L rounds of appends and a
// challenge —, the L challenge inverses, and the item's row of weights.  An item that does not deserialise keeps its state, gets zero
// challenges and a row of zeros: its task sums to the identity and its flag carries the verdict.
//
// One work-group of two waves per item.  Wave 0 carries the transcript (wave_strobe.hpp: one wave per transcript, the retry loop of
// get_and_append_challenge is uniform over it) and inverts the challenges, one lane each; then all lanes write the row, every s_i and
// 1 / s_i from its index (verification_scalar: the field values ark_ff::batch_inversion gives the reference, without n inversions).
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "modinv30.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "kernels.h"
#include "round_algebra.hpp"
#include "subarg_check_plan.hpp"

namespace cpx {

#define LBL(s) s, (sizeof(s) - 1)

constexpr int SUBARG_THREADS = 128;
constexpr int SUBARG_MAX_L = 24;   // n <= kTier0ManyPoints

template <bool IPA> __global__ __launch_bounds__(SUBARG_THREADS) void k_subarg_scalars(const SubargDev d) {
  __shared__ Fr gam[2 * SUBARG_MAX_L];   // gamma_j | their inverses
  __shared__ Fr ab[2];                   // alpha, beta
  __shared__ __attribute__((aligned(16))) uint8_t scratch[64];
  const SubargCheckPlan pl = d.pl;
  const size_t item = blockIdx.x;
  const int n = (int)pl.n, L = (int)pl.L, tid = threadIdx.x, NP = (int)pl.points(), PP = (int)pl.proof_points();
  const uint8_t* proof = d.bytes + pl.by_proofs() + item * pl.proof_bytes();
  Fr* row = d.fr + pl.fr_weights() + item * (size_t)NP;
  Fr* chal = d.fr + pl.fr_challenges() + item * pl.challenges();
  // ---- the deserialisation verdict: every point decoded (status 0), every scalar canonical
  SubargTerms<Fr> w;
  bool ok = load_scalar(proof + pl.scalar_byte(0), w.fin[0]);
  if (IPA) ok &= load_scalar(proof + pl.scalar_byte(1), w.fin[1]);
  int badpt = 0;
  for (int q = tid; q < PP; q += SUBARG_THREADS) badpt |= d.status[item * (size_t)PP + q];
  const bool bad = __syncthreads_or(badpt) || !ok;   // (uniform over the work-group)
  if (tid == 0) d.bad[item] = bad ? 1 : 0;
  if (bad) {
    for (int i = tid; i < NP; i += SUBARG_THREADS) row[i] = Fr::zero();
    for (int i = tid; i < (int)pl.challenges(); i += SUBARG_THREADS) chal[i] = Fr::zero();
    return;
  }
  if (IPA) w.z = d.fr[pl.fr_z() + item];
  // ---- the transcript
  if (tid < 64) {   // (uniform over each wave)
    uint64_t* st = d.states + item * 27;
    const uint8_t* stmt = d.bytes + pl.by_statement() + item * SubargCheckPlan::kStatement * 48;   // crs_H C D resp. A Z_t Z_u
    WaveStrobe t;
    t.load(st, tid);
    Fr alpha, beta = Fr::zero();
    if (IPA) {   // inner_product_argument.rs:283-287
      t.append_message(LBL("ipa_step1"), stmt + 48, 48, scratch);
      t.append_message(LBL("ipa_step1"), stmt + 96, 48, scratch);
      t.append_scalar(LBL("ipa_step1"), w.z, scratch);
      t.append_message(LBL("ipa_step1"), proof + pl.point_byte(0), 48, scratch);
      t.append_message(LBL("ipa_step1"), proof + pl.point_byte(1), 48, scratch);
      alpha = t.challenge_scalar(LBL("ipa_alpha"), scratch);
      beta = t.challenge_scalar(LBL("ipa_beta"), scratch);
    } else {     // same_multiscalar_argument.rs:230-233
      for (int k = 0; k < 3; k++) t.append_message(LBL("same_msm_step1"), stmt + 48 * k, 48, scratch);
      const uint8_t* tu = d.bytes + pl.by_tu() + item * 2 * (size_t)n * 48;
      for (int which = 0; which < 2; which++) {   // vec_T, vec_U as Vec<G1Affine>: the length as u64, then the encodings
        t.append_begin(LBL("same_msm_step1"), 8 + 48 * (size_t)n, scratch);
        t.absorb(nullptr, 0, (uint32_t)n, 4);
        t.absorb(nullptr, 0, 0, 4);
        t.absorb(tu + (size_t)which * n * 48, 48 * (size_t)n);
      }
      for (int k = 0; k < 3; k++) t.append_message(LBL("same_msm_step1"), proof + pl.point_byte(k), 48, scratch);
      alpha = t.challenge_scalar(LBL("same_msm_alpha"), scratch);
    }
    for (int j = 0; j < L; j++) {
      for (int q = 0; q < pl.terms(); q++) {
        const uint8_t* p = proof + pl.point_byte(pl.round_slot(j, q));
        if (IPA) t.append_message(LBL("ipa_loop"), p, 48, scratch);
        else t.append_message(LBL("same_msm_loop"), p, 48, scratch);
      }
      const Fr g = IPA ? t.challenge_scalar(LBL("ipa_gamma"), scratch) : t.challenge_scalar(LBL("same_msm_gamma"), scratch);
      if (tid == 0) {
        gam[j] = g;
        chal[(IPA ? 2 : 1) + j] = g;
      }
    }
    t.store(st);
    if (tid == 0) {
      ab[0] = chal[0] = alpha;
      ab[1] = beta;
      if (IPA) chal[1] = beta;
    }
    wave_lds_sync();
    if (tid < L) gam[L + tid] = fr_inv_divsteps(gam[tid]);   // the L inverses, one lane each
  }
  __syncthreads();
  // ---- the row of weights
  w.alpha = ab[0];
  w.beta = ab[1];
  const Fr* a = d.fr + pl.fr_rand() + item * pl.checks();
  w.a[0] = a[0], w.a[1] = a[1];   // (constant indices: a run-time one would put the whole struct into scratch memory)
  if (!IPA) w.a[2] = a[2];
  w.gam = gam;
  w.gam_inv = gam + L;
  w.set(IPA);
  const Fr* u = d.fr + pl.fr_u() + item * (size_t)n;
  for (int i = tid; i < n; i += SUBARG_THREADS) {
    const Fr s_i = verification_scalar(w.gam, L, i);
    if (IPA) {
      row[i] = subarg_base_weight(w, true, 0, s_i, fe_mul(u[i], verification_scalar(w.gam_inv, L, i)));
    } else {
      CPX_UNROLL for (int f = 0; f < 3; f++) row[pl.base_off(f) + i] = subarg_base_weight(w, false, f, s_i, s_i);
    }
  }
  for (int s = tid; s < PP; s += SUBARG_THREADS) row[pl.proof_off() + s] = subarg_proof_weight(w, pl, s);
  if (tid < (int)SubargCheckPlan::kStatement) row[pl.statement_off() + tid] = subarg_statement_weight(w, IPA, tid);
}

void launch_subarg_scalars(const SubargDev& d, hipStream_t s) {
  if (!d.pl.count) return;
  if (d.pl.ipa) hipLaunchKernelGGL(k_subarg_scalars<true>, dim3(d.pl.count), dim3(SUBARG_THREADS), 0, s, d);
  else hipLaunchKernelGGL(k_subarg_scalars<false>, dim3(d.pl.count), dim3(SUBARG_THREADS), 0, s, d);
}

}  // namespace cpx
