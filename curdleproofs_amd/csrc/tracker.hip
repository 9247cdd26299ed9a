// gfx950 kernels of the batched Whisk tracker proofs (whisk.rs:183-263 for `count` independent proofs per call; whisk.cpp drives them).
//
//  k_tracker_challenge   one wave per proof on the lane-parallel STROBE (wave_strobe.hpp): the six-point transcript of both tracker-proof
//                        functions (whisk.rs:204-218, :243-257) and its one challenge.  Verifier form: leaves the challenge and the
//                        proof's deserialisation flag.  Prover form: also  s = blinder - c k  and the serialized proof A || B || s.
//  k_tracker_relations   the verifier's two relations  s G + c k_G == A,  s r_G + c k_r_G == B  (whisk.rs:219-223): one QUAD per relation,
//                        16 relations per wave, a two-base joint ladder over the schedule of tracker_ladder.hpp on the quad-cooperative
//                        XYZZ formulas (g1_28_quad.hpp), built like k_smul_quad.  The claimed point is subtracted at the end and the
//                        accumulator tested for the identity: no inversion, normalisation or compression anywhere in the verifier.
//  k_tracker_check_scalars   the grouped / fused check (tracker_check_plan.hpp): both relations weighted by the caller's a, b and summed per
//                        group of items are ONE MSM — this kernel writes every group task's bases and scalars, a work-group per task; the
//                        bucket MSM behind it is the tier-0 chain (k_to_table_endo + k_msm_tblw<2, true> + k_reduce_sets + k_msm_tail).
//  k_tracker_gather      the compaction in front of k_tracker_relations when a group's sum is not the identity: the suspects, dense.
// Decoding, the prover's scalar multiplications and its compression are the existing kernels (k_decompress / k_decompress_quad, k_smul /
// k_smul_quad, k_compress).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "../../include/cpx.h"
#include "g1.hpp"
#include "g1_28.hpp"
#include "g1_28_quad.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "recode.hpp"
#include "glv.hpp"
#include "tracker_ladder.hpp"
#include "tracker_check_plan.hpp"
#include "kernels.h"

namespace cpx {

namespace {
__constant__ uint8_t kGenComp[48] = CPX_G1_GENERATOR_COMPRESSED;

#define TRK_LABEL(s) s, sizeof(s) - 1

// 32 little-endian bytes (4-byte aligned) -> 8 words; false if the value is not below r (`Fr::deserialize_compressed`)
__device__ __forceinline__ bool load_canonical_fr(const uint8_t* b, Fr& out) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(b);
  CPX_UNROLL for (int j = 0; j < 8; j++) out.v[j] = w[j];
  bool lt = false;
  for (int j = 7; j >= 0; j--) {
    if (out.v[j] != FrCfg::P[j]) {
      lt = out.v[j] < FrCfg::P[j];
      break;
    }
  }
  return lt;
}
}  // namespace

// Verifier form (PROVER = false).  in = trackers [count][96] | k_commitments [count][48] | proofs [count][128]; status: the decoding
// verdicts of the 5 count points, plane-major (A, B, k_r_G, r_G, k_G: tracker_point_offsets).  Writes chal[p] (canonical) and bad[p] = 1
// where a point did not decode or s >= r.
// Prover form.  in = trackers [count][96]; comp = k_G | A | B, [3][count][48] (the compressed results of the scalar multiplications);
// status: r_G, k_r_G plane-major; k, blinder in Montgomery form.  Writes proofs_out[p] = A || B || s (128 zero bytes for an undecodable
// tracker) and verdict[p] = CPX_OK / CPX_ERR_DESERIALIZE.
template <bool PROVER>
__global__ __launch_bounds__(64) void k_tracker_challenge(const uint8_t* __restrict__ in, const uint8_t* __restrict__ comp, const uint8_t* __restrict__ status,
                                                          const Fr* __restrict__ k, const Fr* __restrict__ blinder, int count, Fr* __restrict__ chal,
                                                          uint8_t* __restrict__ bad, uint8_t* __restrict__ proofs_out, int* __restrict__ verdict) {
  __shared__ uint8_t scratch[64];
  const int p = blockIdx.x, lane = threadIdx.x;
  if (p >= count) return;
  const size_t cnt = (size_t)count;
  const uint8_t* trk = in + 96 * (size_t)p;
  const uint8_t* prf = PROVER ? nullptr : in + 144 * cnt + 128 * (size_t)p;
  // skipped proofs leave the wave as a whole: every lane reads the same flags
  bool is_bad = false;
  for (int j = 0; j < (PROVER ? 2 : 5); j++) is_bad |= status[(size_t)j * cnt + p] != 0;
  if (!PROVER) {
    Fr s;
    is_bad |= !load_canonical_fr(prf + 96, s);
    if (lane == 0) bad[p] = is_bad ? 1 : 0;
  }
  if (is_bad) {
    if (PROVER) {
      proofs_out[128 * (size_t)p + lane] = 0;
      proofs_out[128 * (size_t)p + 64 + lane] = 0;
      if (lane == 0) verdict[p] = CPX_ERR_DESERIALIZE;
    }
    return;
  }
  // The reference hashes serialize_compressed of the DECODED points.  A point that decodes has exactly one compressed encoding — x < p is
  // checked, the sort bit is fixed by y, and an infinity encoding is canonical by now (k_decompress accepts only 0xc0 || 0^47; with
  // strict_infinity = 0 the host rewrote the others before the upload) — so the input bytes ARE those encodings and are hashed as they
  // came; the single-proof path's decode / re-compress round trip (whisk.cpp) is not needed.
  const uint8_t* k_g = PROVER ? comp + 48 * (size_t)p : in + 96 * cnt + 48 * (size_t)p;
  const uint8_t* a_pt = PROVER ? comp + 48 * (cnt + p) : prf;
  const uint8_t* b_pt = PROVER ? comp + 48 * (2 * cnt + p) : prf + 48;
  WaveStrobe t;
  t.set_lane(lane);
  t.init(TRK_LABEL("whisk_opening_proof"), scratch);
  for (int j = 0; j < 6; j++) {   // k_G, G, k_r_G, r_G, A, B (whisk.rs:204-216)
    const uint8_t* pt = j == 0 ? k_g : j == 1 ? kGenComp : j == 2 ? trk + 48 : j == 3 ? trk : j == 4 ? a_pt : b_pt;
    t.append_message(TRK_LABEL("tracker_opening_proof"), pt, 48, scratch);
  }
  Fr c;
  while (!t.challenge_attempt(TRK_LABEL("tracker_opening_proof_challenge"), scratch, c)) {
  }
  if (!PROVER) {
    if (lane == 0) chal[p] = c;
    return;
  }
  const Fr s = fe_from_mont(fe_sub(blinder[p], fe_mul(fe_to_mont(c), k[p])));   // s = blinder - c k (whisk.rs:259), canonical
  uint8_t* out = proofs_out + 128 * (size_t)p;
  if (lane < 48) {
    out[lane] = a_pt[lane];
    out[48 + lane] = b_pt[lane];
  }
  if (lane == 0) {
    uint32_t* sw = reinterpret_cast<uint32_t*>(out + 96);
    CPX_UNROLL for (int j = 0; j < 8; j++) sw[j] = s.v[j];
    verdict[p] = CPX_OK;
  }
}

// pts: the decoded points [5][count] (A, B, k_r_G, r_G, k_G); proofs [count][128] (s at byte 96); chal / bad: k_tracker_challenge's.
// Relation g = 2 p + j of proof p: j = 0  s G + c k_G - A,  j = 1  s r_G + c k_r_G - B.  verdict[p] = CPX_OK iff both sums are the identity,
// CPX_ERR_DESERIALIZE where bad[p].  Control flow is uniform over the wave: dead quads and skipped proofs run on the identity, and every
// lane reaches every barrier.
constexpr int TR_IDENT = 16 * TL_PER_REL;
constexpr size_t TR_LDS = (size_t)(TR_IDENT + 1) * sizeof(TAcc);
__global__ __launch_bounds__(64) void k_tracker_relations(const Aff* __restrict__ pts, const uint8_t* __restrict__ proofs, const Fr* __restrict__ chal,
                                                          const uint8_t* __restrict__ bad, Aff gen, int count, int* __restrict__ verdict) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);
  const int lane = threadIdx.x, quad = lane >> 2, sub = lane & 3;
  const long g = (long)blockIdx.x * 16 + quad;
  const bool in_range = g < 2L * count;
  const size_t p = (size_t)(g >> 1), cnt = (size_t)count;
  const int j = (int)(g & 1);
  const bool is_bad = in_range && bad[p] != 0;
  const bool live = in_range && !is_bad;
  const int base = quad * TL_PER_REL;
  TAcc* mine = buf + base;
  SmulNaf rs{}, rc{};
  if (live) {   // (replicated over the quad: the four lanes take identical branches)
    Fr s;
    (void)load_canonical_fr(proofs + 128 * p + 96, s);
    recode_smul_glv(s.v, rs);
    recode_smul_glv(chal[p].v, rc);
  }
  if (sub == 0) {
    mine[TL_ACC] = TAcc::identity();
    for (int b = 0; b < 2; b++) {
      TAcc XP = TAcc::identity(), XN = TAcc::identity();
      if (live) {
        const TAff P = t_from_std(b == 0 ? (j ? pts[3 * cnt + p] : gen) : pts[(j ? 2 : 4) * cnt + p]);
        if (!P.is_identity()) {
          XP = TAcc{P.x, P.y, t_one(), t_one()};
          XN = TAcc{t_mul(P.x, t_beta()), t_neg(P.y), t_one(), t_one()};   // N P = -phi(P) (glv.hpp)
        }
      }
      mine[TL_TAB + 8 * b + 0] = XP;
      mine[TL_TAB + 8 * b + 2] = XN;
    }
  }
  if (lane == 0) buf[TR_IDENT] = TAcc::identity();
  __syncthreads();
  auto neg_of = [](const TAcc& a) { return a.is_identity() ? a : TAcc{a.x, t_neg(a.y), a.zz, a.zzz}; };
  for (int b = 0; b < 2; b++) {   // P + N P, P - N P and the negatives, per base
    const int tb = base + TL_TAB + 8 * b;
    const TAcc sum = xyzz28_add_quad_mem(buf, tb + 0, tb + 2);
    if (sub == 0) {
      buf[tb + 4] = sum;
      buf[tb + 1] = neg_of(buf[tb + 0]);
      buf[tb + 3] = neg_of(buf[tb + 2]);
    }
    __syncthreads();
    const TAcc dif = xyzz28_add_quad_mem(buf, tb + 0, tb + 3);
    if (sub == 0) {
      buf[tb + 6] = dif;
      buf[tb + 5] = neg_of(sum);
      buf[tb + 7] = neg_of(dif);
    }
    __syncthreads();
  }
  for (int i = TRACKER_LADDER_TOP; i >= 0; i--) {
    const TAcc dbl = xyzz28_dbl_quad(buf[base + TL_ACC]);
    if (sub == 0) mine[TL_ACC] = dbl;
    __syncthreads();
    const TrackerStep st = tracker_ladder_step(rs, rc, i);
    CPX_UNROLL for (int b = 0; b < 2; b++) {
      const int e = st.e[b];
      if (!__any(e >= 0)) continue;   // (uniform: no quad of the wave adds from this base in this step)
      const TAcc sum = xyzz28_add_quad_mem(buf, base + TL_ACC, e >= 0 ? base + TL_TAB + 8 * b + e : TR_IDENT);
      if (sub == 0) mine[TL_ACC] = sum;
      __syncthreads();
    }
  }
  // - A resp. - B as an affine addend; the relation holds iff the sum is the identity
  if (sub == 0) {
    TAcc a = TAcc::identity();
    if (live) {
      const TAff C = t_from_std(pts[(size_t)j * cnt + p]);
      if (!C.is_identity()) a = TAcc{C.x, t_neg(C.y), t_one(), t_one()};
    }
    mine[TL_TAB] = a;
  }
  __syncthreads();
  const TAcc fin = xyzz28_add_quad_mem(buf, base + TL_ACC, base + TL_TAB);
  const int ok = fin.is_identity() ? 1 : 0;
  const int ok_other = __shfl_xor(ok, 4, 64);   // the proof's second relation: the next quad of the same wave
  if (in_range && j == 0 && sub == 0) verdict[p] = is_bad ? CPX_ERR_DESERIALIZE : (ok && ok_other) ? CPX_OK : CPX_ERR_VERIFY;
}

// ---- the grouped / fused check (tracker_check_plan.hpp) ----
// k_tracker_check_scalars: a work-group of TCS_THREADS lanes per group task of the plan, a lane per item (the group's items in strides of
// the work-group).  Item p of the group gets its five bases and Montgomery scalars at the plan's slots; a flagged item, and an identity
// point of a live one, is written as (generator, 0).  Every lane adds up the a s of its items in batch order, the lanes' sums are added
// in a fixed binary tree through LDS (Fr addition is exact: the tree only fixes the order of execution), lane 0 writes the generator term.
constexpr int TCS_THREADS = 256;
__global__ __launch_bounds__(TCS_THREADS) void k_tracker_check_scalars(const Aff* __restrict__ pts, const uint8_t* __restrict__ proofs, const Fr* __restrict__ chal,
                                                                       const uint8_t* __restrict__ bad, const Fr* __restrict__ weights, Aff gen, int count, int group,
                                                                       Aff* __restrict__ bases, Fr* __restrict__ scalars) {
  __shared__ Fr red[TCS_THREADS];
  const int t = threadIdx.x;
  const size_t cnt = (size_t)count, g = blockIdx.x, first = g * (size_t)group;
  const size_t n = first >= cnt ? 0 : (cnt - first < (size_t)group ? cnt - first : (size_t)group);   // LocatePlan::group_count
  const size_t off = g + TCK_TERMS * first;                                                           // TrackerCheckPlan::task_off
  Fr acc = Fr::zero();
  for (size_t i = t; i < n; i += TCS_THREADS) {
    const size_t p = first + i;
    const bool live = bad[p] == 0;
    TrackerCheckScalars sc{};
    if (live) {
      Fr s;
      (void)load_canonical_fr(proofs + 128 * p + 96, s);
      sc = tracker_check_scalars(weights[2 * p], weights[2 * p + 1], fe_to_mont(s), fe_to_mont(chal[p]));
      acc = fe_add(acc, sc.gen);
    }
    for (int j = 0; j < TCK_TERMS; j++) {
      const size_t slot = off + 1 + TCK_TERMS * i + (size_t)j;
      Aff P = gen;
      bool use = false;
      if (live) {
        const Aff Q = pts[(size_t)tck_plane(j) * cnt + p];
        if (!Q.is_identity()) {
          P = Q;
          use = true;
        }
      }
      bases[slot] = P;
      scalars[slot] = use ? sc.term[j] : Fr::zero();
    }
  }
  red[t] = acc;
  __syncthreads();
  for (int w = TCS_THREADS / 2; w > 0; w >>= 1) {
    if (t < w) red[t] = fe_add(red[t], red[t + w]);
    __syncthreads();
  }
  if (t == 0) {
    bases[off] = gen;
    scalars[off] = red[0];
  }
}

// k_tracker_gather: a lane per suspect
__global__ __launch_bounds__(64) void k_tracker_gather(const uint32_t* __restrict__ list, int n_suspects, int count, const Aff* __restrict__ pts,
                                                       const uint8_t* __restrict__ proofs, const Fr* __restrict__ chal, Aff* __restrict__ pts_out,
                                                       uint8_t* __restrict__ proofs_out, Fr* __restrict__ chal_out, uint8_t* __restrict__ bad_out) {
  const size_t s = (size_t)blockIdx.x * 64 + threadIdx.x, S = (size_t)n_suspects, cnt = (size_t)count;
  if (s >= S) return;
  const size_t p = list[s];
  if (p >= cnt) return;   // (never: the list holds items of the batch)
  for (int pl = 0; pl < TCK_TERMS; pl++) pts_out[(size_t)pl * S + s] = pts[(size_t)pl * cnt + p];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(proofs + 128 * p);   // (4-byte aligned: the proofs start at a multiple of 16)
  uint32_t* dst = reinterpret_cast<uint32_t*>(proofs_out + 128 * s);
  for (int w = 0; w < 32; w++) dst[w] = src[w];
  chal_out[s] = chal[p];
  bad_out[s] = 0;
}

#define TRK_LAUNCH(kern, grid, block, lds, stream, ...)                                            \
  do {                                                                                                \
    hipEvent_t _a = nullptr, _b = nullptr;                                                            \
    take_launch_events(&_a, &_b);                                                                     \
    if (_a || _b) hipExtLaunchKernelGGL(kern, grid, block, lds, stream, _a, _b, 0, __VA_ARGS__);      \
    else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);                             \
  } while (0)

void launch_tracker_challenge_verify(const uint8_t* d_in, const uint8_t* d_status, int count, Fr* d_chal, uint8_t* d_bad, hipStream_t s) {
  if (count <= 0) return;
  TRK_LAUNCH(k_tracker_challenge<false>, dim3(count), dim3(64), 0, s, d_in, (const uint8_t*)nullptr, d_status, (const Fr*)nullptr, (const Fr*)nullptr, count, d_chal,
             d_bad, (uint8_t*)nullptr, (int*)nullptr);
}
void launch_tracker_challenge_prove(const uint8_t* d_trackers, const uint8_t* d_comp, const uint8_t* d_status, const Fr* d_k, const Fr* d_blinder, int count,
                                    uint8_t* d_proofs_out, int* d_verdict, hipStream_t s) {
  if (count <= 0) return;
  TRK_LAUNCH(k_tracker_challenge<true>, dim3(count), dim3(64), 0, s, d_trackers, d_comp, d_status, d_k, d_blinder, count, (Fr*)nullptr, (uint8_t*)nullptr,
             d_proofs_out, d_verdict);
}
void launch_tracker_relations(const Aff* d_pts, const uint8_t* d_proofs, const Fr* d_chal, const uint8_t* d_bad, const Aff& gen, int count, int* d_verdict,
                              hipStream_t s) {
  if (count <= 0) return;
  const unsigned waves = (unsigned)((2L * count + 15) / 16);
  TRK_LAUNCH(k_tracker_relations, dim3(waves), dim3(64), TR_LDS, s, d_pts, d_proofs, d_chal, d_bad, gen, count, d_verdict);
}
void launch_tracker_check_scalars(const Aff* d_pts, const uint8_t* d_proofs, const Fr* d_chal, const uint8_t* d_bad, const Fr* d_weights, const Aff& gen, int count,
                                  int group, int ntasks, Aff* d_bases, Fr* d_scalars, hipStream_t s) {
  if (count <= 0 || ntasks <= 0) return;
  TRK_LAUNCH(k_tracker_check_scalars, dim3(ntasks), dim3(TCS_THREADS), 0, s, d_pts, d_proofs, d_chal, d_bad, d_weights, gen, count, group, d_bases, d_scalars);
}
void launch_tracker_gather(const uint32_t* d_list, int n_suspects, int count, const Aff* d_pts, const uint8_t* d_proofs, const Fr* d_chal, Aff* d_pts_out,
                           uint8_t* d_proofs_out, Fr* d_chal_out, uint8_t* d_bad_out, hipStream_t s) {
  if (n_suspects <= 0) return;
  TRK_LAUNCH(k_tracker_gather, dim3((n_suspects + 63) / 64), dim3(64), 0, s, d_list, n_suspects, count, d_pts, d_proofs, d_chal, d_pts_out, d_proofs_out, d_chal_out,
             d_bad_out);
}

}  // namespace cpx
