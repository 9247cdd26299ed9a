// gfx950 (MI355X / CDNA4) kernels for the Curdleproofs G1 hot path.
//
// Replaces, behind include/cpx.h, the arithmetic the reference reaches through
//   util::msm                       /root/reference/src/util.rs:19-22             -> k_to_table_endo + k_msm_tblw<2, true> + k_reduce_sets
//                                                                                    + k_msm_tail (fewer than 64 points: k_to_table + k_msm_accw)
//   the commitments and log-round cross terms of the prover (all MSMs over fixed bases in the batch engine)
//                                   inner_product_argument.rs:126-127,158-161,
//                                   same_multiscalar_argument.rs:80-82,107-112 ...  -> k_msm_fix (CRS), k_msm_tblw (per-proof tables), k_reduce_sets
//   IPA / SameMSM basis folds       inner_product_argument.rs:174-179,
//                                   same_multiscalar_argument.rs:126-131            -> k_smul (add operand set; tier 0)
//   G' rescale / shuffle scaling    grand_product_argument.rs:90-102, util.rs:94-95 -> k_smul (no add operand)
//   into_affine / normalize_batch + compressed serialisation                        -> k_finalize, k_finalize_ranges, k_compress
//   deserialize_compressed (Validate::Yes)                                          -> k_decompress
//   MsmAccumulator shared by many proofs (BASELINE config 5)                        -> k_msm_tblw<2, true> over groups of proofs
//
// Integer big-number work on the VALU; no MFMA — there is no dense contraction here.  Design notes:
//  * every group operation runs on the carry-free 28-bit-limb "table form" (fp28.hpp / g1_28.hpp);
//    points enter a kernel through t_from_std and leave through t_to_std / t_jac_to_std;
//  * MSM work-groups are single waves (no inter-wave barriers): lanes own buckets in registers and walk per-bucket
//    lists sorted into LDS (k_msm_tblw) or digit rows staged in LDS (k_msm_fix, k_msm_accw), points are gathered from
//    HBM/L2 tables; the lane accumulators are added up by separate work-efficient kernels (k_reduce_sets);
//  * scalars of the table kernels are split by the G1 endomorphism (glv.hpp): half the doublings in the table build;
//  * the long doubling chain that combines the windows of a bucket MSM is split out into k_msm_tail, one *lane* per
//    partial Horner evaluation, so that lanes stay busy across the many independent MSMs of a proof batch;
//  * Jacobian results are normalised with one inversion per work-group (LDS product scans + a division-step
//    inversion, modinv30.hpp) instead of the reference's one inversion per point.
#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <cctype>
#include <string>
#include <hip/hip_ext.h>
#include "g1.hpp"
#include "g1_28.hpp"
#include "g1_28_quad.hpp"
#include "quad_program.hpp"
#include "strobe.hpp"
#include "wave_strobe.hpp"
#include "lane_strobe.hpp"
#include "recode.hpp"
#include "glv.hpp"
#include "kernels.h"
#include "block_inverse.hpp"
#include "msm_body.hpp"
#include "round_algebra.hpp"
#include "tier0_plan.hpp"

namespace cpx {

// ------------------------------------------------------------------ MSM over arbitrary bases: bucket accumulation
// Pippenger with signed radix-16 windows for small caller-supplied MSMs (tier 0 below 64 points, the CRS sums of
// set_crs; larger one-off MSMs — the verifier's per-proof points, R and S — take k_msm_tblw<2, true>).  Two kernels:
//  k_to_table   converts every base of every task to the table form once (2 products per coordinate) into a
//               scratch array (task.conv_off); the 8 waves of a task then gather 112-B points from it (L2).
//  k_msm_accw   barrier-free single-wave groups as in k_msm_tblw: a wave owns 8 windows of one task, lane =
//               (window, bucket); the digit rows of the whole task (<= 1344 points per pass) sit in LDS, so lanes
//               only re-synchronise once per task and the slowest lane is decided over the whole task.  Windows
//               carry different weights here (no pre-shifted copies), so buckets cannot be shared across windows:
//               output = 64 window sums per task, folded by the Horner tails below.
// The previous one-group-per-task version (512 threads, LDS-staged points, 4 barriers per 256 points) spent 37 %
// of its wave-cycles waiting and, at one 86 KB group per CU, left no room for other kernels' waves to fill in.
constexpr int ACW_CHUNK = 1344;   // 8 digit rows of 1344 bytes = the 64 x 168 B the reduction needs anyway; one pass for the verifier's 1191-point tasks
constexpr int ACW_LDS = 64 * (int)sizeof(TJac) > 8 * ACW_CHUNK ? 64 * (int)sizeof(TJac) : 8 * ACW_CHUNK;

__global__ __launch_bounds__(64) void k_to_table(const MsmTask* __restrict__ tasks, TAff* __restrict__ conv) {
  const MsmTask task = tasks[blockIdx.y];
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  if (j >= task.n) return;
  conv[(size_t)task.conv_off + j] = t_from_std(task.bases[task.idx ? task.idx[j] : j]);
}

// bases of the endomorphism MSM (k_msm_tblw<2, true>): per task the table-form points followed by their images
// -phi(P) = (beta x, -y), and the table task describing them (two "copies", stride n; 32 partial sums from task * 32)
__global__ __launch_bounds__(64) void k_to_table_endo(const MsmTask* __restrict__ tasks, TAff* __restrict__ conv, uint32_t* __restrict__ digits,
                                                      TblTask* __restrict__ ttasks, int slices) {
  const MsmTask task = tasks[blockIdx.y];
  const uint32_t j = blockIdx.x * 64 + threadIdx.x;
  TAff* dst = conv + 2 * (size_t)task.conv_off;
  uint32_t* dgs = digits + 9 * (size_t)task.conv_off;
  if (j == 0) {
    TblTask t;
    t.seg[0] = TblSeg{dst, nullptr, task.n, task.n};
    t.seg[1] = TblSeg{nullptr, nullptr, 0, 0};
    t.scalars = task.scalars;
    t.flags = task.flags;
    t.pad = blockIdx.y * 32 * slices;
    t.digits = dgs;
    ttasks[blockIdx.y] = t;
  }
  if (j >= task.n) return;
  {   // the scalar's split and its 2 x 16 signed radix-256 digits, once for the 16 waves of the task
    Fr k = task.scalars[j];
    if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
    uint32_t t[4], q[4], bytes[8], nk, nt;
    glv_split(k.v, t, q, nk, nt);
    glv_biased_bytes(t, bytes);
    glv_biased_bytes(q, bytes + 4);
    CPX_UNROLL for (int w = 0; w < 8; w++) dgs[9 * (size_t)j + w] = bytes[w];
    dgs[9 * (size_t)j + 8] = (nk ^ nt) | (nk << 1);
  }
  const TAff P = t_from_std(task.bases[task.idx ? task.idx[j] : j]);
  dst[j] = P;
  dst[task.n + j] = P.is_identity() ? P : TAff{t_mul(P.x, t_beta()), t_neg(P.y)};
}

__global__ __launch_bounds__(64, 2) void k_msm_accw(const MsmTask* __restrict__ tasks, const TAff* __restrict__ conv, TJac* __restrict__ wsum) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  int8_t* digits = reinterpret_cast<int8_t*>(smem);   // [8][ACW_CHUNK]
  TJac* red = reinterpret_cast<TJac*>(smem);          // [64] (aliases the digits afterwards)
  const MsmTask task = tasks[blockIdx.x >> 3];
  const int w8 = blockIdx.x & 7;
  const int lane = threadIdx.x;
  const int wl = lane >> 3, mag = (lane & 7) + 1;
  const TAff* pts = conv + task.conv_off;
  TAcc xacc = TAcc::identity();

  for (uint32_t base = 0; base < task.n; base += ACW_CHUNK) {
    const int m = min((uint32_t)ACW_CHUNK, task.n - base);
    __syncthreads();
    for (int t = lane; t < m; t += 64) {
      Fr k = task.scalars[base + t];
      if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
      int8_t d[64];
      recode_signed16(k.v, d);
      CPX_UNROLL for (int j = 0; j < 8; j++) digits[j * ACW_CHUNK + t] = d[w8 * 8 + j];
    }
    __syncthreads();
    const int8_t* row = digits + wl * ACW_CHUNK;
    int i = 0;
    for (;;) {
      int d = 0;
      while (i < m) {   // cheap divergent scan to this lane's next matching point
        d = row[i];
        if (d == mag || d == -mag) break;
        i++;
      }
      const bool have = i < m;
      if (!__any(have)) break;
      if (have) {
        const TAff q = pts[base + i];
        xacc = t_acc_add_mixed(xacc, t_cneg(q, d < 0));
        i++;
      }
    }
  }
  TJac acc = t_acc_to_jac(xacc);
  __syncthreads();
  red[lane] = acc;
  __syncthreads();
  // Window sum  sum_{b=1..8} b * B_b  =  sum_b (suffix sum of B from b): a Hillis-Steele suffix scan over the
  // window's 8 lanes (3 steps) followed by a tree sum (3 steps).
  const int b = lane & 7;
  for (int sft = 1; sft < 8; sft <<= 1) {
    const bool has = b + sft < 8;
    TJac other;
    if (has) other = red[lane + sft];
    __syncthreads();
    if (has) {
      acc = t_add(acc, other);
      red[lane] = acc;
    }
    __syncthreads();
  }
  for (int sft = 4; sft >= 1; sft >>= 1) {
    const bool has = b < sft;
    TJac other;
    if (has) other = red[lane + sft];
    __syncthreads();
    if (has) {
      acc = t_add(acc, other);
      red[lane] = acc;
    }
    __syncthreads();
  }
  if (b == 0) wsum[(size_t)(blockIdx.x >> 3) * 64 + w8 * 8 + wl] = acc;
}

// ------------------------------------------------------------------ lane accumulators -> partial sums
// The MSM waves below do not reduce their 64 lane accumulators themselves: an in-wave reduction is a chain of 6-12
// DEPENDENT point additions during which most lanes idle (a quarter of k_msm_fix's time, a third of k_msm_tblw's at
// the 128-point tasks of the ell = 252 prover).  They store the raw accumulators ("sets" of 64 extended-Jacobian
// points, 224 B each) and k_reduce_sets adds them up with
// every lane busy: 8 threads per set sum 8 entries each (k_reduce_sets), one thread per set combines the 8 group
// results (k_reduce_groups).
//   plain    (k_msm_fix):  sum_l A_l
//   weighted (k_msm_tblw): lane l of set 2k + h holds bucket |d| = 64 h + l + 1  ->  sum_l (64 h + l + 1) A_l,
//            as running sums per group of 8 (W_g = sum_j (j+1) A_{8g+j}, S_g = sum_j A_{8g+j}) and once more over
//            the groups: sum_g W_g + 8 sum_g g S_g + 64 h sum_g S_g.

// Two launches so that no lane idles while a few finish: level 1 = thread per (set, group of 8 lanes), level 2 = thread
// per set over the 8 group results (mid: [set][8] x {S, W}).
// (Both levels stay in the accumulators' extended-Jacobian coordinates: a full XYZZ addition is 12M + 2S with Y3 under one
// reduction, 5110 multiply-adds, against 5817 for the Jacobian 11M + 5S plus two products per input for the conversion; only the
// partial sum a set ends in is converted.)
constexpr int MID_PER_SET = 16;   // TAcc entries of `mid` per set: 8 groups x {S, W}
// a lane's parked accumulator in LDS, word-interleaved by lane (word w of lane l at [w * 64 + l]: conflict-free)
__device__ __forceinline__ void lds_park(uint32_t* __restrict__ buf, int lane, const TAcc& a) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
  CPX_UNROLL for (int i = 0; i < ACC_WORDS; i++) buf[i * 64 + lane] = w[i];
}
__device__ __forceinline__ TAcc lds_unpark(const uint32_t* __restrict__ buf, int lane) {
  TAcc a;
  uint32_t* w = reinterpret_cast<uint32_t*>(&a);
  CPX_UNROLL for (int i = 0; i < ACC_WORDS; i++) w[i] = buf[i * 64 + lane];
  return a;
}
// Product body (fp28.hpp): Karatsuba with the Karatsuba reduction (the default) here and in k_reduce_groups; both spilled at 256
// VGPRs before it and keep their 176 scratch bytes, their spill counts (61 / 98) and two waves per SIMD
// (profiles/r07_f28_karatsuba.md, profiles/r08_f28_redc_karatsuba.md).
template <bool WEIGHTED> __global__ __launch_bounds__(64, 2) void k_reduce_sets(const uint32_t* __restrict__ raw, int nsets, TAcc* __restrict__ mid) {
  __shared__ uint32_t park[WEIGHTED ? ACC_WORDS * 64 : 1];
  const int t = blockIdx.x * 64 + threadIdx.x, lane = threadIdx.x;
  if (t >= nsets * 8) return;
  const int set = t >> 3, g = t & 7;
  const uint32_t* rs = raw + (size_t)set * RAW_SET_WORDS;
  // the weighted running sum W waits in LDS between its additions (two XYZZ sums live in registers beside the operands of an
  // addition are 300 VGPRs: one wave per SIMD instead of two; until round 3 it waited in its global output slot: a round trip
  // to HBM inside every step of the dependent chain)
  TAcc run = raw_load(rs, g * 8 + 7);
  if (WEIGHTED) lds_park(park, lane, run);
  for (int j = 6; j >= 0; j--) {
    run = t_acc_add(run, raw_load(rs, g * 8 + j));
    if (WEIGHTED) lds_park(park, lane, t_acc_add(lds_unpark(park, lane), run));
  }
  mid[(size_t)t * (WEIGHTED ? 2 : 1)] = run;
  if (WEIGHTED) mid[(size_t)t * 2 + 1] = lds_unpark(park, lane);
}
template <bool WEIGHTED> __global__ __launch_bounds__(64, 2) void k_reduce_groups(TAcc* __restrict__ mid, const uint32_t* __restrict__ slot, int nsets,
                                                                              TJac* __restrict__ part) {
  __shared__ uint32_t park[WEIGHTED ? ACC_WORDS * 64 : 1];
  const int set = blockIdx.x * 64 + threadIdx.x;
  if (set >= nsets) return;
  const TAcc* m = mid + (size_t)set * 8 * (WEIGHTED ? 2 : 1);
  if (!WEIGHTED) {
    TAcc run = m[7];
    for (int k = 6; k >= 0; k--) run = t_acc_add(run, m[k]);
    part[slot[set]] = t_acc_to_jac(run);
    return;
  }
  // (v waits in LDS while run is being updated: see k_reduce_sets)
  const int lane = threadIdx.x;
  TAcc run = m[2 * 7];                          // S_7
  lds_park(park, lane, run);
  for (int k = 6; k >= 1; k--) {
    run = t_acc_add(run, m[2 * k]);
    lds_park(park, lane, t_acc_add(lds_unpark(park, lane), run));
  }
  run = t_acc_add(run, m[0]);                   // run = sum_g S_g, parked = sum_g g S_g
  TAcc v = lds_unpark(park, lane);
  if (set & 1) {                                // upper half of the magnitudes: + 64 sum_g S_g, parked while v is finished
    for (int d = 0; d < 6; d++) run = t_acc_dbl(run);
    lds_park(park, lane, run);
  }
  for (int d = 0; d < 3; d++) v = t_acc_dbl(v); // 8 v
  for (int k = 0; k < 8; k++) v = t_acc_add(v, m[2 * k + 1]);
  if (set & 1) v = t_acc_add(v, lds_unpark(park, lane));
  part[slot[set]] = t_acc_to_jac(v);
}

__global__ __launch_bounds__(64) void k_reduce_sets_wave(const uint32_t* __restrict__ raw, const uint32_t* __restrict__ slot, int nplain, TJac* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);   // [QP_ENTRIES]
  const int set = blockIdx.x, lane = threadIdx.x;
  // sets [0, nplain) are plain (k_msm_fix), the rest bucket sets (k_msm_tblw), lower / upper half of the magnitudes alternating
  const QuadProgram& prog = c_quad_prog[set < nplain ? 0 : 1 + ((set - nplain) & 1)];
  buf[lane] = raw_load(raw + (size_t)set * RAW_SET_WORDS, lane);
  if (lane == 0) buf[QP_IDENT] = TAcc::identity();
  __syncthreads();
  quad_exec(buf, prog.nrounds, [&](int r, int quad, bool& dbl) {
    dbl = prog.dbl[r] != 0;
    return prog.job[r][quad];
  });
  if (lane == 0) part[slot[set]] = t_acc_to_jac(buf[prog.result]);
}

// Product body of the bucket loops below (k_msm_tblw, k_msm_tblw_pair, k_msm_fix): Karatsuba columns with the Karatsuba
// reduction, the default — 215–225 VGPRs, no scratch, two waves per SIMD; 2731 multiply-adds per addition against 3155 with the
// schoolbook reduction (profiles/r08_f28_redc_karatsuba.md).
template <int WPW, bool PERWIN = false> __global__ __launch_bounds__(64, 2) void k_msm_tblw(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw,
                                                                                            uint32_t* __restrict__ raw_slot, int slices) {
  msm_tblw_body<WPW, PERWIN>(tasks, raw, raw_slot, slices, blockIdx.x);
}

// Two-segment per-proof tables (kernels.h): a wave of 16 or 32 windows serves both weight classes (four raw sets), a narrower one lies
// inside one class.
template <int WPW> __global__ __launch_bounds__(64, 2) void k_msm_tblw2(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot,
                                                                        int slices) {
  msm_tblw_body<WPW, false, false, 2>(tasks, raw, raw_slot, slices, blockIdx.x);
}

__global__ __launch_bounds__(64, 2) void k_msm_tblw_pair(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot) {
  msm_tblw_body<2, true, true>(tasks, raw, raw_slot, 1, blockIdx.x);
}

template <int CB, int FIX_WPW> __global__ __launch_bounds__(64, 2) void k_msm_fix(const FixTask* __restrict__ tasks, const TFix* __restrict__ tab, int nc,
                                                                     uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot) {
  msm_fix_body<CB, FIX_WPW>(tasks, tab, nc, raw, raw_slot, blockIdx.x);
}
// A lone proof's phase: the fixed-base waves and the shifted-table waves of a phase do not depend on each other, and each of the two
// launches leaves most of the GPU empty (8 waves per fixed-base task, 16 per table task).  One launch for both: the first
// nfix_blocks work-groups run the fixed-base body, the rest the table body (39 + 95 us one after the other -> the longer of the two).
__global__ __launch_bounds__(64, 2) void k_msm_fix_tblw(const FixTask* __restrict__ ftasks, const TFix* __restrict__ tab, int nc, uint32_t* __restrict__ fraw,
                                                        uint32_t* __restrict__ fraw_slot, uint32_t nfix_blocks, const TblTask* __restrict__ ttasks,
                                                        uint32_t* __restrict__ traw, uint32_t* __restrict__ traw_slot, int slices) {
  if (blockIdx.x < nfix_blocks) msm_fix_body<16, 2>(ftasks, tab, nc, fraw, fraw_slot, blockIdx.x);
  else msm_tblw_body<2, false>(ttasks, traw, traw_slot, slices, blockIdx.x - nfix_blocks);
}

// Table of multiples from the shifted copies: thread per (window, base) walks m = 1..M with mixed additions and
// normalises `chunk` entries at a time (own Montgomery trick + one inversion per work-group).
// (segs > 1: the M multiples of a (window, base) are split over that many threads, each starting from seg * (M / segs) * S.)
template <int CB> __global__ __launch_bounds__(64) void k_fix_build(const TAff* __restrict__ shift, int nc, TFix* __restrict__ tab, TblTmp* __restrict__ tmp, int chunk,
                                                                    int segs) {
  constexpr int W = (256 + CB - 1) / CB;
  constexpr uint32_t M = 1u << (CB - 1);
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = g < W * nc * segs;
  const int seg = live ? g / (W * nc) : 0, wi = live ? g % (W * nc) : 0;
  const int w = wi / nc, i = wi % nc;
  const TAff S = live ? shift[(size_t)w * nc + i] : TAff::identity();
  const bool inf = S.is_identity();
  TblTmp* my = tmp + (size_t)g * chunk;
  const uint32_t per = M / (uint32_t)segs, first = (uint32_t)seg * per;
  TFix* out = tab + (size_t)w * M * nc + i;
  TJac acc = TJac::identity();
  if (live && !inf && first) {   // first * S by double-and-add
    for (int b = 31; b >= 0; b--) {
      acc = t_dbl(acc);
      if ((first >> b) & 1u) acc = t_add_mixed(acc, S);
    }
  }
  for (uint32_t m0 = first; m0 < first + per; m0 += chunk) {
    TF prod = t_one();
    if (live) {
      for (int j = 0; j < chunk; j++) {
        acc = t_add_mixed(acc, S);          // (m0 + j + 1) * S
        my[j].p = acc;
        my[j].pre = prod;
        if (!inf) prod = t_mul(prod, acc.z);
      }
    }
    TF inv = t_block_batch_inverse(prod, buf);
    if (live) {
      for (int j = chunk - 1; j >= 0; j--) {
        TAff a = TAff::identity();
        if (!inf) {
          const TJac p = my[j].p;
          const TF zinv = t_mul(inv, my[j].pre);
          inv = t_mul(inv, p.z);
          a = t_to_affine(p, zinv);
        }
        out[(size_t)(m0 + j) * nc].a = a;
      }
    }
  }
}

__device__ __noinline__ TJac t_dbl_n(TJac p, int n) {
#pragma unroll 1
  for (int s = 0; s < n; s++) p = t_dbl(p);
  return p;
}
// Thread per request: add its partial sums [first, first + count), normalise (one inversion per work-group),
// convert to the standard form, scatter the affine point and emit the 48-byte compressed encoding.
__global__ __launch_bounds__(64) void k_finalize_ranges(const TJac* __restrict__ part, const uint32_t* __restrict__ first, const uint32_t* __restrict__ count,
                                                         int n, Aff* __restrict__ out_aff, const uint32_t* __restrict__ dst_index, uint8_t* __restrict__ out_comp,
                                                         const uint32_t* __restrict__ addends, const uint32_t* __restrict__ comp_index) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  TJac p = TJac::identity();
  if (g < n) {
    const TJac* src = part + first[g];
    const uint32_t c = count[g] & 0xffffu, hi = count[g] >> 16;   // the first `hi` partial sums carry the weight 2^64 (two-segment tables, kernels.h)
    if (c) p = src[0];
    for (uint32_t j = 1; j < c; j++) {
      if (j == hi) p = t_dbl_n(p, 64);
      p = t_add(p, src[j]);
    }
    if (hi && hi == c) p = t_dbl_n(p, 64);
    if (addends) {   // up to three already-normalised points of out_aff (results of earlier phases) added with coefficient 1
      for (int j = 0; j < 3; j++) {
        const uint32_t a = addends[3 * g + j];
        if (a != ~0u) p = t_add_mixed(p, t_from_std(out_aff[a]));
      }
    }
  }
  const bool inf = p.is_identity();
  const TF zinv = t_block_batch_inverse(p.z, buf);
  if (g >= n) return;
  const Aff a = inf ? Aff::identity() : t_to_std(t_to_affine(p, zinv));
  if (out_aff) out_aff[dst_index ? dst_index[g] : g] = a;
  if (out_comp) aff_compress_store(a, out_comp + (size_t)(comp_index ? comp_index[g] : (uint32_t)g) * 48);
}

// Small grids (a few proofs in flight: latency matters, not throughput): one single-wave WORK-GROUP per request.  The quads of the
// wave add the request's partial sums in a tree (ceil(log2(count)) rounds of quad additions, 6 us each, instead of count additions
// of 18-20 us), lane 0 adds the affine addends, inverts Z and emits the point.  One wave per group on purpose: the four waves of a
// 256-thread group (the first version: four requests sharing one inversion) were often placed two or more to a SIMD — these
// 241-VGPR waves then time-share its VALU, and the tree ran 1x ... 2.8x slower from launch to launch (83 ... 229 us for the same
// 16 partials); single-wave groups spread over the CUs.
__global__ __launch_bounds__(64) void k_finalize_ranges_wave(const TJac* __restrict__ part, const uint32_t* __restrict__ first, const uint32_t* __restrict__ count,
                                                             int n, Aff* __restrict__ out_aff, const uint32_t* __restrict__ dst_index, uint8_t* __restrict__ out_comp,
                                                             const uint32_t* __restrict__ addends, const uint32_t* __restrict__ comp_index) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);   // [256]: up to 255 sums + the identity (entry 255) for idle quads
  const int lane = threadIdx.x, g = blockIdx.x;
  const TJac* src = part + first[g];
  const uint32_t c = count[g] & 0xffffu, hi = count[g] >> 16;   // the first `hi` partial sums carry the weight 2^64 (two-segment tables, kernels.h)
  int m = c < 255 ? (int)c : 255;
  for (int i = lane; i < m; i += 64) {
    TJac p = (uint32_t)i < hi ? t_dbl_n(src[i], 64) : src[i];   // (every lane shifts its own entry: the 64 doublings are paid once in time)
    for (uint32_t j = i + 255; j < c; j += 255) p = t_add(p, j < hi ? t_dbl_n(src[j], 64) : src[j]);   // (more partial sums than entries: never in the shipped configurations)
    buf[i] = xyzz28_from_jac(p);
  }
  if (lane == 0) {
    buf[255] = TAcc::identity();
    if (m == 0) buf[0] = TAcc::identity();
  }
  __syncthreads();
  // level by level: live entries [0, m); top = the largest power of two below m; entries [top, m) fold onto [0, m - top)
  int nrounds = 0;
  for (int mm = m; mm > 1;) {
    int top = 1;
    while (top * 2 < mm) top *= 2;
    nrounds += (mm - top + 15) / 16;
    mm = top;
  }
  int top = 1, done = 0;
  if (m > 1) while (top * 2 < m) top *= 2;
  quad_exec(buf, nrounds, [&](int, int quad, bool&) {
    const int j = done + quad, njobs = m - top;
    const QuadJob jb = j < njobs ? QuadJob{(uint8_t)j, (uint8_t)(j + top), (uint8_t)j, 1} : QuadJob{255, 255, 255, 0};
    done += 16;
    if (done >= njobs) {   // next level
      m = top;
      top = top > 1 ? top / 2 : 1;
      done = 0;
    }
    return jb;
  });
  if (lane != 0) return;
  TJac p = t_acc_to_jac(buf[0]);
  if (addends) {
    for (int j = 0; j < 3; j++) {
      const uint32_t a = addends[3 * g + j];
      if (a != ~0u) p = t_add_mixed(p, t_from_std(out_aff[a]));
    }
  }
  const bool inf = p.is_identity();
  const TF zinv = inf ? t_one() : t_inv_device(p.z);
  const Aff a = inf ? Aff::identity() : t_to_std(t_to_affine(p, zinv));
  if (out_aff) out_aff[dst_index ? dst_index[g] : g] = a;
  if (out_comp) aff_compress_store(a, out_comp + (size_t)(comp_index ? comp_index[g] : (uint32_t)g) * 48);
}

// ------------------------------------------------------------------ table construction
// Scratch of the build kernels in structure-of-arrays form: word k of entry c of thread g lives at
// ((c * TMP_WORDS + k) * nthreads + g), so the 64 lanes of a wave store / load 256 contiguous bytes per
// instruction (the array-of-structs layout wrote 4 bytes per 14 KB stride: 3.5x write amplification in HBM).
constexpr int TF_WORDS = (int)(sizeof(TF) / 4), TMP_WORDS = 4 * TF_WORDS;
__device__ __forceinline__ void tmp_store_f(uint32_t* b, size_t stride, const TF& a) {
  CPX_UNROLL for (int i = 0; i < TF_WORDS; i++) b[(size_t)i * stride] = (uint32_t)a.v[i];
}
__device__ __forceinline__ void tmp_load_f(const uint32_t* b, size_t stride, TF& a) {
  CPX_UNROLL for (int i = 0; i < TF_WORDS; i++) a.v[i] = (decltype(a.v[0] + 0))b[(size_t)i * stride];
}
__device__ __forceinline__ void tmp_store(uint32_t* tmp, size_t nthreads, size_t g, int c, const TJac& p, const TF& pre) {
  uint32_t* b = tmp + (size_t)c * TMP_WORDS * nthreads + g;
  tmp_store_f(b, nthreads, p.x);
  tmp_store_f(b + (size_t)TF_WORDS * nthreads, nthreads, p.y);
  tmp_store_f(b + (size_t)2 * TF_WORDS * nthreads, nthreads, p.z);
  tmp_store_f(b + (size_t)3 * TF_WORDS * nthreads, nthreads, pre);
}
__device__ __forceinline__ void tmp_load(const uint32_t* tmp, size_t nthreads, size_t g, int c, TJac& p, TF& pre) {
  const uint32_t* b = tmp + (size_t)c * TMP_WORDS * nthreads + g;
  tmp_load_f(b, nthreads, p.x);
  tmp_load_f(b + (size_t)TF_WORDS * nthreads, nthreads, p.y);
  tmp_load_f(b + (size_t)2 * TF_WORDS * nthreads, nthreads, p.z);
  tmp_load_f(b + (size_t)3 * TF_WORDS * nthreads, nthreads, pre);
}

// Thread per base point: reads the standard-form source point, writes copy 0 in table form, then runs a chain
// of (real - 1) sb doublings storing every sb-th value (real = shifted copies: 16 for a 32-copy endomorphism row, 120 doublings; 8
// for a two-segment per-proof row, 56 doublings, sb passed as step_bits = 8); the real - 1 Jacobian copies are normalised with the
// thread's own Montgomery trick plus one inversion per work-group.
// Product body: Karatsuba through the out-of-line f28_mul / f28_sqr (its 56 or 120 doublings per base), Karatsuba reduction included;
// resources unchanged (profiles/r08_f28_redc_karatsuba.md).
__global__ __launch_bounds__(64) void k_table_build(const Aff* __restrict__ src, size_t src_row_stride, TAff* __restrict__ table, int rows, size_t row_stride,
                                                     int npts, int copy_stride, int copies, int endo, TblTmp* __restrict__ tmp_, int step_bits) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);
  uint32_t* tmp = reinterpret_cast<uint32_t*>(tmp_);
  const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long total = (long)rows * npts;
  const bool live = g < total;
  // endo: the row holds copies / 2 shifted copies 2^(8c) P followed by their images -phi(.) = (beta x, -y) (glv.hpp)
  const int real = endo ? copies / 2 : copies;
  const int sb = step_bits > 0 ? step_bits : (endo ? 128 : 256) / real;
  const TF beta = t_beta();
  TAff* col = nullptr;
  TF prod = t_one();
  bool inf = true;
  if (live) {
    // point-major thread order: the lanes of a wave hold the same column of different rows (proofs), so the
    // identity columns of the instance tables (blinder slots, curdleproofs.rs:141-155) retire whole waves at once
    const long r = g % rows, i = g / rows;
    col = table + r * row_stride + i;
    const TAff P = t_from_std(src[r * src_row_stride + i]);
    col[0] = P;
    inf = P.is_identity();
    if (endo) col[(size_t)real * copy_stride] = inf ? P : TAff{t_mul(P.x, beta), t_neg(P.y)};
    if (!inf) {
      TJac acc = TJac::from_affine(P);
      for (int c = 1; c < real; c++) {
        for (int s = 0; s < sb; s++) acc = t_dbl(acc);
        tmp_store(tmp, (size_t)total, (size_t)g, c - 1, acc, prod);   // prod = z_1 ... z_{c-1}
        prod = t_mul(prod, acc.z);
      }
    }
  }
  TF inv = t_block_batch_inverse(prod, buf);   // 1 / (z_1 ... z_{C-1})
  if (!live) return;
  for (int c = real - 1; c >= 1; c--) {
    TAff a = TAff::identity();
    if (!inf) {
      TJac p;
      TF pre;
      tmp_load(tmp, (size_t)total, (size_t)g, c - 1, p, pre);
      const TF zinv = t_mul(inv, pre);   // inv = 1/(z_1..z_c)
      inv = t_mul(inv, p.z);
      a = t_to_affine(p, zinv);
    }
    col[(size_t)c * copy_stride] = a;
    if (endo) col[(size_t)(real + c) * copy_stride] = inf ? a : TAff{t_mul(a.x, beta), t_neg(a.y)};
  }
}

// A few rows (a lone proof): one QUAD per base point.  The chain of doublings is what the build waits for (120 of them for the
// 16 + 16 copies of an endomorphism row, 56 for the 8 + 8 of a two-segment one): three product rounds per doubling over the quad instead of seven products of one lane;
// the copies are dealt to the four lanes, which normalise their four each (the work-group's one inversion as before).  The copies
// wait in LDS instead of the scratch buffer.
constexpr int TBQ_CHUNK = 4;   // copies per lane: real - 1 <= 16
__global__ __launch_bounds__(64) void k_table_build_quad(const Aff* __restrict__ src, size_t src_row_stride, TAff* __restrict__ table, int rows, size_t row_stride,
                                                          int npts, int copy_stride, int copies, int endo, int step_bits) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TF* buf = reinterpret_cast<TF*>(smem);                         // [2 * 64] batch inversion
  TF* pre_s = buf + 2 * 64;                                      // [TBQ_CHUNK][64]
  TJac* cp_s = reinterpret_cast<TJac*>(pre_s + TBQ_CHUNK * 64);  // [TBQ_CHUNK][64]
  const int tid = threadIdx.x, sub = tid & 3;
  const long g = (long)blockIdx.x * 16 + (tid >> 2);
  const long total = (long)rows * npts;
  const bool live = g < total;
  const int real = endo ? copies / 2 : copies;
  const int sb = step_bits > 0 ? step_bits : (endo ? 128 : 256) / real;
  const TF beta = t_beta();
  TAff* col = nullptr;
  TAff P = TAff::identity();
  if (live) {
    const long r = g % rows, i = g / rows;
    col = table + r * row_stride + i;
    P = t_from_std(src[r * src_row_stride + i]);
  }
  const bool inf = P.is_identity();
  if (live && sub == 0) {
    col[0] = P;
    if (endo) col[(size_t)real * copy_stride] = inf ? P : TAff{t_mul(P.x, beta), t_neg(P.y)};
  }
  TF prod = t_one();
  TJac acc = TJac::from_affine(P);   // (the identity doubles to the identity: idle quads just run along)
  int mine = 0;
  for (int c = 1; c < real; c++) {
    for (int s = 0; s < sb; s++) acc = jac28_dbl_quad(acc);
    if (((c - 1) & 3) == sub) {      // copy c belongs to lane (c - 1) mod 4
      cp_s[mine * 64 + tid] = acc;
      pre_s[mine * 64 + tid] = prod;
      if (!inf) prod = t_mul(prod, acc.z);
      mine++;
    }
  }
  TF inv = t_block_batch_inverse(prod, buf);
  if (!live) return;
  for (int k = mine - 1; k >= 0; k--) {
    const int c = 4 * k + sub + 1;
    TAff a = TAff::identity();
    if (!inf) {
      const TJac p = cp_s[k * 64 + tid];
      const TF zinv = t_mul(inv, pre_s[k * 64 + tid]);
      inv = t_mul(inv, p.z);
      a = t_to_affine(p, zinv);
    }
    col[(size_t)c * copy_stride] = a;
    if (endo) col[(size_t)(real + c) * copy_stride] = inf ? a : TAff{t_mul(a.x, beta), t_neg(a.y)};
  }
}

// ------------------------------------------------------------------ MSM: Horner tails
// out[t] = sum_{j < group} 2^(shift*j) in[t*group + j], one lane per output; the last stage hands the result
// over in the standard form.
template <bool STD_OUT> __global__ __launch_bounds__(64) void k_msm_tail(const TJac* __restrict__ in, TJac* __restrict__ out, Jac* __restrict__ out_std, int nout,
                                                                         int group, int shift, const TJac* __restrict__ extra, int extra_per_out, int dup) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nout) return;
  const TJac* src = in + (size_t)t * group * dup;   // `dup` consecutive inputs share a weight
  TJac acc = src[(group - 1) * dup];
  for (int d = 1; d < dup; d++) acc = t_add(acc, src[(group - 1) * dup + d]);
  for (int j = group - 2; j >= 0; j--) {
    for (int s = 0; s < shift; s++) acc = t_dbl(acc);
    for (int d = 0; d < dup; d++) acc = t_add(acc, src[j * dup + d]);
  }
  for (int j = 0; j < extra_per_out; j++) acc = t_add(acc, extra[(size_t)t * extra_per_out + j]);   // e.g. fixed-base partial sums
  if (STD_OUT) out_std[t] = t_jac_to_std(acc);
  else out[t] = acc;
}

// A few outputs (a lone proof's verification, tier-0 MSMs, R and S of a lone prover): one wave per output and one QUAD per window.
// The `dup` inputs of a window are added in a tree, quad j then shifts the sum of window j by shift * j doublings — the doublings
// of the 16 windows run side by side instead of one after the other in a Horner chain, each spread over the four lanes
// (g1_28_quad.hpp: 4.4 us instead of 7.6 us) — and the window sums and the extra partial sums are added in a tree of quad
// additions: shift * (group - 1) doublings and ~6 additions deep (0.6 ms for the verifier's 16 x 2 + 8 partial sums; the one-lane
// Horner chain took 1.6 ms).  Needs group <= 16, dup a power of two, extra_per_out <= 64 and group * dup + extra_per_out <= 255.
template <bool STD_OUT> __global__ __launch_bounds__(64) void k_msm_tail_wave(const TJac* __restrict__ in, TJac* __restrict__ out, Jac* __restrict__ out_std,
                                                                              int group, int shift, const TJac* __restrict__ extra, int extra_per_out, int dup) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);   // [nin + extra + 1]: the inputs, then the window sums and extras; the last = identity
  const int t = blockIdx.x, lane = threadIdx.x, quad = lane >> 2, sub = lane & 3;
  const int nin = group * dup, nall = nin + extra_per_out;
  const uint8_t ident = (uint8_t)nall;
  for (int i = lane; i < nall; i += 64) buf[i] = xyzz28_from_jac(i < nin ? in[(size_t)t * nin + i] : extra[(size_t)t * extra_per_out + (i - nin)]);
  if (lane == 0) buf[nall] = TAcc::identity();
  __syncthreads();
  {   // the inputs of a window: halving tree, level h adds entry i + h to entry i (i < h) of every window
    int nrounds = 0;
    for (int h = dup / 2; h >= 1; h >>= 1) nrounds += (group * h + 15) / 16;
    int h = dup / 2, done = 0;
    quad_exec(buf, nrounds, [&](int, int q, bool&) {
      const int j = done + q, njobs = group * h;
      const int w = j / h, i = j % h;
      const QuadJob jb = j < njobs ? QuadJob{(uint8_t)(w * dup + i), (uint8_t)(w * dup + i + h), (uint8_t)(w * dup + i), 1} : QuadJob{ident, ident, ident, 0};
      done += 16;
      if (done >= njobs) {
        h >>= 1;
        done = 0;
      }
      return jb;
    });
  }
  TAcc acc = buf[quad < group ? quad * dup : nall];
  TAcc ex = buf[nall];
  if (lane < extra_per_out) ex = buf[nin + lane];
  const int nd = shift * (group - 1), mine = quad < group ? shift * quad : 0;
  for (int s = 0; s < nd; s++) {
    const TAcc d = xyzz28_dbl_quad(acc);
    if (s < mine) acc = d;
  }
  __syncthreads();                              // every quad holds its window sum: the inputs may go
  if (quad < group && sub == 0) buf[quad] = acc;
  if (lane < extra_per_out) buf[group + lane] = ex;
  if (lane == 0) buf[group + extra_per_out] = TAcc::identity();
  __syncthreads();
  const uint8_t ident2 = (uint8_t)(group + extra_per_out);
  int m = group + extra_per_out, nrounds = 0;
  for (int mm = m; mm > 1;) {
    int top = 1;
    while (top * 2 < mm) top *= 2;
    nrounds += (mm - top + 15) / 16;
    mm = top;
  }
  int top = 1, done = 0;
  while (top * 2 < m) top *= 2;
  quad_exec(buf, nrounds, [&](int, int q, bool&) {
    const int j = done + q, njobs = m - top;
    const QuadJob jb = j < njobs ? QuadJob{(uint8_t)j, (uint8_t)(j + top), (uint8_t)j, 1} : QuadJob{ident2, ident2, ident2, 0};
    done += 16;
    if (done >= njobs) {   // next level
      m = top;
      top = top > 1 ? top / 2 : 1;
      done = 0;
    }
    return jb;
  });
  if (lane != 0) return;
  const TJac res = t_acc_to_jac(buf[0]);
  if (STD_OUT) out_std[t] = t_jac_to_std(res);
  else out[t] = res;
}

// ------------------------------------------------------------------ normalise + compress
// Thread per point: Jacobian -> affine (one inversion per work-group) and, optionally, the 48-byte
// compressed encoding the transcript and the proof bytes need.
__global__ __launch_bounds__(64) void k_finalize(const Jac* __restrict__ in, int n, Aff* __restrict__ out_aff, const uint32_t* __restrict__ dst_index,
                                                   uint8_t* __restrict__ out_comp, const uint32_t* __restrict__ addend_index) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  Fp* buf = reinterpret_cast<Fp*>(smem);
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  Jac p = Jac::identity();
  if (g < n) p = in[g];
  if (addend_index && g < n && addend_index[g] != ~0u)   // + an already-normalised point of out_aff (a result of an earlier phase)
    p = t_jac_to_std(t_add_mixed(t_jac_from_std(p), t_from_std(out_aff[addend_index[g]])));
  const bool inf = p.is_identity();
  Fp zinv = block_batch_inverse(p.z, buf);
  if (g >= n) return;
  Aff a = inf ? Aff::identity() : jac_to_affine_with_zinv(p, zinv);
  if (out_aff) out_aff[dst_index ? dst_index[g] : g] = a;
  if (out_comp) aff_compress_store(a, out_comp + (size_t)g * 48);
}
__global__ __launch_bounds__(256) void k_compress(const Aff* __restrict__ in, int n, int stride, uint8_t* __restrict__ out, int out_stride) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const size_t row = blockIdx.y;
  aff_compress_store(in[row * stride + g], out + (row * out_stride + g) * 48);
}

// selected columns of strided rows: out[(row * out_stride + cols[t]) * 48] = compress(in[row * stride + cols[t]]), t < ncols
__global__ __launch_bounds__(64) void k_compress_cols(const Aff* __restrict__ in, const uint32_t* __restrict__ cols, int ncols, int stride, uint8_t* __restrict__ out,
                                                      int out_stride) {
  const size_t row = blockIdx.x;
  for (int t = threadIdx.x; t < ncols; t += 64) aff_compress_store(in[row * stride + cols[t]], out + (row * out_stride + cols[t]) * 48);
}

// ------------------------------------------------------------------ per-element scalar-mul (+ add)
// Element e of task t:  out[e] = affine( (add ? add[e] : 0) + s * mul[e] ),
//   s = scalars[e * scalar_stride]  (stride 0: one scalar for the whole task = a fold).
// All tasks of a launch have `cnt` elements; consecutive threads take consecutive elements so the
// 96-byte point loads/stores of a wave are contiguous.
// The arithmetic runs on the table form: the two input points are converted on load (2 products per coordinate)
// and the result is converted back after the in-group batch inversion.  The scalar is split by the endomorphism (recode.hpp
// recode_smul_glv): a chain of 129 doublings with the non-adjacent forms of both halves instead of 257.
constexpr int SMUL_THREADS = 64;   // single-wave groups: no whole-CU placement constraint beside the MSM waves of other contexts

// EXCL (launches of at most 16 waves: the T_2 commitments of a small batch on the side stream): the wave claims the whole register file
// of its SIMD — the 215-operation chain is not slowed by a neighbour and, more to the point, does not slow the waves of the main
// stream's phase kernels that would otherwise share its SIMD for 3 ms (the slowest wave is the kernel: 605 instead of 302 us per
// k_msm_fix of the first IPA rounds at 128 proofs).
// (The claim rests on gfx950's unified 512-entry VGPR file — 256 architectural + 256 accumulation registers per lane — and on the compiler
// sizing a wave's allocation by the highest register a clobber names: checked for this target only.)
template <bool EXCL>
__global__ __launch_bounds__(SMUL_THREADS) void k_smul(const SmulTask* __restrict__ tasks, int ntasks, int cnt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#if defined(__gfx950__)
  if (EXCL) {
    asm volatile("v_mov_b32 v255, 0" ::: "v255");
    asm volatile("v_accvgpr_write_b32 a255, 0" ::: "a255");
  }
#elif defined(__HIP_DEVICE_COMPILE__)
  static_assert(!EXCL, "the exclusive-SIMD form is written for gfx950's register file");
#endif
  TF* buf = reinterpret_cast<TF*>(smem);                                             // 2 * SMUL_THREADS field elements
  uint32_t* naf = reinterpret_cast<uint32_t*>(smem + 2 * SMUL_THREADS * sizeof(TF));  // [20][SMUL_THREADS]: nz / ng words of both halves
  const int tid = threadIdx.x;
  const long g = (long)blockIdx.x * blockDim.x + tid;
  const long total = (long)ntasks * cnt;
  const bool live = g < total;
  TJac acc = TJac::identity();
  Aff* dst = nullptr;
  if (live) {
    const int t = (int)(g / cnt), e = (int)(g % cnt);
    const SmulTask task = tasks[t];
    dst = task.out + e;
    Fr k = task.scalars[(size_t)e * task.scalar_stride];
    if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
    // SMUL_PLAIN: the non-adjacent form of the whole scalar (rows 0..8 non-zero bits, 9..17 signs) — valid on all of E(Fp); otherwise the
    // endomorphism split, valid on the order-r subgroup (rows 0..4 / 5..9: t, rows 10..14 / 15..19: q)
    const bool plain = (task.flags & SMUL_PLAIN) != 0;
    if (plain) {
      uint32_t nz[9], ng[9];
      recode_naf(k.v, nz, ng);
      CPX_UNROLL for (int i = 0; i < 9; i++) {
        naf[i * SMUL_THREADS + tid] = nz[i];
        naf[(9 + i) * SMUL_THREADS + tid] = ng[i];
      }
    } else {
      SmulNaf rn;
      recode_smul_glv(k.v, rn);
      CPX_UNROLL for (int hh = 0; hh < 2; hh++)
        CPX_UNROLL for (int i = 0; i < 5; i++) {
          naf[(10 * hh + i) * SMUL_THREADS + tid] = rn.nz[hh][i];
          naf[(10 * hh + 5 + i) * SMUL_THREADS + tid] = rn.ng[hh][i];
        }
    }
    const TAff P = t_from_std(task.mul[e]);
    const TAff NP = P.is_identity() ? P : TAff{t_mul(P.x, t_beta()), t_neg(P.y)};   // N P = -phi(P) (glv.hpp)
    for (int i = plain ? 256 : 128; i >= 0; i--) {
      acc = t_dbl(acc);
      const int wd = i >> 5, bt = i & 31;
      if (plain) {
        if ((naf[wd * SMUL_THREADS + tid] >> bt) & 1u) acc = t_add_mixed(acc, t_cneg(P, (naf[(9 + wd) * SMUL_THREADS + tid] >> bt) & 1u));
        continue;
      }
      if ((naf[wd * SMUL_THREADS + tid] >> bt) & 1u) acc = t_add_mixed(acc, t_cneg(P, (naf[(5 + wd) * SMUL_THREADS + tid] >> bt) & 1u));
      if ((naf[(10 + wd) * SMUL_THREADS + tid] >> bt) & 1u) acc = t_add_mixed(acc, t_cneg(NP, (naf[(15 + wd) * SMUL_THREADS + tid] >> bt) & 1u));
    }
    if (task.add) acc = t_add_mixed(acc, t_from_std(task.add[e]));
  }
  const bool inf = acc.is_identity();
  const TF zinv = t_block_batch_inverse(acc.z, buf);
  if (!live) return;
  *dst = inf ? Aff::identity() : t_to_std(t_to_affine(acc, zinv));
}

// The same per-element computation with a QUAD per element (g1_28_quad.hpp) — the T_2 commitments of a small batch on the side stream
// (curdleproofs.rs:115-116, same_scalar_argument.rs:60-61): the one-lane form is a chain of 129 doublings + ~86 additions, 4.6 ms during which
// its waves sit beside the log rounds of the main stream; four lanes per element finish a doubling in 4.4 us and an addition in 6.1 us, and the
// two digit streams of the endomorphism split share ONE addition per step from the table {P, N P, P + N P, P - N P} and their negatives.
// Per step all quads of the wave double, then all add (the identity where both digits are zero): uniform control flow, operands in LDS.
constexpr int SQ_ACC = 0, SQ_TAB = 1, SQ_PER_QUAD = 9;   // per quad: the accumulator, +-P, +-NP, +-(P + NP), +-(P - NP)
constexpr int SQ_IDENT = 16 * SQ_PER_QUAD;
constexpr size_t SQ_LDS = (size_t)(SQ_IDENT + 1) * sizeof(TAcc) + 2 * 64 * sizeof(TF);
__global__ __launch_bounds__(64) void k_smul_quad(const SmulTask* __restrict__ tasks, int ntasks, int cnt) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);
  TF* inv_buf = reinterpret_cast<TF*>(smem + (size_t)(SQ_IDENT + 1) * sizeof(TAcc));
  const int lane = threadIdx.x, quad = lane >> 2, sub = lane & 3;
  const long g = (long)blockIdx.x * 16 + quad, total = (long)ntasks * cnt;
  const bool live = g < total;
  TAcc* mine = buf + quad * SQ_PER_QUAD;
  SmulNaf rn{};
  Aff* dst = nullptr;
  bool has_add = false;
  if (live) {
    const int t = (int)(g / cnt), e = (int)(g % cnt);
    const SmulTask task = tasks[t];
    dst = task.out + e;
    Fr k = task.scalars[(size_t)e * task.scalar_stride];
    if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
    recode_smul_glv(k.v, rn);   // (replicated over the quad: the four lanes take identical branches)
    if (sub == 0) {
      const TAff P = t_from_std(task.mul[e]);
      const bool inf = P.is_identity();
      const TAcc XP = inf ? TAcc::identity() : TAcc{P.x, P.y, t_one(), t_one()};
      const TAcc XN = inf ? TAcc::identity() : TAcc{t_mul(P.x, t_beta()), t_neg(P.y), t_one(), t_one()};   // N P = -phi(P) (glv.hpp)
      mine[SQ_ACC] = TAcc::identity();
      mine[SQ_TAB + 0] = XP;
      mine[SQ_TAB + 2] = XN;
    }
    has_add = task.add != nullptr;
  } else if (sub == 0) {
    mine[SQ_ACC] = mine[SQ_TAB + 0] = mine[SQ_TAB + 2] = TAcc::identity();
  }
  if (lane == 0) buf[SQ_IDENT] = TAcc::identity();
  __syncthreads();
  auto neg_of = [](const TAcc& a) { return a.is_identity() ? a : TAcc{a.x, t_neg(a.y), a.zz, a.zzz}; };
  {   // P + N P, then P - N P and the four negatives
    const TAcc sum = xyzz28_add_quad_mem(buf, quad * SQ_PER_QUAD + SQ_TAB + 0, quad * SQ_PER_QUAD + SQ_TAB + 2);
    if (sub == 0) {
      mine[SQ_TAB + 4] = sum;
      mine[SQ_TAB + 1] = neg_of(mine[SQ_TAB + 0]);
      mine[SQ_TAB + 3] = neg_of(mine[SQ_TAB + 2]);
    }
    __syncthreads();
    const TAcc dif = xyzz28_add_quad_mem(buf, quad * SQ_PER_QUAD + SQ_TAB + 0, quad * SQ_PER_QUAD + SQ_TAB + 3);
    if (sub == 0) {
      mine[SQ_TAB + 6] = dif;
      mine[SQ_TAB + 5] = neg_of(sum);
      mine[SQ_TAB + 7] = neg_of(dif);
    }
    __syncthreads();
  }
  for (int i = 128; i >= 0; i--) {
    const TAcc dbl = xyzz28_dbl_quad(buf[quad * SQ_PER_QUAD + SQ_ACC]);
    if (sub == 0) mine[SQ_ACC] = dbl;
    __syncthreads();
    const int wd = i >> 5, bt = i & 31;
    const int dt = ((rn.nz[0][wd] >> bt) & 1u) ? (((rn.ng[0][wd] >> bt) & 1u) ? -1 : 1) : 0;
    const int dq = ((rn.nz[1][wd] >> bt) & 1u) ? (((rn.ng[1][wd] >> bt) & 1u) ? -1 : 1) : 0;
    // table entry of dt P + dq N P: +P 0, -P 1, +NP 2, -NP 3, +(P+NP) 4, -(P+NP) 5, +(P-NP) 6, -(P-NP) 7
    int e = -1;
    if (dt && !dq) e = dt > 0 ? 0 : 1;
    else if (!dt && dq) e = dq > 0 ? 2 : 3;
    else if (dt && dq) e = dt == dq ? (dt > 0 ? 4 : 5) : (dt > 0 ? 6 : 7);
    if (!__any(e >= 0)) continue;   // (uniform: no quad of the wave adds in this step)
    const TAcc sum = xyzz28_add_quad_mem(buf, quad * SQ_PER_QUAD + SQ_ACC, e >= 0 ? quad * SQ_PER_QUAD + SQ_TAB + e : SQ_IDENT);
    if (sub == 0) mine[SQ_ACC] = sum;
    __syncthreads();
  }
  if (__any(has_add)) {   // + the affine addend (r H of a T_2 commitment)
    if (sub == 0) {
      TAcc a = TAcc::identity();
      if (live && has_add) {
        const int t = (int)(g / cnt), e = (int)(g % cnt);
        const TAff A = t_from_std(tasks[t].add[e]);
        if (!A.is_identity()) a = TAcc{A.x, A.y, t_one(), t_one()};
      }
      mine[SQ_TAB + 0] = a;
    }
    __syncthreads();
    const TAcc sum = xyzz28_add_quad_mem(buf, quad * SQ_PER_QUAD + SQ_ACC, quad * SQ_PER_QUAD + SQ_TAB + 0);
    if (sub == 0) mine[SQ_ACC] = sum;
    __syncthreads();
  }
  // one inversion per wave; lane 0 of every quad writes its element
  TJac pt = TJac::identity();
  if (sub == 0) pt = t_acc_to_jac(mine[SQ_ACC]);
  const bool inf = pt.is_identity();
  const TF zinv = t_block_batch_inverse(pt.z, inv_buf);
  if (live && sub == 0) *dst = inf ? Aff::identity() : t_to_std(t_to_affine(pt, zinv));
}

// ------------------------------------------------------------------ decompression (+ subgroup check)
// ark-bls12-381 `deserialize_compressed` (Validate::Yes) for tracker / proof ingestion
// (/root/reference/src/whisk.rs:265-277, :318-320; curdleproofs.rs:312-323): y = sqrt(x^3 + 4) by
// a^((p+1)/4), sign chosen by the flag bit, then r * P == O.
// All field work runs on the table form (fp28.hpp); the subgroup test is the endomorphism test of g1_28.hpp.
__device__ __noinline__ F28 f28_sqrt_device(const F28& a) { return f28_sqrt_candidate(a); }
__device__ __noinline__ bool g1_in_subgroup_device(const Aff28& P) { return g1_28_in_subgroup(P); }

// Product body: Karatsuba (reduction included) through the out-of-line f28_mul / f28_sqr; the kernel keeps its 336 scratch bytes,
// 37 spilled VGPRs and two waves per SIMD.
__global__ __launch_bounds__(64, 2) void k_decompress(const uint8_t* __restrict__ in, int n, Aff* __restrict__ out,
                                                   const uint32_t* __restrict__ dst_index, uint8_t* __restrict__ status, int check_subgroup,
                                                   const uint32_t* __restrict__ src_offset) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n) return;
  const uint8_t* b = in + (src_offset ? (size_t)src_offset[g] : (size_t)g * 48);   // dense encodings, or byte offsets into serialized proofs
  Fp xc;
  if ((reinterpret_cast<uintptr_t>(b) & 15) == 0) {   // 16-byte aligned (device-resident proofs / dense arrays): three 16-byte loads
    const uint4* q = reinterpret_cast<const uint4*>(b);
    const uint4 q0 = q[0], q1 = q[1], q2 = q[2];
    const uint32_t ww[12] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w};
    CPX_UNROLL for (int l = 0; l < 12; l++) xc.v[11 - l] = bswap32(ww[l]);
  } else {
    for (int l = 0; l < 12; l++) xc.v[11 - l] = ((uint32_t)b[4 * l] << 24) | ((uint32_t)b[4 * l + 1] << 16) | ((uint32_t)b[4 * l + 2] << 8) | b[4 * l + 3];
  }
  const uint8_t b0 = (uint8_t)(xc.v[11] >> 24);
  xc.v[11] &= 0x1fffffffu;
  const bool compressed = b0 & 0x80, infinity = b0 & 0x40, sort = b0 & 0x20;
  Aff res = Aff::identity();
  uint8_t st = 0;
  if (!compressed) {
    st = 1;
  } else if (infinity) {
    if (sort || !xc.is_zero()) st = 1;
  } else {
    Fp pm;   // x must be < p
    for (int i = 0; i < 12; i++) pm.v[i] = FpCfg::P[i];
    if (!fe_raw_gt(pm, xc)) {
      st = 1;
    } else {
      const Fp x = fe_to_mont(xc);
      const F28 x28 = f28_from_std(x);
      const F28 rhs = f28_add(f28_mul(f28_sqr(x28), x28), f28_const(F28Cfg::FOUR));
      const F28 y28 = f28_sqrt_device(rhs);
      if (!f28_eq(f28_sqr(y28), rhs)) {
        st = 1;
      } else {
        const Fp y = f28_to_std(y28), ny = fe_neg(y);
        const bool y_larger = fe_raw_gt(fe_from_mont(y), fe_from_mont(ny));
        const bool keep = (y_larger == sort);
        res.x = x;
        res.y = keep ? y : ny;
        if (check_subgroup && !g1_in_subgroup_device(Aff28{x28, f28_cneg(y28, !keep)})) st = 2;
      }
    }
  }
  out[dst_index ? dst_index[g] : g] = st ? Aff::identity() : res;
  status[g] = st;
}

// A few points (a lone proof's 45): one QUAD per point.  The four lanes parse the encoding and take the square root redundantly; the
// subgroup test — [u^2] P by two chains of 63 doublings and 5 additions, what a lone verification waits for longest — runs on the
// quad-cooperative XYZZ formulas (g1_28_quad.hpp: 4.4 us per doubling instead of 7.6 us).  Same verdicts as k_decompress.
__device__ __forceinline__ bool g1_28_in_subgroup_quad(const Aff28& P, TAcc* slot /* [3]: scratch, P, [|u|] P */) {
  const int sub = threadIdx.x & 3;
  const bool idP = P.is_identity();
  const uint64_t U = 0xd201000000010000ull;
  TAcc acc = idP ? TAcc::identity() : TAcc{P.x, P.y, f28_one(), f28_one()};
  if (sub == 0) slot[1] = acc;
  for (int pass = 0; pass < 2; pass++) {      // [|u|] P, then [|u|] ([|u|] P)
    if (sub == 0) slot[2] = acc;              // (pass 0: unused; pass 1: the addend [|u|] P)
    __syncthreads();
    for (int b = 62; b >= 0; b--) {
      acc = xyzz28_dbl_quad(acc);
      if ((U >> b) & 1) {
        if (sub == 0) slot[0] = acc;
        __syncthreads();
        acc = xyzz28_add_quad_mem(slot, 0, 1 + pass);
        __syncthreads();
      }
    }
  }
  if (idP) return true;
  if (acc.is_identity()) return false;
  // (beta x_P, y_P) == (X / ZZ, -Y / ZZZ)
  const F28 lhs_x = f28_mul(f28_mul(f28_const(F28Cfg::BETA), P.x), acc.zz);
  const F28 lhs_y = f28_mul(P.y, acc.zzz);
  return f28_eq(lhs_x, acc.x) && f28_eq(lhs_y, f28_neg(acc.y));
}
__global__ __launch_bounds__(64) void k_decompress_quad(const uint8_t* __restrict__ in, int n, Aff* __restrict__ out, const uint32_t* __restrict__ dst_index,
                                                         uint8_t* __restrict__ status, int check_subgroup, const uint32_t* __restrict__ src_offset) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  TAcc* buf = reinterpret_cast<TAcc*>(smem);   // [16][3]
  const int quad = threadIdx.x >> 2, sub = threadIdx.x & 3;
  const int g = blockIdx.x * 16 + quad;
  const bool live = g < n;
  Aff res = Aff::identity();
  Aff28 chk = Aff28::identity();               // the point whose membership is tested (identity: nothing to test)
  uint8_t st = 0;
  if (live) {
    const uint8_t* b = in + (src_offset ? (size_t)src_offset[g] : (size_t)g * 48);
    Fp xc;
    for (int l = 0; l < 12; l++) xc.v[11 - l] = ((uint32_t)b[4 * l] << 24) | ((uint32_t)b[4 * l + 1] << 16) | ((uint32_t)b[4 * l + 2] << 8) | b[4 * l + 3];
    const uint8_t b0 = (uint8_t)(xc.v[11] >> 24);
    xc.v[11] &= 0x1fffffffu;
    const bool compressed = b0 & 0x80, infinity = b0 & 0x40, sort = b0 & 0x20;
    if (!compressed) {
      st = 1;
    } else if (infinity) {
      if (sort || !xc.is_zero()) st = 1;
    } else {
      Fp pm;   // x must be < p
      for (int i = 0; i < 12; i++) pm.v[i] = FpCfg::P[i];
      if (!fe_raw_gt(pm, xc)) {
        st = 1;
      } else {
        const Fp x = fe_to_mont(xc);
        const F28 x28 = f28_from_std(x);
        const F28 rhs = f28_add(f28_mul(f28_sqr(x28), x28), f28_const(F28Cfg::FOUR));
        const F28 y28 = f28_sqrt_device(rhs);
        if (!f28_eq(f28_sqr(y28), rhs)) {
          st = 1;
        } else {
          const Fp y = f28_to_std(y28), ny = fe_neg(y);
          const bool y_larger = fe_raw_gt(fe_from_mont(y), fe_from_mont(ny));
          const bool keep = (y_larger == sort);
          res.x = x;
          res.y = keep ? y : ny;
          if (check_subgroup) chk = Aff28{x28, f28_cneg(y28, !keep)};
        }
      }
    }
  }
  if (!g1_28_in_subgroup_quad(chk, buf + quad * 3)) st = 2;   // every lane of the wave takes part
  if (!live || sub != 0) return;
  out[dst_index ? dst_index[g] : g] = st ? Aff::identity() : res;
  status[g] = st;
}


// sum of n Jacobian points (the partial sums of several engines / GPUs); flag[0] = 1 iff the sum is the identity
__global__ __launch_bounds__(64) void k_sum_jac(const Jac* __restrict__ in, int n, Jac* __restrict__ out, int* __restrict__ flag) {
  if (threadIdx.x || blockIdx.x) return;
  TJac acc = TJac::identity();
  for (int i = 0; i < n; i++) acc = t_add(acc, t_jac_from_std(in[i]));
  out[0] = t_jac_to_std(acc);
  flag[0] = acc.is_identity() ? 1 : 0;
}

// ------------------------------------------------------------------ Fr algebra of the log rounds on the device
// The prover's per-round scalar vectors (cross-term scalars = vector entry x fold coefficient, the two inner products,
// the folds of c, d / x and the updates of the fold coefficients S) are elementwise Fr work on vectors that never need
// to leave the GPU: the host only hashes the round's L/R points and sends back the challenge gamma and its inverse.
// Round j of n = 2^L elements: half = n >> (j+1); original base k has bit `half` set (hi) or clear (lo); the t-th
// lo index is kl = (t / half) * 2 half + t % half, the t-th hi index kh = kl + half (t < n/2).
//
// IPA (inner_product_argument.rs:150-186 in all-MSM form).  vec: [B][4][n] = c | d | SG | SGp.
// out per proof: [ L_C scalars (n/2), beta<c_L,d_R> | L_D (n/2) | R_C (n/2), beta<c_R,d_L> | R_D (n/2) ]
// (n = the elements the round still works on: the full length, or m for the late rounds on materialised bases (late.hip), which
// restart the fold coefficients at 1 inside the first m entries; stride = the allocated length of every sub-vector)
__global__ __launch_bounds__(128) void k_ipa_round_scalars(const Fr* __restrict__ vec, int stride, int n, int half, const Fr* __restrict__ beta, Fr* __restrict__ out) {
  __shared__ Fr red[2][128];
  const int p = blockIdx.x, hn = n / 2;
  const Fr* c = vec + (size_t)p * 4 * stride;
  ipa_round_scalars_body(c, c + stride, c + 2 * stride, c + 3 * stride, n, half, beta[p], out + (size_t)p * (4 * hn + 2), &red[0][0]);
}
// gam: [B][2] = gamma, gamma^-1.  c_L += gamma^-1 c_R, d_L += gamma d_R, SG[hi] *= gamma, SGp[hi] *= gamma^-1
__global__ __launch_bounds__(128) void k_ipa_round_fold(Fr* __restrict__ vec, int stride, int n, int half, const Fr* __restrict__ gam) {
  const int p = blockIdx.x;
  Fr* c = vec + (size_t)p * 4 * stride;
  const Fr g = gam[2 * p], gi = gam[2 * p + 1];
  ipa_round_fold_body(c, c + stride, c + 2 * stride, c + 3 * stride, n, half, g, gi);
}
// SameMSM (same_multiscalar_argument.rs:99-136 in all-MSM form).  vec: [B][2][n] = x | SM.
// out per proof: [ L_* scalars (n/2) | R_* scalars (n/2) ]
__global__ __launch_bounds__(128) void k_smsm_round_scalars(const Fr* __restrict__ vec, int stride, int n, int half, Fr* __restrict__ out) {
  const int p = blockIdx.x, hn = n / 2;
  const Fr* x = vec + (size_t)p * 2 * stride;
  smsm_round_scalars_body(x, x + stride, n, half, out + (size_t)p * 2 * hn);
}
// gam: [B][2] = gamma, gamma^-1.  x_L += gamma^-1 x_R, SM[hi] *= gamma
__global__ __launch_bounds__(128) void k_smsm_round_fold(Fr* __restrict__ vec, int stride, int n, int half, const Fr* __restrict__ gam) {
  const int p = blockIdx.x;
  Fr* x = vec + (size_t)p * 2 * stride;
  const Fr g = gam[2 * p], gi = gam[2 * p + 1];
  smsm_round_fold_body(x, x + stride, n, half, g, gi);
}

// ------------------------------------------------------------------ transcript prefix on the device
// Every prover / verifier transcript starts by absorbing the compressed instance (4 vectors of ell points and M, 48 KB
// at ell = 252) and drawing the ell challenges of vec_a (curdleproofs.rs:78-83, :213-222): ~770 Keccak permutations
// per proof, a third of the host's per-proof work.  The bytes are produced on the GPU anyway (k_compress), so they are
// hashed here and only the transcript state (25 lanes + pos + pos_begin) and vec_a travel to the host, which
// continues from the state (host::Transcript::load_state).
//
// Lane-parallel STROBE (wave_strobe.hpp): one wave per proof, the 25 state words bit-interleaved over the two halves of the wave
// (a single GPU lane needs ~17 us per permutation).  Message bytes are absorbed by the lanes that own their position in the rate.
// Same semantics as strobe.hpp (the host's code), pinned by the bit-exact proof tests.
// out_state: [nproofs][27] u64, out_vec_a: [nproofs][ell] Fr (Montgomery wire form)
// EXCL (small batches, option transcript_excl_max): the wave claims all 512 registers of its SIMD, so no wave of the kernels that run
// beside the prefix (table build, phase 1, decompression) is placed on the same SIMD — a lone dependent chain that shares its SIMD
// takes 1.7 times as long, and the slowest wave is the kernel.
template <bool EXCL>
__global__ __launch_bounds__(64) void k_transcript_step1(const uint8_t* __restrict__ inst_comp, const uint8_t* __restrict__ m_comp, int nproofs, int ell,
                                                         uint64_t* __restrict__ out_state, Fr* __restrict__ out_vec_a) {
  __shared__ uint8_t scratch[64];
  const int p = blockIdx.x;
  if (p >= nproofs) return;
#if defined(__gfx950__)
  if (EXCL) {   // (gfx950's unified 512-register file: see k_smul)
    asm volatile("v_mov_b32 v255, 0" ::: "v255");
    asm volatile("v_accvgpr_write_b32 a255, 0" ::: "a255");
  }
#elif defined(__HIP_DEVICE_COMPILE__)
  static_assert(!EXCL, "the exclusive-SIMD form is written for gfx950's register file");
#endif
  WaveStrobe t;
  t.set_lane(threadIdx.x);
  t.init("curdleproofs", 12, scratch);
  for (int v = 0; v < 4; v++) {   // Vec<G1Affine>: u64-LE length prefix, then the compressed points, as one message
    t.append_begin("curdleproofs_step1", 18, 8 + 48 * (size_t)ell, scratch);
    if (t.l < 8) scratch[8 + t.l] = (uint8_t)((uint64_t)ell >> (8 * t.l));
    wave_lds_sync();
    t.absorb(scratch + 8, 8);
    t.absorb(inst_comp + ((size_t)p * 4 + v) * ell * 48, 48 * (size_t)ell);
  }
  t.append_begin("curdleproofs_step1", 18, 48, scratch);
  t.absorb(m_comp + (size_t)p * 48, 48);
  for (int i = 0; i < ell; i++) {   // get_and_append_challenge (transcript.rs:40-60)
    Fr c;
    while (!t.challenge_attempt("curdleproofs_vec_a", 18, scratch, c)) {
    }
    if (threadIdx.x == 0) out_vec_a[(size_t)p * ell + i] = c;   // canonical for now
  }
  t.store(out_state + (size_t)p * 27);
  // Montgomery form, 64 challenges at a time (a product per challenge inside the serial loop above costs as much as half a permutation)
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
  for (int i = threadIdx.x; i < ell; i += 64) {
    Fr* q = out_vec_a + (size_t)p * ell + i;
    *q = fe_to_mont(*q);
  }
}

// The same prefix with ONE LANE per transcript (large batches: option transcript_lane_min_batch).  The lane-parallel form above is built
// for latency — 32 lanes and ~1.07 M wave instructions per pair of proofs, 3.5 % of a pass's VALU time at 8192 proofs — but a large
// batch hides the prefix behind the table build (prover) and the decompression (verifier) anyway; one lane per transcript runs the
// plain 64-bit Keccak of strobe.hpp (~1/5 of the wave instructions per proof) on 1/32 of the waves (LaneStrobe, lane_strobe.hpp: the
// sponge state in LDS, word-interleaved by lane).
__global__ __launch_bounds__(64) void k_transcript_step1_lane(const uint8_t* __restrict__ inst_comp, const uint8_t* __restrict__ m_comp, int nproofs, int ell,
                                                              uint64_t* __restrict__ out_state, Fr* __restrict__ out_vec_a) {
  __shared__ uint64_t lds[25 * 64];
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= nproofs) return;   // (no barrier below: a lane only touches its own words)
  LaneStrobe t;
  t.st = lds + threadIdx.x;
  t.init("curdleproofs", 12);
  for (int v = 0; v < 4; v++) {   // Vec<G1Affine>: u64-LE length prefix, then the compressed points, as one message
    t.append_begin("curdleproofs_step1", 18, 8 + 48 * (size_t)ell);
    uint8_t len8[8];
    for (int j = 0; j < 8; j++) len8[j] = (uint8_t)((uint64_t)ell >> (8 * j));
    t.absorb(len8, 8);
    t.absorb(inst_comp + ((size_t)p * 4 + v) * ell * 48, 48 * (size_t)ell);
  }
  t.append_begin("curdleproofs_step1", 18, 48);
  t.absorb(m_comp + (size_t)p * 48, 48);
  for (int i = 0; i < ell; i++) {   // get_and_append_challenge (transcript.rs:40-60), as in k_transcript_step1
    Fr c;
    while (!t.challenge_attempt("curdleproofs_vec_a", 18, c)) {
    }
    out_vec_a[(size_t)p * ell + i] = fe_to_mont(c);
  }
  uint64_t* o = out_state + (size_t)p * 27;
  for (int i = 0; i < 25; i++) o[i] = t.w(i);
  o[25] = t.pos;
  o[26] = t.pos_begin;
}

// ------------------------------------------------------------------ micro-benchmarks (bench.py --micro)
// Dependent Fp multiply chains: measures the achieved modular-multiply rate of this build.
__global__ __launch_bounds__(256) void k_bench_fpmul(Fp* data, int iters) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  Fp x = data[g], y = data[g + gridDim.x * blockDim.x];
  for (int i = 0; i < iters; i++) {
    x = fe_mul(x, y);
    y = fe_mul(y, x);
  }
  data[g] = fe_add(x, y);
}
// the same chain on the 28-bit-limb field (fp28.hpp), with the product body the hot loops use by default (F28_KARA,
// F28_REDC_KARA): the peak roofline.valu divides by stays comparable with the kernels
__global__ __launch_bounds__(256) void k_bench_f28mul(Fp* data, int iters) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  F28 x = f28_from_std(data[g]), y = f28_from_std(data[g + gridDim.x * blockDim.x]);
  for (int i = 0; i < iters; i++) {
    x = f28_mul(x, y);
    y = f28_mul(y, x);
  }
  data[g] = f28_to_std(f28_add(x, y));
}

// ------------------------------------------------------------------ host-callable launchers
// Every launch goes through hipExtLaunchKernelGGL so that, when the engine is profiling, the pair of events set
// by set_launch_events() is bound to the dispatch itself (kernel begin / end — the interval rocprofv3 reports)
// instead of bracketing it on the stream, which would include queueing behind another engine's kernels.
static thread_local hipEvent_t tl_ev_start = nullptr, tl_ev_stop = nullptr;
static thread_local int tl_launches = 0;

// ---- options (kernels.h) ----
namespace {
struct OptField {
  const char* key;
  long Options::*field;
  long lo, hi;
};
const OptField kOptFields[] = {
    {"tail_wave_max", &Options::tail_wave_max, 0, 1L << 30},     {"tbw_min_waves", &Options::tbw_min_waves, 0, 1L << 30},
    {"tbw_wpw", &Options::tbw_wpw, 0, 32},                       {"tbw_lat_waves", &Options::tbw_lat_waves, 0, 1L << 30},
    {"tbw_slices", &Options::tbw_slices, 0, 4},                  {"reduce_wave_max", &Options::reduce_wave_max, -1, 1L << 30},
    {"fix_min_waves", &Options::fix_min_waves, 0, 1L << 30},     {"fix_lat_waves", &Options::fix_lat_waves, 0, 1L << 30},
    {"finalize_wave_max", &Options::finalize_wave_max, 0, 1L << 30}, {"table_quad_max", &Options::table_quad_max, 0, 1L << 30},
    {"decompress_quad_max", &Options::decompress_quad_max, 0, 1L << 30}, {"fix_bits", &Options::fix_bits, 8, 19},
    {"device_min_batch", &Options::device_min_batch, 1, 1L << 30}, {"spin_team", &Options::spin_team, 0, 1},
    {"spin_team_threads", &Options::spin_team_threads, 1, 256},  {"inline_below", &Options::inline_below, 0, 1L << 30},
    {"cu_mask", &Options::cu_mask, 0, 1},                        {"trace", &Options::trace, 0, 1},
    {"bench_field", &Options::bench_field, 12, 28},              {"serial_streams", &Options::serial_streams, 0, 1},
    {"p1_split", &Options::p1_split, 0, 1},                      {"transcript_lane_min_batch", &Options::transcript_lane_min_batch, 1, 1L << 30},
    {"late_rounds", &Options::late_rounds, 0, 4},                {"late_min_batch", &Options::late_min_batch, 1, 1L << 30},
    {"late_slices", &Options::late_slices, 1, 8},                {"rs_pairs", &Options::rs_pairs, 0, 1},                         {"late_m", &Options::late_m, 0, 64},
    {"table_chunks", &Options::table_chunks, 0, 64},                {"msm_endo_min", &Options::msm_endo_min, 1, 1L << 30},
    {"transcript_excl_max", &Options::transcript_excl_max, 0, 1L << 30}, {"table_stream_max", &Options::table_stream_max, 0, 1L << 30},
    {"scale_any_point", &Options::scale_any_point, 0, 1},         {"strict_infinity", &Options::strict_infinity, 0, 1},
    {"fused_rounds_max", &Options::fused_rounds_max, 0, 1L << 30}, {"fused_smsm_max", &Options::fused_smsm_max, 0, 1L << 30}, {"fused_fix_wpw", &Options::fused_fix_wpw, 0, 16},
    {"smul_quad_max", &Options::smul_quad_max, 0, 1L << 30},       {"fused_tbl_wpw", &Options::fused_tbl_wpw, 8, 32},             {"fused_combine", &Options::fused_combine, -1, 1},
    {"tbl_segments", &Options::tbl_segments, 0, 2},                {"fold_quad_max", &Options::fold_quad_max, 0, 1L << 30},
    {"locate_groups_max", &Options::locate_groups_max, 1, 256},    {"find_table_min_keys", &Options::find_table_min_keys, 1, (1L << 20) + 1},
    {"find_table_mb", &Options::find_table_mb, 1, 65536},          {"rng_g1_round_cap", &Options::rng_g1_round_cap, 0, 1L << 20},
    {"rs_from_tables", &Options::rs_from_tables, 0, 1},
};
bool option_value_ok(const OptField& f, long v) {
  if (v < f.lo || v > f.hi) return false;
  if (!strcmp(f.key, "tbw_wpw")) return v == 0 || v == 2 || v == 4 || v == 8 || v == 16 || v == 32;
  if (!strcmp(f.key, "tbw_slices")) return v == 0 || v == 1 || v == 2 || v == 4;
  if (!strcmp(f.key, "fix_bits")) return v == 8 || v == 16 || v == 19;
  if (!strcmp(f.key, "late_rounds")) return v == 0 || v == 4;
  if (!strcmp(f.key, "late_m")) return v == 0 || v == 16 || v == 32 || v == 64;
  if (!strcmp(f.key, "late_slices")) return v == 1 || v == 2 || v == 4 || v == 8;
  if (!strcmp(f.key, "fused_fix_wpw")) return v == 0 || v == 4 || v == 8 || v == 16;
  if (!strcmp(f.key, "fused_tbl_wpw")) return v == 8 || v == 16 || v == 32;
  return true;
}
}  // namespace
bool set_option(Options& o, const char* key, long value) {
  if (!key) return false;
  for (const OptField& f : kOptFields)
    if (!strcmp(f.key, key)) {
      if (!option_value_ok(f, value)) return false;
      o.*(f.field) = value;
      return true;
    }
  return false;
}
bool get_option(const Options& o, const char* key, long* value) {
  if (!key) return false;
  for (const OptField& f : kOptFields)
    if (!strcmp(f.key, key)) {
      if (value) *value = o.*(f.field);
      return true;
    }
  return false;
}
const Options& default_options() {
  static const Options defaults = [] {   // the environment is read ONCE per process and only seeds new contexts
    Options o;
    for (const OptField& f : kOptFields) {
      std::string name = "CPX_";
      for (const char* c = f.key; *c; c++) name += (char)toupper((unsigned char)*c);
      const char* e = getenv(name.c_str());
      if (!e && !strcmp(f.key, "device_min_batch")) e = getenv("CPX_DEVICE_TRANSCRIPT_MIN_BATCH");   // former name
      if (e && *e) (void)set_option(o, f.key, atol(e));   // an out-of-range value keeps the built-in default
    }
    return o;
  }();
  return defaults;
}
void set_launch_events(hipEvent_t start, hipEvent_t stop) {
  tl_ev_start = start;
  tl_ev_stop = stop;
  tl_launches = 0;
}
int launches_since_set() { return tl_launches; }
void take_launch_events(hipEvent_t* start, hipEvent_t* stop) {
  tl_launches++;
  *start = tl_ev_start;
  *stop = tl_ev_stop;
}
#define CPX_LAUNCH(kern, grid, block, lds, stream, ...)                                                   \
  do {                                                                                                    \
    tl_launches++;                                                                                        \
    if (tl_ev_start || tl_ev_stop) hipExtLaunchKernelGGL(kern, grid, block, lds, stream, tl_ev_start, tl_ev_stop, 0, __VA_ARGS__); \
    else hipLaunchKernelGGL(kern, grid, block, lds, stream, __VA_ARGS__);   /* plain launch: capturable into a HIP graph */ \
  } while (0)
void launch_msm_accum(const MsmTask* d_tasks, int ntasks, int max_n, TAff* d_conv, TJac* d_wsum, hipStream_t s) {
  if (ntasks <= 0) return;
  if (max_n > 0) {
    hipEvent_t ea = tl_ev_start, eb = tl_ev_stop;   // the profiling events belong to the accumulation kernel
    tl_ev_start = tl_ev_stop = nullptr;
    CPX_LAUNCH(k_to_table, dim3((max_n + 63) / 64, ntasks), dim3(64), 0, s, d_tasks, d_conv);
    tl_ev_start = ea;
    tl_ev_stop = eb;
  }
  CPX_LAUNCH(k_msm_accw, dim3(ntasks * 8), dim3(64), ACW_LDS, s, d_tasks, d_conv, d_wsum);
}
void launch_msm_tail(const Options& o, const TJac* d_in, TJac* d_out, Jac* d_out_std, int nout, int group, int shift, hipStream_t s, const TJac* d_extra, int extra_per_out,
                     int dup) {
  if (nout <= 0) return;
  const long wave_max = o.tail_wave_max;   // moves the switch-over (tests reach both forms with small inputs)
  if (nout <= wave_max && shift > 0 && group <= 16 && dup >= 1 && (dup & (dup - 1)) == 0 && extra_per_out <= 64 &&
      group * dup + extra_per_out <= 255) {   // a few outputs: wave per output, windows shifted side by side
    const size_t lds = (size_t)(group * dup + extra_per_out + 1) * sizeof(TAcc);
    if (d_out_std) CPX_LAUNCH(k_msm_tail_wave<true>, dim3(nout), dim3(64), lds, s, d_in, d_out, d_out_std, group, shift, d_extra, extra_per_out, dup);
    else CPX_LAUNCH(k_msm_tail_wave<false>, dim3(nout), dim3(64), lds, s, d_in, d_out, d_out_std, group, shift, d_extra, extra_per_out, dup);
    return;
  }
  if (d_out_std) CPX_LAUNCH(k_msm_tail<true>, dim3((nout + 63) / 64), dim3(64), 0, s, d_in, d_out, d_out_std, nout, group, shift, d_extra, extra_per_out, dup);
  else CPX_LAUNCH(k_msm_tail<false>, dim3((nout + 63) / 64), dim3(64), 0, s, d_in, d_out, d_out_std, nout, group, shift, d_extra, extra_per_out, dup);
}
void launch_msm_endo(const MsmTask* d_tasks, int ntasks, int max_n, TAff* d_conv, uint32_t* d_digits, TblTask* d_ttasks, uint32_t* d_raw, uint32_t* d_raw_slot,
                     hipStream_t s, int slices) {
  if (ntasks <= 0) return;
  {
    hipEvent_t ea = tl_ev_start, eb = tl_ev_stop;   // the profiling events belong to the accumulation kernel
    tl_ev_start = tl_ev_stop = nullptr;
    CPX_LAUNCH(k_to_table_endo, dim3((std::max(max_n, 1) + 63) / 64, ntasks), dim3(64), 0, s, d_tasks, d_conv, d_digits, d_ttasks, slices);
    tl_ev_start = ea;
    tl_ev_stop = eb;
  }
  CPX_LAUNCH((k_msm_tblw<2, true>), dim3(ntasks * 16 * slices), dim3(64), TBW_LDS, s, d_ttasks, d_raw, d_raw_slot, slices);
}
void launch_msm_endo_pairs(const MsmTask* d_tasks, int npairs, int max_n, TAff* d_conv, uint32_t* d_digits, TblTask* d_ttasks, uint32_t* d_raw, uint32_t* d_raw_slot,
                           hipStream_t s) {
  if (npairs <= 0) return;
  {
    hipEvent_t ea = tl_ev_start, eb = tl_ev_stop;   // the profiling events belong to the accumulation kernel
    tl_ev_start = tl_ev_stop = nullptr;
    CPX_LAUNCH(k_to_table_endo, dim3((std::max(max_n, 1) + 63) / 64, 2 * npairs), dim3(64), 0, s, d_tasks, d_conv, d_digits, d_ttasks, 1);
    tl_ev_start = ea;
    tl_ev_stop = eb;
  }
  CPX_LAUNCH(k_msm_tblw_pair, dim3(npairs * 16), dim3(64), TBW_LDS, s, d_ttasks, d_raw, d_raw_slot);
}
int msm_tblw_windows_per_wave(const Options& o, int ntasks) {
  // the largest group of windows per wave that still yields one wave per wave slot of the GPU (256 CUs x 4 SIMDs x 2);
  // a task takes 32 / wpw waves, each of which leaves two raw sets (-> 64 / wpw partial sums per task)
  const long min_waves = o.tbw_min_waves;
  if (o.tbw_wpw) return (int)o.tbw_wpw;   // 2|4|8|16|32 pins the grouping (tests exercise every instantiation)
  for (int wpw = 32; wpw > 8; wpw >>= 1)
    if ((long)ntasks * (TBW_WINDOWS / wpw) >= min_waves) return wpw;
  // a few proofs in flight: latency matters, so spread a task over as many (short) waves as the GPU can hold at once
  const long lat_waves = o.tbw_lat_waves;
  if ((long)ntasks * 16 <= lat_waves) return 2;
  if ((long)ntasks * 8 <= lat_waves) return 4;
  return 8;
}
int msm_tblw_parts(int wpw, int segments) { return (int)tbw_parts((uint32_t)wpw, (uint32_t)segments); }   // recode.hpp, shared with the waves
int msm_tblw_slices(const Options& o, int ntasks, int wpw, int max_n) {
  // waves per task over its points: only when the GPU would otherwise stand almost empty (a lone proof: 16 waves per task) and a
  // slice keeps >= 256 points — below that the longest of a wave's 128 bucket lists no longer shrinks with the slice (a lane adds
  // max, not mean, and 64 points leave lists of 0..6), while every slice costs two more sets to reduce
  return tbw_slices_rule(o.tbw_slices, ntasks, wpw, max_n);   // tier0_plan.hpp: the rule, where a host program can check it
}
void launch_msm_tblw(const TblTask* d_tasks, int ntasks, int wpw, uint32_t* d_raw, uint32_t* d_raw_slot, hipStream_t s, int slices, int segments) {
  if (ntasks <= 0) return;
  const dim3 grid(ntasks * (TBW_WINDOWS / wpw) * slices), block(64);
  if (segments == 2) {
    switch (wpw) {
      case 32: CPX_LAUNCH(k_msm_tblw2<32>, grid, block, TBW2_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
      case 16: CPX_LAUNCH(k_msm_tblw2<16>, grid, block, TBW2_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
      case 4: CPX_LAUNCH(k_msm_tblw2<4>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
      case 2: CPX_LAUNCH(k_msm_tblw2<2>, grid, block, TBW_LDS_CACHE, s, d_tasks, d_raw, d_raw_slot, slices); break;
      default: CPX_LAUNCH(k_msm_tblw2<8>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
    }
    return;
  }
  switch (wpw) {
    case 32: CPX_LAUNCH(k_msm_tblw<32>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
    case 16: CPX_LAUNCH(k_msm_tblw<16>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
    case 4: CPX_LAUNCH(k_msm_tblw<4>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
    case 2: CPX_LAUNCH(k_msm_tblw<2>, grid, block, TBW_LDS_CACHE, s, d_tasks, d_raw, d_raw_slot, slices); break;
    default: CPX_LAUNCH(k_msm_tblw<8>, grid, block, TBW_LDS, s, d_tasks, d_raw, d_raw_slot, slices); break;
  }
}
size_t raw_set_words() { return RAW_SET_WORDS; }
size_t reduce_mid_per_set() { return (MID_PER_SET * sizeof(TAcc) + sizeof(TJac) - 1) / sizeof(TJac); }
void launch_reduce_sets(const Options& o, const uint32_t* d_raw, const uint32_t* d_raw_slot, int nplain, int nweighted, TJac* d_mid, TJac* d_part, hipStream_t s,
                        int nproofs) {
  const int nsets = nplain + nweighted;
  if (nsets <= 0) return;
  // reduce_wave_max / finalize_wave_max move the switch-over between the latency (wave per item) and the
  // throughput instantiations, so that tests reach the throughput kernels with small batches.
  // The wave form spends ~4x the lane time of the work-efficient form: it pays while the GPU is not full — up to 16384 sets when
  // at most 1024 proofs are in flight (64 ... 512 proofs per pass: +5-9 %, 1024: +2 %); a large batch (several contexts keep the GPU busy) keeps
  // it for launches of at most 2048 sets (at 16384 for every batch size the bench lost 3 %)
  const long forced = o.reduce_wave_max;
  const long wave_max = forced >= 0 ? forced : (nproofs > 0 && nproofs <= 1024 ? 16384L : 2048L);   // (1024 proofs: 94.0 -> 92.0 ms per pass, 512: no difference)
  if (nsets <= wave_max) {   // a few proofs: wave per set, both kinds in one launch
    CPX_LAUNCH(k_reduce_sets_wave, dim3(nsets), dim3(64), QP_ENTRIES * sizeof(TAcc), s, d_raw, d_raw_slot, nplain, d_part);
    return;
  }
  const dim3 block(64);
  TAcc* const mid = reinterpret_cast<TAcc*>(d_mid);   // reduce_mid_per_set() TJac per set hold MID_PER_SET TAcc
  if (nplain > 0) {
    CPX_LAUNCH(k_reduce_sets<false>, dim3((nplain * 8 + 63) / 64), block, 0, s, d_raw, nplain, mid);
    CPX_LAUNCH(k_reduce_groups<false>, dim3((nplain + 63) / 64), block, 0, s, mid, d_raw_slot, nplain, d_part);
  }
  if (nweighted > 0) {   // (an even number of plain sets keeps the lower / upper parity of the bucket sets)
    const uint32_t* raw_w = d_raw + (size_t)nplain * RAW_SET_WORDS;
    TAcc* mid_w = mid + (size_t)nplain * MID_PER_SET;
    CPX_LAUNCH(k_reduce_sets<true>, dim3((nweighted * 8 + 63) / 64), block, 0, s, raw_w, nweighted, mid_w);
    CPX_LAUNCH(k_reduce_groups<true>, dim3((nweighted + 63) / 64), block, 0, s, mid_w, d_raw_slot + nplain, nweighted, d_part);
  }
}
int msm_fix_windows_per_wave(const Options& o, int ntasks, int cbits) {
  if (cbits == 19) return 7;   // 14 windows: two waves per task, 7 windows x 9 point slices each
  const int w = 256 / cbits;
  const long min_waves = o.fix_min_waves;   // default: two waves per SIMD
  if ((long)ntasks * (w / 16) >= min_waves) return 16;
  const long lat_waves = o.fix_lat_waves;   // up to how many waves the short-wave forms may launch
  if (cbits == 16) {   // a few proofs in flight: more, shorter waves per task
    if ((long)ntasks * 8 <= lat_waves) return 2;
    if ((long)ntasks * 4 <= lat_waves) return 4;
  }
  return 8;
}
void launch_msm_fix(const FixTask* d_tasks, int ntasks, const TFix* d_fix_tab, int cbits, int wpw, int nc, uint32_t* d_raw, uint32_t* d_raw_slot, hipStream_t s) {
  if (ntasks <= 0) return;
  const size_t lds = 16 * FIX_CHUNK * 2;   // digit rows (7 rows of 32-bit digits at 19 bits)
  const dim3 grid(ntasks * msm_fix_parts(cbits, wpw)), block(64);
  if (cbits == 19) CPX_LAUNCH((k_msm_fix<19, 7>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else if (cbits == 16 && wpw == 16) CPX_LAUNCH((k_msm_fix<16, 16>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else if (cbits == 16 && wpw == 4) CPX_LAUNCH((k_msm_fix<16, 4>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else if (cbits == 16 && wpw == 2) CPX_LAUNCH((k_msm_fix<16, 2>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else if (cbits == 16) CPX_LAUNCH((k_msm_fix<16, 8>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else if (wpw == 16) CPX_LAUNCH((k_msm_fix<8, 16>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
  else CPX_LAUNCH((k_msm_fix<8, 8>), grid, block, lds, s, d_tasks, d_fix_tab, nc, d_raw, d_raw_slot);
}
void launch_msm_fix_tblw(const FixTask* d_ftasks, int nftasks, const TFix* d_fix_tab, int nc, uint32_t* d_fraw, uint32_t* d_fraw_slot, const TblTask* d_ttasks,
                         int nttasks, int slices, uint32_t* d_traw, uint32_t* d_traw_slot, hipStream_t s) {
  const uint32_t nfix_blocks = (uint32_t)nftasks * 8, ntbl_blocks = (uint32_t)nttasks * 16 * (uint32_t)slices;
  const size_t lds = std::max<size_t>(16 * FIX_CHUNK * 2, TBW_LDS_CACHE);
  CPX_LAUNCH(k_msm_fix_tblw, dim3(nfix_blocks + ntbl_blocks), dim3(64), lds, s, d_ftasks, d_fix_tab, nc, d_fraw, d_fraw_slot, nfix_blocks, d_ttasks, d_traw,
             d_traw_slot, slices);
}
int msm_fix_windows(int cbits) { return (256 + cbits - 1) / cbits; }
int msm_fix_parts(int cbits, int wpw) { return msm_fix_windows(cbits) / wpw; }
void launch_fix_build(const TAff* d_shift, int nc, int cbits, TFix* d_fix_tab, TblTmp* d_tmp, int chunk, hipStream_t s, int segs) {
  const int W = msm_fix_windows(cbits), total = W * nc * segs;
  const size_t lds = 2 * 64 * sizeof(TF);
  if (cbits == 19) CPX_LAUNCH(k_fix_build<19>, dim3((total + 63) / 64), dim3(64), lds, s, d_shift, nc, d_fix_tab, d_tmp, chunk, segs);
  else if (cbits == 16) CPX_LAUNCH(k_fix_build<16>, dim3((total + 63) / 64), dim3(64), lds, s, d_shift, nc, d_fix_tab, d_tmp, chunk, segs);
  else CPX_LAUNCH(k_fix_build<8>, dim3((total + 63) / 64), dim3(64), lds, s, d_shift, nc, d_fix_tab, d_tmp, chunk, segs);
}
void launch_finalize_ranges(const Options& o, const TJac* d_part, const uint32_t* d_first, const uint32_t* d_count, int n, Aff* d_aff, const uint32_t* d_dst_index,
                            uint8_t* d_comp, hipStream_t s, const uint32_t* d_addends, const uint32_t* d_comp_index) {
  if (n <= 0) return;
  const long wave_max = o.finalize_wave_max;
  if (n <= wave_max) {   // a few proofs: wave per request (tree over the partial sums)
    CPX_LAUNCH(k_finalize_ranges_wave, dim3(n), dim3(64), 256 * sizeof(TAcc), s, d_part, d_first, d_count, n, d_aff, d_dst_index, d_comp, d_addends, d_comp_index);
    return;
  }
  CPX_LAUNCH(k_finalize_ranges, dim3((n + 63) / 64), dim3(64), 2 * 64 * sizeof(TF), s, d_part, d_first, d_count, n, d_aff, d_dst_index, d_comp, d_addends, d_comp_index);
}
void launch_table_build(const Options& o, const Aff* d_src, size_t src_row_stride, TAff* d_table, int rows, size_t row_stride, int npts, int copy_stride, int copies, bool endo,
                        TblTmp* d_tmp, hipStream_t s, int step_bits) {
  const long total = (long)rows * npts;
  if (total <= 0) return;
  // single-wave work-groups: a 256-thread group of this 241-VGPR kernel only ever got one group per CU (38 ms against 19 ms per
  // 2048 proofs); one inversion per 64 bases instead of per 256 costs ~5 % of a wave's time
  constexpr int blk = 64;
  const long quad_max = o.table_quad_max;   // moves the switch-over (tests reach both forms with small inputs)
  const int real = endo ? copies / 2 : copies;
  if (total <= quad_max && real - 1 <= 4 * TBQ_CHUNK) {   // a few rows: quad per base point
    const size_t lds = (2 * 64 + TBQ_CHUNK * 64) * sizeof(TF) + TBQ_CHUNK * 64 * sizeof(TJac);
    CPX_LAUNCH(k_table_build_quad, dim3((unsigned)((total + 15) / 16)), dim3(blk), lds, s, d_src, src_row_stride, d_table, rows, row_stride, npts, copy_stride, copies,
               endo ? 1 : 0, step_bits);
    return;
  }
  CPX_LAUNCH(k_table_build, dim3((unsigned)((total + blk - 1) / blk)), dim3(blk), 2 * blk * sizeof(TF), s, d_src, src_row_stride, d_table, rows, row_stride, npts,
                     copy_stride, copies, endo ? 1 : 0, d_tmp, step_bits);
}
void launch_finalize(const Jac* d_in, int n, Aff* d_aff, const uint32_t* d_dst_index, uint8_t* d_comp, hipStream_t s, const uint32_t* d_addend_index) {
  if (n <= 0) return;
  CPX_LAUNCH(k_finalize, dim3((n + 63) / 64), dim3(64), 2 * 64 * sizeof(Fp), s, d_in, n, d_aff, d_dst_index, d_comp, d_addend_index);
}
void launch_compress(const Aff* d_in, int n, int stride, int batch, uint8_t* d_out, hipStream_t s, int out_stride) {
  if (n <= 0 || batch <= 0) return;
  CPX_LAUNCH(k_compress, dim3((n + 255) / 256, batch), dim3(256), 0, s, d_in, n, stride, d_out, out_stride > 0 ? out_stride : n);
}
void launch_compress_cols(const Aff* d_in, const uint32_t* d_cols, int ncols, int stride, int batch, uint8_t* d_out, int out_stride, hipStream_t s) {
  if (ncols <= 0 || batch <= 0) return;
  CPX_LAUNCH(k_compress_cols, dim3(batch), dim3(64), 0, s, d_in, d_cols, ncols, stride, d_out, out_stride);
}
bool launch_smul(const SmulTask* d_tasks, int ntasks, int cnt, hipStream_t s, bool exclusive_simd, long quad_max) {
  const long total = (long)ntasks * cnt;
  if (total <= 0) return false;
  const size_t lds = 2 * SMUL_THREADS * sizeof(TF) + 20 * SMUL_THREADS * sizeof(uint32_t);
  const unsigned groups = (unsigned)((total + SMUL_THREADS - 1) / SMUL_THREADS);
  if (quad_max > 0 && total <= quad_max) {   // a small batch's T_2 commitments: a quad per element (never with SMUL_PLAIN tasks: the side stream's only)
    CPX_LAUNCH(k_smul_quad, dim3((unsigned)((total + 15) / 16)), dim3(64), SQ_LDS, s, d_tasks, ntasks, cnt);
    return true;
  }
  if (exclusive_simd && groups <= 16) CPX_LAUNCH(k_smul<true>, dim3(groups), dim3(SMUL_THREADS), lds, s, d_tasks, ntasks, cnt);
  else CPX_LAUNCH(k_smul<false>, dim3(groups), dim3(SMUL_THREADS), lds, s, d_tasks, ntasks, cnt);
  return false;
}
void launch_decompress(const Options& o, const uint8_t* d_in, int n, Aff* d_out, const uint32_t* d_dst_index, uint8_t* d_status, int check_subgroup, hipStream_t s,
                       const uint32_t* d_src_offset) {
  if (n <= 0) return;
  const long quad_max = o.decompress_quad_max;   // moves the switch-over (tests reach both forms with small inputs)
  if (n <= quad_max && check_subgroup) {   // a few points: quad per point
    CPX_LAUNCH(k_decompress_quad, dim3((n + 15) / 16), dim3(64), 16 * 3 * sizeof(TAcc), s, d_in, n, d_out, d_dst_index, d_status, check_subgroup, d_src_offset);
    return;
  }
  CPX_LAUNCH(k_decompress, dim3((n + 63) / 64), dim3(64), 0, s, d_in, n, d_out, d_dst_index, d_status, check_subgroup, d_src_offset);
}
void launch_ipa_round_scalars(const Fr* d_vec, int nproofs, int n, int half, const Fr* d_beta, Fr* d_out, hipStream_t s, int active) {
  if (nproofs > 0) CPX_LAUNCH(k_ipa_round_scalars, dim3(nproofs), dim3(128), 0, s, d_vec, n, active > 0 ? active : n, half, d_beta, d_out);
}
void launch_ipa_round_fold(Fr* d_vec, int nproofs, int n, int half, const Fr* d_gam, hipStream_t s, int active) {
  if (nproofs > 0) CPX_LAUNCH(k_ipa_round_fold, dim3(nproofs), dim3(128), 0, s, d_vec, n, active > 0 ? active : n, half, d_gam);
}
void launch_smsm_round_scalars(const Fr* d_vec, int nproofs, int n, int half, Fr* d_out, hipStream_t s, int active) {
  if (nproofs > 0) CPX_LAUNCH(k_smsm_round_scalars, dim3(nproofs), dim3(128), 0, s, d_vec, n, active > 0 ? active : n, half, d_out);
}
void launch_smsm_round_fold(Fr* d_vec, int nproofs, int n, int half, const Fr* d_gam, hipStream_t s, int active) {
  if (nproofs > 0) CPX_LAUNCH(k_smsm_round_fold, dim3(nproofs), dim3(128), 0, s, d_vec, n, active > 0 ? active : n, half, d_gam);
}
void launch_transcript_step1(const uint8_t* d_inst_comp, const uint8_t* d_m_comp, int nproofs, int ell, uint64_t* d_state, Fr* d_vec_a, hipStream_t s, bool lane_per_proof,
                             bool exclusive_simd) {
  if (nproofs <= 0) return;
  if (lane_per_proof) {
    CPX_LAUNCH(k_transcript_step1_lane, dim3((nproofs + 63) / 64), dim3(64), 0, s, d_inst_comp, d_m_comp, nproofs, ell, d_state, d_vec_a);
    return;
  }
  if (exclusive_simd) CPX_LAUNCH(k_transcript_step1<true>, dim3(nproofs), dim3(64), 0, s, d_inst_comp, d_m_comp, nproofs, ell, d_state, d_vec_a);
  else CPX_LAUNCH(k_transcript_step1<false>, dim3(nproofs), dim3(64), 0, s, d_inst_comp, d_m_comp, nproofs, ell, d_state, d_vec_a);
}
void launch_sum_jac(const Jac* d_in, int n, Jac* d_out, int* d_flag, hipStream_t s) { CPX_LAUNCH(k_sum_jac, dim3(1), dim3(64), 0, s, d_in, n, d_out, d_flag); }
void launch_bench_f28mul(Fp* d_data, int blocks, int iters, hipStream_t s) {
  CPX_LAUNCH(k_bench_f28mul, dim3(blocks), dim3(256), 0, s, d_data, iters);
}
void launch_bench_fpmul(Fp* d_data, int blocks, int iters, hipStream_t s) {
  CPX_LAUNCH(k_bench_fpmul, dim3(blocks), dim3(256), 0, s, d_data, iters);
}

}  // namespace cpx
