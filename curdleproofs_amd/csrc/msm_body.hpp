// The MSM wave bodies of the gfx950 kernels and what they share with the in-wave reductions — device code included by kernels.hip (the
// stand-alone MSM / reduction kernels) and round.hip (the fused log-round kernels: MSM waves that reduce their own accumulators and
// whose last arriver runs the round's finalisation, transcript step and Fr folds).
#pragma once
#include <hip/hip_runtime.h>
#include "g1.hpp"
#include "g1_28.hpp"
#include "g1_28_quad.hpp"
#include "quad_program.hpp"
#include "recode.hpp"
#include "glv.hpp"
#include "kernels.h"

namespace cpx {

// compressed encoding of a point to a 16-byte-aligned destination (every compressed-point buffer of the engine is: 48-byte records
// in hipMalloc'ed arrays): three 16-byte stores instead of 48 single-byte ones
__device__ __forceinline__ void aff_compress_store(const Aff& a, uint8_t* out) {
  uint32_t w[12];
  aff_compress_words(a, w);
  uint4* o = reinterpret_cast<uint4*>(out);
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
  o[2] = make_uint4(w[8], w[9], w[10], w[11]);
}

// ------------------------------------------------------------------ raw lane accumulators ("sets")
constexpr int ACC_WORDS = (int)(sizeof(TAcc) / 4);   // 56
constexpr int RAW_SET_WORDS = ACC_WORDS * 64;
__device__ __forceinline__ void raw_store(uint32_t* __restrict__ set, int lane, const TAcc& a) { reinterpret_cast<TAcc*>(set)[lane] = a; }
__device__ __forceinline__ TAcc raw_load(const uint32_t* __restrict__ set, int lane) { return reinterpret_cast<const TAcc*>(set)[lane]; }

// Small grids (a few proofs in flight: latency matters, not throughput): one WAVE per set and every point addition spread over the
// four lanes of a quad (g1_28_quad.hpp: 6 us instead of 18-20 us per dependent addition), 16 additions per wave and round.  The
// rounds of a set are a fixed PROGRAM of (operand, operand, destination) jobs over an array of points in LDS, one job per quad:
//   plain    (k_msm_fix):  the tree over 64 lanes, 32 + 16 + ... + 1 additions in 7 rounds.
//   weighted (k_msm_tblw): sum_l (l + 1) A_l with l = 8 a + b is 8 sum_a a R_a + sum_b (b + 1) C_b over the row sums R_a and the
//            column sums C_b of the 8 x 8 arrangement (three tree levels for both, 7 rounds); a weighted sum of EIGHT points is,
//            bit by bit of the weights, three sums of four points (2 rounds), so that seven points with weights 2^0 .. 2^6 remain
//            (2^6: the plain sum, for the upper half of the magnitudes): shifted side by side (<= 6 doubling rounds) and added in a
//            tree (3 rounds).  13 addition + 6 doubling rounds, ~105 us, against the 12 + 1 additions and 6 doublings of one lane
//            each (~310 us) of the scan + tree this replaces.
static __constant__ QuadProgram c_quad_prog[3] = {qp_plain(), qp_weighted(false), qp_weighted(true)};

// One round per iteration: quad q of the wave runs job(q) — the SAME code for every round, a few KB that stay in the
// instruction cache.  `dbl` must be uniform over the wave.
template <class JobFn> __device__ __forceinline__ void quad_exec(TAcc* buf, int nrounds, JobFn fn) {
  const int quad = threadIdx.x >> 2, sub = threadIdx.x & 3;
  for (int r = 0; r < nrounds; r++) {
    bool dbl = false;
    const QuadJob jb = fn(r, quad, dbl);
    TAcc res;
    if (dbl) res = xyzz28_dbl_quad(buf[jb.a]);
    else res = xyzz28_add_quad_mem(buf, jb.a, jb.b);
    if (jb.on && sub == 0) buf[jb.dst] = res;
    __syncthreads();
  }
}

// ------------------------------------------------------------------ table-backed MSM, barrier-free single-wave groups
// 32-copy tables (the CRS table, one-segment per-proof tables; the two-segment ones with 8 + 8 copies and two weight classes
// further down): every radix-256 window of a scalar has its own pre-shifted copy 2^(8c) P of the base, so ALL window
// sums carry weight 1 and a bucket may collect additions from any window: one (scalar, base) pair costs 32 mixed
// additions, the 128 bucket magnitudes of the signed digits are the only reduction.  (Radix 16 with 64 copies — the
// previous layout — paid 60 additions per pair.)
// A single-wave work-group owns WPW consecutive windows of one task and all 128 buckets, two per lane.  With a hit
// rate of 1/128 per (window, point) pair a lane cannot scan for its digits; the wave sorts instead (tbw_sort): every lane recodes
// one scalar of a 64-point slab, a histogram over the 128 magnitudes (LDS atomics) gives the list offsets, a second
// pass scatters 16-bit (point, window, sign) entries into per-bucket lists in LDS.  The buckets are then ranked by
// size and lane l takes rank l and rank 127 - l (longest with shortest): the lanes' totals differ by a few additions
// (random pairs: mean 64, slowest lane ~83).  Every lane walks its two lists in ONE loop — gather the pre-shifted
// point from the table in HBM/L2, add; at the boundary it parks the first accumulator in the raw-set buffer.
// A round takes as many slabs as fit the list (8704 entries = 256 points x 32 windows); later rounds of a longer task
// reload the parked accumulators (they are kept per bucket).  Waves never wait for each other and the CU scheduler
// backfills a finished wave's slot.  Output: two raw sets per wave (buckets 1..64, 65..128; k_reduce_sets turns them
// into two partial sums, k_finalize_ranges adds the partials of a request).
constexpr int TBW_WINDOWS = 32;       // radix-256 windows of a scalar < 2^255
constexpr int TBW_CAP = 8704;         // list entries per round
constexpr int TBW_ROUND_PTS = 1024;   // a list entry holds a 10-bit point index beside a 5-bit window and the sign ...
constexpr int TBW_ROUND_PTS_PERWIN = 4096;   // ... or, with one window per scalar half (PERWIN), a 14-bit one: a round takes TBW_CAP / 2 points
static_assert(2 * TBW_ROUND_PTS_PERWIN <= TBW_CAP, "two entries per point of a PERWIN round");
static_assert(TBW_CAP >= 64 * TBW_WINDOWS, "one slab always fits");

// The LDS of a wave's sort over NBINS bins: 128 (the bucket magnitudes) or 256 (weight class x magnitude, the two-segment tables below).
// The list offsets are not kept beside the cursors: after the scatter list b is [cur[b] - cnt[b], cur[b]).
template <int NBINS> struct TbwSort {
  static constexpr int LDS = TBW_CAP * 2 + 2 * NBINS * 4 + NBINS;
  uint16_t* list;     // [TBW_CAP]
  uint32_t* cnt;      // [NBINS] bin sizes of the round
  uint32_t* cur;      // [NBINS] scatter cursors
  uint8_t* order;     // [NBINS] bins by size
  uint32_t* dcache;   // [TBW_ROUND_PTS] a round's recoded digits, CACHE only
  __device__ __forceinline__ explicit TbwSort(uint8_t* smem)
      : list(reinterpret_cast<uint16_t*>(smem)), cnt(reinterpret_cast<uint32_t*>(smem + TBW_CAP * 2)), cur(cnt + NBINS),
        order(reinterpret_cast<uint8_t*>(cur + NBINS)), dcache(reinterpret_cast<uint32_t*>(smem + LDS)) {}
  __device__ __forceinline__ uint32_t start(uint32_t b) const { return cur[b] - cnt[b]; }
};
constexpr int TBW_LDS = TbwSort<128>::LDS;                   // 18 560 B
constexpr int TBW_LDS_CACHE = TBW_LDS + TBW_ROUND_PTS * 4;   // k_msm_tblw<2, false> keeps a round's recoded digits (tbw_sort)
constexpr int TBW2_LDS = TbwSort<256>::LDS;                  // 19 712 B
static_assert(TBW_LDS <= 20480 && TBW2_LDS <= 20480, "eight single-wave groups per CU share 160 KiB of LDS");

__device__ __forceinline__ const TAff* tbl_point(const TblTask& t, uint32_t g, uint32_t copy) {
  const uint32_t n0 = t.seg[0].n;
  const TblSeg& sg = (g < n0) ? t.seg[0] : t.seg[1];
  const uint32_t i = (g < n0) ? g : g - n0;
  return sg.base + (size_t)copy * sg.copy_stride + (sg.idx ? sg.idx[i] : i);
}

// Signed radix-256 digits of windows [w0, w0 + WPW) of scalar i, biased by 128 and packed four per word.  The scalar
// is split by the endomorphism first (glv.hpp): k = +-(+-|t| + q z^2), windows 0..15 are the digits of |t| (table copies
// 2^(8c) P), windows 16..31 those of q (table copies -phi(2^(8c) P) = z^2 2^(8c) P); sg_lo / sg_hi are the signs the
// two halves carry.
template <int WPW, bool PERWIN> __device__ __forceinline__ void tbw_digits(const TblTask& task, uint32_t i, int w0, uint32_t (&dg)[(WPW + 3) / 4],
                                                                           uint32_t& sg_lo, uint32_t& sg_hi) {
  if (PERWIN && task.digits) {   // recoded once per task by k_to_table_endo
    const uint32_t* dgs = task.digits + 9 * (size_t)i;
    const uint32_t bt = dgs[w0 >> 2], bq = dgs[4 + (w0 >> 2)], sg = dgs[8];
    dg[0] = ((bt >> (8 * (w0 & 3))) & 255u) | (((bq >> (8 * (w0 & 3))) & 255u) << 8);
    sg_lo = sg & 1u;
    sg_hi = sg >> 1;
    return;
  }
  Fr k = task.scalars[i];
  if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
  uint32_t t[4], q[4], bytes[8], nk, nt;
  glv_split(k.v, t, q, nk, nt);
  glv_biased_bytes(t, bytes);
  glv_biased_bytes(q, bytes + 4);
  sg_lo = nk ^ nt;
  sg_hi = nk;
  if (PERWIN) {   // w0 = the window: its digit of |t| (entry j = 0) and of q (j = 1)
    uint32_t bt = 0, bq = 0;
    CPX_UNROLL for (int w = 0; w < 4; w++) {
      if (w == (w0 >> 2)) {
        bt = bytes[w];
        bq = bytes[4 + w];
      }
    }
    dg[0] = ((bt >> (8 * (w0 & 3))) & 255u) | (((bq >> (8 * (w0 & 3))) & 255u) << 8);
    return;
  }
  CPX_UNROLL for (int w = 0; w < 8; w++) {
    CPX_UNROLL for (int x = 0; x < (WPW + 3) / 4; x++)
      if (w == (w0 >> 2) + x) dg[x] = bytes[w];
  }
  if (WPW < 4) dg[0] >>= 8 * (w0 & 3);
}
// bucket |d| - 1 of window j's digit, or >= 128 for a zero digit
__device__ __forceinline__ uint32_t tbw_bucket(uint32_t word, int j, uint32_t& neg) {
  const int d = (int)((word >> (8 * (j & 3))) & 255u) - 128;
  neg = d < 0 ? 1u : 0u;
  return (uint32_t)((d < 0 ? -d : d) - 1);   // digit 0 -> 0xffffffff
}
// bin of window j's digit, or >= NBINS for a zero digit: the bucket, or with 256 bins weight class x bucket (a wave of both classes
// starts at a multiple of 16 windows, so the class of window w0 + j is bit 3 of j)
template <int NBINS> __device__ __forceinline__ uint32_t tbw_bin(uint32_t word, int j, uint32_t& neg) {
  const uint32_t b = tbw_bucket(word, j, neg);
  if constexpr (NBINS == 128) return b;
  else return b < 128u ? b + 128u * (uint32_t)((j >> 3) & 1) : (uint32_t)NBINS;
}
// list entry: (point index inside the round << ESH) | (window j << 1) | sign.  PERWIN has j < 2, so 14 bits of point index fit: the
// verifier's 1112 points per proof are ONE round instead of 1024 + 88 (the short second round cost a tenth of the kernel: its lists of
// 0 - 6 entries wait for the longest, and the histogram, ranking and parking are paid again)
template <bool PERWIN> struct TbwEntry {
  static constexpr int ESH = PERWIN ? 2 : 6;
  static constexpr uint32_t EJM = PERWIN ? 1u : 31u;
  static constexpr uint32_t ROUND_PTS = PERWIN ? (uint32_t)TBW_ROUND_PTS_PERWIN : (uint32_t)TBW_ROUND_PTS;
};

// The sort of one round, by the whole wave: the points [next, end) of the task — as many 64-point slabs from `next` on as fit the
// list — with their digits of windows [w0, w0 + WPW) sorted into the NBINS lists of ts.  On return (behind a barrier) cnt[b] is the
// size of list b, ts.start(b) its offset, and order[] holds the bins by size.  Returns end.
// CACHE (the latency form: two windows per wave, a lone proof): the split + recoding of a scalar (~700 instructions) is done in the
// histogram pass and kept for the scatter pass (one word per point); the other forms recompute it (2 x per 4-32 windows: < 1 %
// of their additions, and 4 KB more LDS per wave would cost them the second wave per SIMD).
template <int WPW, bool PERWIN, int NBINS, bool CACHE>
__device__ __forceinline__ uint32_t tbw_sort(const TbwSort<NBINS>& ts, const TblTask& task, int w0, uint32_t next, uint32_t ntot) {
  constexpr int NW = (WPW + 3) / 4, K = NBINS / 64;   // K bins per lane
  typedef TbwEntry<PERWIN> E;
  const int lane = threadIdx.x;
  CPX_UNROLL for (int k = 0; k < K; k++) ts.cnt[64 * k + lane] = 0;
  __syncthreads();
  // histogram over as many 64-point slabs as fit the list
  uint32_t total = 0, end = next;
  while (end < ntot && end - next + 64 <= E::ROUND_PTS) {
    const uint32_t i = end + lane;
    uint32_t dg[NW], sg_lo, sg_hi;
    int mine = 0;
    if (i < ntot) {
      tbw_digits<WPW, PERWIN>(task, i, w0, dg, sg_lo, sg_hi);
      if (CACHE) ts.dcache[i - next] = (dg[0] & 0xffffu) | (sg_lo << 16) | (sg_hi << 17);
      CPX_UNROLL for (int j = 0; j < WPW; j++) {
        uint32_t neg;
        mine += tbw_bucket(dg[j >> 2], j, neg) < 128u ? 1 : 0;
      }
    }
    int ct = mine;
    CPX_UNROLL for (int m = 32; m >= 1; m >>= 1) ct += __shfl_xor(ct, m, 64);
    if (total && total + (uint32_t)ct > (uint32_t)TBW_CAP) break;
    if (i < ntot) {
      CPX_UNROLL for (int j = 0; j < WPW; j++) {
        uint32_t neg;
        const uint32_t b = tbw_bin<NBINS>(dg[j >> 2], j, neg);
        if (b < (uint32_t)NBINS) atomicAdd(&ts.cnt[b], 1u);
      }
    }
    total += (uint32_t)ct;
    end = min(end + 64, ntot);
  }
  __syncthreads();
  // list offsets: exclusive scan of the bin sizes over the wave (lane l scans bins K l .. K l + K - 1)
  {
    uint32_t a[K], sum = 0;
    CPX_UNROLL for (int k = 0; k < K; k++) {
      a[k] = ts.cnt[K * lane + k];
      sum += a[k];
    }
    uint32_t incl = sum;
    CPX_UNROLL for (int d = 1; d < 64; d <<= 1) {
      const uint32_t y = (uint32_t)__shfl_up((int)incl, d, 64);
      if (lane >= d) incl += y;
    }
    uint32_t o = incl - sum;
    CPX_UNROLL for (int k = 0; k < K; k++) {
      ts.cur[K * lane + k] = o;
      o += a[k];
    }
    // the bins ranked by size: a lane adds up rank l and rank 127 - l of them (longest with shortest), so the lanes' totals differ
    // by a few additions instead of +-30 %
    uint32_t r[K];
    CPX_UNROLL for (int k = 0; k < K; k++) r[k] = 0;
    for (int q = 0; q < NBINS; q++) {
      const uint32_t c = ts.cnt[q];
      CPX_UNROLL for (int k = 0; k < K; k++) r[k] += (c < a[k] || (c == a[k] && q < K * lane + k)) ? 1u : 0u;
    }
    CPX_UNROLL for (int k = 0; k < K; k++) ts.order[r[k]] = (uint8_t)(K * lane + k);
  }
  __syncthreads();
  for (uint32_t s0 = next; s0 < end; s0 += 64) {
    const uint32_t i = s0 + lane;
    if (i < end) {
      uint32_t dg[NW], sg_lo, sg_hi;
      if (CACHE) {
        const uint32_t v = ts.dcache[i - next];
        dg[0] = v & 0xffffu;
        sg_lo = (v >> 16) & 1u;
        sg_hi = (v >> 17) & 1u;
      } else {
        tbw_digits<WPW, PERWIN>(task, i, w0, dg, sg_lo, sg_hi);
      }
      CPX_UNROLL for (int j = 0; j < WPW; j++) {
        uint32_t neg;
        const uint32_t b = tbw_bin<NBINS>(dg[j >> 2], j, neg);
        neg ^= (PERWIN ? j == 0 : w0 + j < 16) ? sg_lo : sg_hi;
        if (b < (uint32_t)NBINS) ts.list[atomicAdd(&ts.cur[b], 1u)] = (uint16_t)(((i - next) << E::ESH) | ((uint32_t)j << 1) | neg);
      }
    }
  }
  __syncthreads();
  return end;
}

// ONE loop over the lane's NSEG lists: a wave runs a loop until its slowest lane is through, so only inside one loop do a lane's long
// and short lists add up (two loops, one per task of a pair, each waited for the longest pair of buckets of the wave, whoever walked
// it; the same loop in the one-task kernels measured 0.4 % slower than the two-list loop of msm_tblw_body).  Segment sg walks list
// bin(sg) into the accumulator at position bin % 64 of raw set set(sg, bin), reading the point src(sg, entry) for every entry; a
// segment that ends parks its accumulator and loads (or, in the first round of a task, zeroes) the next one.
template <int NSEG, int NBINS, class BinFn, class SetFn, class SrcFn>
__device__ __forceinline__ void tbw_walk_lists(const TbwSort<NBINS>& ts, uint32_t* __restrict__ raw0, bool later, BinFn bin, SetFn set, SrcFn src) {
  uint32_t nwalk = 0;   // entries of all the lane's lists
  CPX_UNROLL for (int s = 0; s < NSEG; s++) nwalk += ts.cnt[bin(s)];
  int sg = 0;
  uint32_t bk, cs, st, kin;
  uint32_t* rb;
  TAcc xacc;
  auto enter = [&]() {
    bk = bin(sg);
    cs = ts.cnt[bk];
    st = ts.start(bk);
    kin = 0;
    rb = raw0 + set(sg, bk) * RAW_SET_WORDS;
    xacc = later ? raw_load(rb, bk & 63) : TAcc::identity();
  };
  auto next_segment = [&]() {
    raw_store(rb, bk & 63, xacc);
    sg++;
    enter();
  };
  enter();
#pragma unroll 1
  for (uint32_t k = 0; k < nwalk; k++) {
    while (kin == cs) next_segment();   // (sg stays below NSEG: entries remain)
    const uint32_t e = ts.list[st + kin];
    const TAff q = *src(sg, e);
    xacc = t_acc_add_mixed_inl(xacc, t_cneg_lazy(q, (e & 1u) != 0));   // products inlined: no argument moves, no scratch
    kin++;
  }
  while (sg + 1 < NSEG) next_segment();   // the lists that were empty or remain: every bin of the round is written
  raw_store(rb, bk & 63, xacc);
}

// PERWIN (k_msm_tblw<2, true>): the same wave over bases WITHOUT shifted copies (the verifier's per-proof points, used once):
// the "table" has two copies, P and -phi(P) (k_to_table_endo), wave w of a task takes digit w of |t| and of q, and the
// 16 window results carry the weights 2^(8w) (Horner tail, k_msm_tail).
// PAIR (with PERWIN; the prover's R = <a, vec_R>, S = <a, vec_S>): tasks 2 t and 2 t + 1 have the SAME scalars, hence the same digits
// and the same sorted bucket lists — one wave serves both, walking its lists once per task: the fixed cost of a wave (digit load,
// histogram, ranking, scatter: as much as a dozen additions) is paid once for 16 instead of 8 additions per lane.  Four raw sets
// per wave: [task 2 t lower | upper | task 2 t + 1 lower | upper].
// SEGS = 2 (every segment of the task a two-segment per-proof table: kernels.h): the tables hold 8 + 8 copies, windows 8..15 of a half
// read the same copies as windows 0..7 (tbl_window(w, 8).copy) and their sums carry the weight 2^64.  A wave of up to 8 windows lies
// inside one weight class and differs from the one-segment wave only in the copy it reads and in its partial slots.  A wave of 16 or 32
// windows serves BOTH classes: ONE histogram over 256 bins (class x magnitude), the bins ranked by size, lane l walks the lists of rank
// l, 127 - l, 128 + l and 255 - l (longest with shortest, twice) in one loop.  Four raw sets per wave — bin b lives in set b / 64:
// [class 0 lower | upper | class 1 lower | upper].  The partial slots of either (recode.hpp tbw_part_slot): class 1 first.
template <int WPW, bool PERWIN, bool PAIR = false, int SEGS = 1> __device__ __forceinline__ void msm_tblw_body(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw,
                                                                                                             uint32_t* __restrict__ raw_slot, int slices, const uint32_t bid) {
  static_assert(!PERWIN || WPW == 2, "one window of each half per wave");
  static_assert(!PAIR || PERWIN, "pairs only for the one-off MSMs");
  static_assert(SEGS == 1 || (SEGS == 2 && !PERWIN), "two-segment tables have shifted copies");
  constexpr bool BOTH = SEGS == 2 && WPW >= 16;   // both weight classes in one wave
  constexpr int NBINS = BOTH ? 256 : 128;
  constexpr int NSETS = (PAIR || BOTH) ? 4 : 2;
  constexpr int WV = PERWIN ? 16 : TBW_WINDOWS / WPW;   // waves per task
  typedef TbwEntry<PERWIN> E;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const TbwSort<NBINS> ts(smem);
  // a few tasks in flight (latency matters): `slices` waves share a task's points (each its own 64-aligned range and raw sets), so
  // that a lane's chain of additions is a quarter as long; slices = 1 otherwise
  const uint32_t tidx = (PAIR ? 2u : 1u) * (bid / (WV * slices));
  const TblTask task = tasks[tidx];
  TblTask task2 = task;   // the second task of a pair: other bases, other partial-sum slots
  if (PAIR) {
    task2.seg[0].base = tasks[tidx + 1].seg[0].base;
    task2.pad = tasks[tidx + 1].pad;
  }
  const int wv = (bid / slices) % WV, w0 = PERWIN ? wv : wv * WPW, slice = bid % slices;
  const int lane = threadIdx.x;
  const uint32_t nall = task.seg[0].n + task.seg[1].n, per = ((nall + slices - 1) / slices + 63) & ~63u;
  const uint32_t first = min(nall, (uint32_t)slice * per), ntot = min(nall, first + per);
  uint32_t* raw0 = raw + (size_t)bid * NSETS * RAW_SET_WORDS;
  if (lane < NSETS)   // pad = first partial slot of the task; a pair's sets 2, 3 are sets 0, 1 of its second task
    raw_slot[bid * NSETS + lane] = ((PAIR && lane >= 2) ? task2.pad : task.pad) + tbw_part_slot(WPW, SEGS, WV, slices, wv, slice, PAIR ? lane & 1 : lane);
  // the table copy that entry e reads
  auto copy_of = [&](uint32_t e) {
    const uint32_t w = (PERWIN ? 0u : (uint32_t)w0) + ((e >> 1) & E::EJM);
    return SEGS == 2 ? tbl_window(w, 8).copy : w;
  };

  uint32_t next = first;
  bool later = false;   // a later round: the accumulators are parked in the raw sets
  do {
    const uint32_t end = tbw_sort<WPW, PERWIN, NBINS, WPW == 2 && !PERWIN>(ts, task, w0, next, ntot);
    if constexpr (BOTH) {
      tbw_walk_lists<4>(
          ts, raw0, later, [&](int sg) { return (uint32_t)ts.order[sg == 0 ? lane : sg == 1 ? 127 - lane : sg == 2 ? 128 + lane : 255 - lane]; },
          [&](int, uint32_t bin) { return bin >> 6; }, [&](int, uint32_t e) { return tbl_point(task, next + (e >> E::ESH), copy_of(e)); });
    } else if constexpr (PAIR) {
      // both tasks have the same lists, so a lane that walked its own bucket pair twice carried twice its imbalance (252 points: the
      // longest pair 10.2 entries against a mean of 7.8).  The second task's walk takes the bucket pair of ANOTHER lane instead: the lanes are
      // ranked by the size of their pair and lane of rank r takes the pair of rank 63 - r (the buckets are parked by bucket index, whoever adds
      // them up): the two walks of a lane sum to about twice the mean
      const uint32_t mine = ts.cnt[ts.order[lane]] + ts.cnt[ts.order[127 - lane]];
      uint32_t rk = 0;
      for (int q = 0; q < 64; q++) {
        const uint32_t o = (uint32_t)__shfl((int)mine, q, 64);
        rk += (o < mine || (o == mine && q < lane)) ? 1u : 0u;
      }
      // lane of rank 63 - rk: every lane publishes its rank, the partner is found by a second sweep
      int partner = lane;
      for (int q = 0; q < 64; q++) {
        const uint32_t o = (uint32_t)__shfl((int)rk, q, 64);
        if (o == 63u - rk) partner = q;
      }
      const ptrdiff_t base2 = task2.seg[0].base - task.seg[0].base;   // (a pair's tasks differ in their bases only)
      // own, own, partner, partner; bucket b lives in set b / 64 (+ 2 for the second task) at position b % 64
      tbw_walk_lists<4>(
          ts, raw0, later, [&](int sg) { return (uint32_t)ts.order[(sg & 1) ? 127 - (sg >= 2 ? partner : lane) : (sg >= 2 ? partner : lane)]; },
          [&](int sg, uint32_t bin) { return 2 * (uint32_t)(sg >> 1) + (bin >> 6); },
          [&](int sg, uint32_t e) { return tbl_point(task, next + (e >> E::ESH), copy_of(e)) + (sg >= 2 ? base2 : 0); });
    } else {
      // every lane walks its two lists in one loop; at the boundary it parks the first accumulator (by bucket index)
      const uint32_t b0 = ts.order[lane], b1 = ts.order[127 - lane];
      const uint32_t c0 = ts.cnt[b0], c1 = ts.cnt[b1], s0_ = ts.start(b0), s1_ = ts.start(b1);
      uint32_t* const rb0 = raw0 + (b0 >> 6) * RAW_SET_WORDS;   // bucket b lives in set b / 64 at position b % 64
      uint32_t* const rb1 = raw0 + (b1 >> 6) * RAW_SET_WORDS;
      TAcc xacc = later ? raw_load(rb0, b0 & 63) : TAcc::identity();
      const uint32_t cboth = c0 + c1;
      for (uint32_t k = 0; k < cboth; k++) {
        if (k == c0) {   // first bucket done: park it, go on with the second
          raw_store(rb0, b0 & 63, xacc);
          xacc = later ? raw_load(rb1, b1 & 63) : TAcc::identity();
        }
        const uint32_t e = ts.list[k < c0 ? s0_ + k : s1_ + (k - c0)];
        const TAff q = *tbl_point(task, next + (e >> E::ESH), copy_of(e));
        xacc = t_acc_add_mixed_inl(xacc, t_cneg_lazy(q, (e & 1u) != 0));   // products inlined: no argument moves, no scratch (profiles/r11_bucket_wave.md)
      }
      if (c1 == 0) {
        raw_store(rb0, b0 & 63, xacc);
        xacc = later ? raw_load(rb1, b1 & 63) : TAcc::identity();
      }
      raw_store(rb1, b1 & 63, xacc);
    }
    __syncthreads();
    next = end;
    later = true;
  } while (next < ntot);
}

// ------------------------------------------------------------------ fixed-base MSM over multiples tables
constexpr int FIX_CHUNK = 256;

// signed radix-2^c digits of a canonical scalar (recode.hpp); writes the NW digits of windows [w0, w0+NW).  Digits in
// [-2^(c-1), 2^(c-1) - 1]: |d| indexes the table, -2^15 still fits int16_t; 19-bit digits need 32 bits
template <int CB> struct FixDigit { typedef int16_t type; };
template <> struct FixDigit<19> { typedef int32_t type; };
template <int CB, int NW> __device__ __forceinline__ void fix_digits(const uint32_t* k, int w0, typename FixDigit<CB>::type* out, int stride) {
  fix_window_digits<CB, NW>(k, w0, out, stride);   // recode.hpp (host + device: checked on the CPU by tests/test_host_emul.py)
}
// One wave = FIX_WPW windows x (64 / FIX_WPW) point slices of one task.  16 windows per wave (a whole radix-2^16
// task) keeps the fixed 6-step tree reduction small against the per-lane additions (n/4 per lane); 8 windows
// per wave double the number of waves when the launch would not fill the GPU otherwise.
template <int CB, int FIX_WPW> __device__ __forceinline__ void msm_fix_body(const FixTask* __restrict__ tasks, const TFix* __restrict__ tab, int nc,
                                                                          uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot, const uint32_t bid) {
  constexpr int W = (256 + CB - 1) / CB, WG = W / FIX_WPW;    // waves per task
  constexpr int LPW = 64 / FIX_WPW;                // lanes (point slices) per window (CB = 19: 7 windows x 9 slices, lane 63 idles)
  constexpr uint32_t M = 1u << (CB - 1);
  static_assert(W % FIX_WPW == 0, "whole waves per task");
  typedef typename FixDigit<CB>::type DT;
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  DT* digits = reinterpret_cast<DT*>(smem);   // [FIX_WPW][FIX_CHUNK]
  const FixTask task = tasks[bid / WG];
  const int wg = bid % WG;
  const int lane = threadIdx.x;
  const bool working = lane < FIX_WPW * LPW;
  const int wl = working ? lane / LPW : 0, sl = lane % LPW;
  const uint32_t w = (uint32_t)(wg * FIX_WPW + wl);
  const TFix* wtab = tab + (size_t)w * M * nc;
  TAcc xacc = TAcc::identity();

  for (uint32_t base = 0; base < task.n; base += FIX_CHUNK) {
    const int m = min((uint32_t)FIX_CHUNK, task.n - base);
    __syncthreads();
    for (int t = lane; t < m; t += 64) {
      Fr k = task.scalars[base + t];
      if (!(task.flags & MSM_SCALARS_CANONICAL)) k = fe_from_mont(k);
      fix_digits<CB, FIX_WPW>(k.v, wg * FIX_WPW, digits + t, FIX_CHUNK);
    }
    __syncthreads();
    const DT* row = digits + wl * FIX_CHUNK;
    // every lane walks its slice i = sl, sl+LPW, ...: same trip count for all lanes; the gather of the next point is in
    // flight while the current one is added (products inlined)
    auto fetch = [&](int i, int& d) {
      d = (i < m && working) ? row[i] : 0;
      const uint32_t g = base + i;
      return d ? wtab[(size_t)((d < 0 ? -d : d) - 1) * nc + task.off + (task.idx ? task.idx[g] : g)].a : TAff::identity();
    };
    int dn;
    TAff pn = fetch(sl, dn);
    for (int i = sl; i < m; i += LPW) {
      const int d = dn;
      const TAff p = pn;
      pn = fetch(i + LPW, dn);
      if (d) xacc = t_acc_add_mixed_inl(xacc, t_cneg_lazy(p, d < 0));
    }
  }
  // all entries carry weight 1: the wave's 64 accumulators form one plain raw set (k_reduce_sets adds them up)
  raw_store(raw + (size_t)bid * RAW_SET_WORDS, lane, xacc);
  if (lane == 0) raw_slot[bid] = task.out_first + wg;
}
}  // namespace cpx
