// Planner of a table-backed MSM phase — host code without a HIP call: turns a list of requests into the task descriptors of
// k_msm_fix (CRS segments) and k_msm_tblw (per-proof segments) and the per-request ranges k_finalize_ranges adds up.  One definition
// for the host-driven phases (Engine::run_tbl_phase, the table stream of batch_prove_tables) and the device-resident plans
// (Engine::build_plan); tests/test_tbl_plan_cpu.py compiles it for the CPU.  WHICH requests the protocol makes is written down in
// prove_reqs.hpp; Engine::make_reqs turns those descriptors into the TblReq below.
#pragma once
#include <algorithm>
#include <vector>
#include "host_math.hpp"
#include "kernels.h"

namespace cpx {

// table-backed MSM request: up to two base segments, each with its own host scalar vector
struct TblReq {
  TblSeg seg0;
  const host::S* s0;
  TblSeg seg1;
  const host::S* s1;
  uint32_t dst = ~0u;       // optional: index into d_pp_ receiving the affine result
  const Fr* dev = nullptr;  // optional: the seg0.n + seg1.n scalars already sit in device memory (s0 / s1 unused)
  uint32_t add[3] = {~0u, ~0u, ~0u};   // optional: d_pp_ indices of affine points of earlier phases added with coefficient 1
};

// The shifted CRS copies [lo, hi): a segment inside them has a fixed-base table of multiples and goes to k_msm_fix.  lo == nullptr
// (no table of multiples): every request, also an empty one, is one task of k_msm_tblw.
struct CrsRange {
  const TAff* lo = nullptr;
  const TAff* hi = nullptr;
  bool is_crs(const TblSeg& sg) const { return lo && sg.n && sg.base >= lo && sg.base < hi; }
  bool needs_tbl(const TblReq& r) const { return !lo || (r.seg0.n && !is_crs(r.seg0)) || (r.seg1.n && !is_crs(r.seg1)); }
};

// What the launches of a phase need to know besides the arrays
struct TblShape {
  size_t nt = 0, ntt = 0, nft = 0;   // requests, tasks of k_msm_tblw, tasks of k_msm_fix
  size_t nscal = 0;                  // scalars of the requests without TblReq::dev: what the caller stages
  uint32_t tbl_max_n = 0;            // points of the largest task of k_msm_tblw
  size_t nparts = 0, fix_sets = 0, tbl_sets = 0;   // partial sums; raw sets [fixed-base waves | bucket sets of the table waves]
  int fix_wpw = 16, tbl_wpw = 32, tbl_slices = 1;
  int tbl_segments = 1;      // 2: the table tasks read two-segment per-proof tables (kernels.h) and leave their weight-2^64 partials first
  double pts_fix = 0, pts_tbl = 0;
  bool any_add = false;
  bool has_comp = false;     // the per-request arrays carry a compressed-bytes slot
  bool one_launch = false;   // both MSM kernels in ONE launch (launch_msm_fix_tblw)
  // the per-request arrays: first partial | partial count | affine destination | [compressed-bytes slot] | addends[3]
  size_t meta_words() const { return (has_comp ? 7 : 6) * nt; }
  size_t add_offset() const { return (has_comp ? 4 : 3) * nt; }
};

// First pass: the counts that decide the windows per wave, the slices and the size of the arrays
inline void tbl_count(const std::vector<TblReq>& reqs, const CrsRange& crs, TblShape& sh) {
  sh.nt = reqs.size();
  sh.ntt = sh.nft = sh.nscal = 0;
  sh.tbl_max_n = 0;
  for (const TblReq& r : reqs) {
    const bool f0 = crs.is_crs(r.seg0), f1 = crs.is_crs(r.seg1);
    sh.nft += (f0 ? 1 : 0) + (f1 ? 1 : 0);
    if (!r.dev) sh.nscal += r.seg0.n + r.seg1.n;
    if (!crs.needs_tbl(r)) continue;
    sh.ntt++;
    sh.tbl_max_n = std::max(sh.tbl_max_n, (f0 ? 0u : r.seg0.n) + (f1 ? 0u : r.seg1.n));
  }
}

// Second pass: tt[sh.ntt], ft[sh.nft] and meta[sh.meta_words()] in request order; a request's partial sums are the table task's
// tbl_parts followed by fix_parts per fixed-base task.  The scalars of a request are at TblReq::dev or, without one, at
// scal + soff[i] of the blob the caller uploads (soff: optional, nt offsets in Fr units, seg0 then seg1 per request).  Requests
// without a destination scatter to dummy_dst; comp_index (optional): the compressed-bytes slot of every request.
// tbl_hi (two-segment per-proof tables, kernels.h): how many of a table task's tbl_parts, the first ones, carry the weight 2^64 — recorded
// in the upper 16 bits of the request's partial count.
inline void tbl_plan(const std::vector<TblReq>& reqs, const CrsRange& crs, uint32_t fix_parts, uint32_t tbl_parts, uint32_t dummy_dst, const Fr* scal,
                     const uint32_t* comp_index, TblShape& sh, TblTask* tt, FixTask* ft, uint32_t* meta, size_t* soff = nullptr, uint32_t tbl_hi = 0) {
  const size_t nt = reqs.size();
  const TblSeg none{nullptr, nullptr, 0, 0};
  sh.has_comp = comp_index != nullptr;
  sh.any_add = false;
  sh.pts_fix = sh.pts_tbl = 0;
  size_t it = 0, jf = 0, nparts = 0, off = 0;
  for (size_t i = 0; i < nt; i++) {
    const TblReq& r = reqs[i];
    const Fr* sbase = r.dev ? r.dev : scal + off;   // where this request's scalars are (or will be) on the device
    if (soff) soff[i] = off;
    if (!r.dev) off += r.seg0.n + r.seg1.n;
    const bool f0 = crs.is_crs(r.seg0), f1 = crs.is_crs(r.seg1);
    const uint32_t first = (uint32_t)nparts;
    uint32_t hi = 0;
    if (crs.needs_tbl(r)) {
      hi = tbl_hi;
      TblTask t;
      t.seg[0] = r.seg0;
      t.seg[1] = f1 ? none : r.seg1;
      t.scalars = sbase;
      if (f0) {   // seg0 goes to the fixed-base kernel: its scalars are skipped, seg1 becomes the only segment
        t.seg[0] = f1 ? none : r.seg1;
        t.seg[1] = none;
        t.scalars = sbase + r.seg0.n;
      }
      t.flags = 0;
      t.pad = (uint32_t)nparts;
      t.digits = nullptr;
      tt[it++] = t;
      nparts += tbl_parts;
    }
    if (f0) {
      ft[jf++] = FixTask{r.seg0.idx, sbase, (uint32_t)(r.seg0.base - crs.lo), r.seg0.n, 0, (uint32_t)nparts};
      nparts += fix_parts;
    }
    if (f1) {
      ft[jf++] = FixTask{r.seg1.idx, sbase + r.seg0.n, (uint32_t)(r.seg1.base - crs.lo), r.seg1.n, 0, (uint32_t)nparts};
      nparts += fix_parts;
    }
    meta[i] = first;
    meta[nt + i] = ((uint32_t)nparts - first) | (hi << 16);
    meta[2 * nt + i] = r.dst != ~0u ? r.dst : dummy_dst;
    if (comp_index) meta[3 * nt + i] = comp_index[i];
    for (int j = 0; j < 3; j++) meta[sh.add_offset() + 3 * i + j] = r.add[j];
    sh.any_add |= r.add[0] != ~0u;
    sh.pts_fix += (f0 ? r.seg0.n : 0) + (f1 ? r.seg1.n : 0);
    sh.pts_tbl += (f0 ? 0 : r.seg0.n) + (f1 ? 0 : r.seg1.n);
  }
  sh.nparts = nparts;
  sh.fix_sets = sh.nft * fix_parts;
  sh.tbl_sets = sh.ntt * tbl_parts;
}

}  // namespace cpx
