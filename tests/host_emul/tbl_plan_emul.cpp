// TEST-ONLY: the planner of a table-backed MSM phase (curdleproofs_amd/csrc/tbl_plan.hpp) compiled for the CPU.  The planner only
// compares and offsets base pointers, so the "device" buffers here are plain host arrays that nothing dereferences.
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/tbl_plan.hpp"

using namespace cpx;

// desc: per request {kind0, n0, kind1, n1, addend, dst}; kind 0 = no segment, 1 = a column range of the CRS copies, 2 = a per-proof table.
// counts: nt ntt nft nparts fix_sets tbl_sets nscal tbl_max_n any_add pts_fix pts_tbl.  tt: per table task {slot, scalar offset, seg0.n, seg1.n};
// ft: per fixed-base task {slot, scalar offset, column, n}; meta: first | count | dst | addends[3]; soff: scalar offset per request.
// Returns 0, or 1 when the device form (every request with TblReq::dev at the same place of the blob, a compressed-bytes slot per
// request) differs from the host form before sorting.
extern "C" int emul_tbl_plan(int nreq, const uint32_t* desc, int fix, uint32_t fix_parts, uint32_t tbl_parts, uint32_t dummy_dst, uint64_t* counts, uint64_t* tt_out,
                             uint64_t* ft_out, uint32_t* meta_out, uint64_t* soff_out) {
  const uint32_t NC = 300, NP = 600;
  std::vector<TAff> ctab(32 * NC), ptab((size_t)32 * NP * 4);
  std::vector<host::S> hscal(1);
  std::vector<TblReq> reqs(nreq);
  size_t total = 0;
  for (int i = 0; i < nreq; i++) {
    const uint32_t* d = desc + 6 * i;
    auto seg = [&](uint32_t kind, uint32_t n, int which) {
      if (!kind) return TblSeg{nullptr, nullptr, 0, 0};
      if (kind == 1) return TblSeg{ctab.data() + (i % 7) + which, nullptr, NC, n};   // (CRS columns start at i % 7 + which: FixTask::off)
      return TblSeg{ptab.data() + (size_t)(i % 4) * 32 * NP + which * 256, nullptr, NP, n};
    };
    reqs[i] = TblReq{seg(d[0], d[1], 0), hscal.data(), seg(d[2], d[3], 1), hscal.data()};
    if (d[4]) reqs[i].add[0] = 1000 + i;
    if (d[5]) reqs[i].dst = 2000 + i;
    total += d[1] + d[3];
  }
  std::vector<Fr> blob(total + 1);
  const CrsRange crs{fix ? ctab.data() : nullptr, fix ? ctab.data() + ctab.size() : nullptr};
  TblShape sh;
  tbl_count(reqs, crs, sh);
  std::vector<TblTask> tt(sh.ntt + 1);
  std::vector<FixTask> ft(sh.nft + 1);
  std::vector<uint32_t> meta(6 * nreq + 1);
  std::vector<size_t> soff(nreq + 1);
  tbl_plan(reqs, crs, fix_parts, tbl_parts, dummy_dst, blob.data(), nullptr, sh, tt.data(), ft.data(), meta.data(), soff.data());
  const uint64_t c[11] = {sh.nt, sh.ntt, sh.nft, sh.nparts, sh.fix_sets, sh.tbl_sets, sh.nscal, sh.tbl_max_n, sh.any_add, (uint64_t)sh.pts_fix, (uint64_t)sh.pts_tbl};
  memcpy(counts, c, sizeof c);
  for (size_t k = 0; k < sh.ntt; k++) {
    const uint64_t r[4] = {tt[k].pad, (uint64_t)(tt[k].scalars - blob.data()), tt[k].seg[0].n, tt[k].seg[1].n};
    memcpy(tt_out + 4 * k, r, sizeof r);
  }
  for (size_t k = 0; k < sh.nft; k++) {
    const uint64_t r[4] = {ft[k].out_first, (uint64_t)(ft[k].scalars - blob.data()), ft[k].off, ft[k].n};
    memcpy(ft_out + 4 * k, r, sizeof r);
  }
  memcpy(meta_out, meta.data(), 6 * nreq * sizeof(uint32_t));
  for (int i = 0; i < nreq; i++) soff_out[i] = soff[i];
  // the device form
  std::vector<TblReq> dreqs(reqs);
  std::vector<uint32_t> ci(nreq + 1);
  for (int i = 0; i < nreq; i++) {
    dreqs[i].dev = blob.data() + soff[i];
    ci[i] = 5000 + i;
  }
  TblShape dsh;
  tbl_count(dreqs, crs, dsh);
  std::vector<TblTask> dtt(dsh.ntt + 1);
  std::vector<FixTask> dft(dsh.nft + 1);
  std::vector<uint32_t> dmeta(7 * nreq + 1);
  tbl_plan(dreqs, crs, fix_parts, tbl_parts, dummy_dst, nullptr, ci.data(), dsh, dtt.data(), dft.data(), dmeta.data());
  bool same = dsh.ntt == sh.ntt && dsh.nft == sh.nft && dsh.nparts == sh.nparts && dsh.fix_sets == sh.fix_sets && dsh.tbl_sets == sh.tbl_sets && dsh.nscal == 0 &&
              dsh.any_add == sh.any_add && dsh.pts_fix == sh.pts_fix && dsh.pts_tbl == sh.pts_tbl && dsh.has_comp && !sh.has_comp;
  for (size_t k = 0; same && k < sh.ntt; k++)
    same = dtt[k].pad == tt[k].pad && dtt[k].scalars == tt[k].scalars && !memcmp(dtt[k].seg, tt[k].seg, sizeof tt[k].seg) && dtt[k].flags == tt[k].flags && !dtt[k].digits;
  for (size_t k = 0; same && k < sh.nft; k++)
    same = dft[k].out_first == ft[k].out_first && dft[k].scalars == ft[k].scalars && dft[k].off == ft[k].off && dft[k].n == ft[k].n && dft[k].idx == ft[k].idx;
  for (int i = 0; same && i < nreq; i++) {
    same = dmeta[i] == meta[i] && dmeta[nreq + i] == meta[nreq + i] && dmeta[2 * nreq + i] == meta[2 * nreq + i] && dmeta[3 * nreq + i] == ci[i];
    for (int j = 0; j < 3; j++) same = same && dmeta[4 * nreq + 3 * i + j] == meta[3 * nreq + 3 * i + j];
  }
  return same ? 0 : 1;
}
