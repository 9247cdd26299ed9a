// Host engine of the MI355X Curdleproofs core — see engine.hpp.  Product code: no CPU fallback for
// the group arithmetic exists here; every point operation below is a kernel launch (kernels.hip).
#include "engine.hpp"
#include "canon_infinity.hpp"
#include "host_prove.hpp"
#include "host_verify.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <thread>

namespace cpx {

using host::S;
using host::SVec;

std::atomic<int>& Engine::live_engines() {
  static std::atomic<int> n{0};
  return n;
}
Engine::Engine(int device) : device_(device) {
  live_engines()++;
  try {
    CPX_HIP(hipSetDevice(device_));
    CPX_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    CPX_HIP(hipStreamCreateWithFlags(&side_.stream, hipStreamNonBlocking));
    CPX_HIP(hipEventCreateWithFlags(&side_.ev, hipEventDisableTiming));
  } catch (...) {   // a half-built engine owns nothing afterwards
    if (side_.ev) (void)hipEventDestroy(side_.ev);
    if (side_.stream) (void)hipStreamDestroy(side_.stream);
    if (stream_) (void)hipStreamDestroy(stream_);
    live_engines()--;
    throw;
  }
  fix_bits_cfg_ = fix_bits_ = (int)opt_.fix_bits;   // radix of the fixed-base CRS table (8: 0.1 GB, 16: 17.5 GB at ell = 252)
}
bool Engine::set_option(const char* key, long value) {
  if (!cpx::set_option(opt_, key, value)) return false;
  fix_bits_cfg_ = (int)opt_.fix_bits;   // used by the next set_crs
  dprove_.signature.clear();            // plans are laid out for a kernel selection: rebuild them
  dverify_.signature.clear();
  return true;
}
Engine::~Engine() {
  live_engines()--;
  for (auto p : idx_allocs_) (void)hipFree(p);
  if (side_.ev) (void)hipEventDestroy(side_.ev);
  if (side_.ev2) (void)hipEventDestroy(side_.ev2);
  if (ev_block_) (void)hipEventDestroy(ev_block_);
  for (hipEvent_t e : {tab_.ev_start, tab_.ev_m, tab_.ev_done})
    if (e) (void)hipEventDestroy(e);
  if (tab_.stream) (void)hipStreamDestroy(tab_.stream);
  if (tab_.dstream) (void)hipStreamDestroy(tab_.dstream);
  for (hipEvent_t e : {dprove_.ev_a, dprove_.ev_b, dprove_.ev_c, dprove_.ev_d, dprove_.ev_t1, dprove_.ev_t2, dprove_.ev_a2, dprove_.ev_ap, dprove_.ev_rs, dverify_.ev_a, dverify_.ev_b})
    if (e) (void)hipEventDestroy(e);
  if (stage_.uploaded) (void)hipEventDestroy(stage_.uploaded);
  if (stage_.consumed) (void)hipEventDestroy(stage_.consumed);
  if (stage_.stream) (void)hipStreamDestroy(stage_.stream);
  if (side_.stream) (void)hipStreamDestroy(side_.stream);
  if (side_.hi_stream) (void)hipStreamDestroy(side_.hi_stream);
  if (side_.lat_stream) (void)hipStreamDestroy(side_.lat_stream);
  if (side_.lat_main) (void)hipStreamDestroy(side_.lat_main);
  if (side_.lat_ev) (void)hipEventDestroy(side_.lat_ev);
  if (stream_) (void)hipStreamDestroy(stream_);
}

// ---------------------------------------------------------------- timing
void Engine::tick(const char* name, double bytes, double units, bool span) {
  if (!profiling_) return;
  Timed t;
  t.units = units;
  CPX_HIP(hipEventCreate(&t.a));
  CPX_HIP(hipEventCreate(&t.b));
  t.name = name;
  t.bytes = bytes;
  span_ = span;
  if (span) CPX_HIP(hipEventRecord(t.a, stream_));   // a sequence of launches: bracket it on the stream
  else set_launch_events(t.a, t.b);                  // one dispatch: events bound to kernel begin / end
  pending_.push_back(t);
}
void Engine::tock() {
  if (!profiling_) return;
  if (span_) {
    CPX_HIP(hipEventRecord(pending_.back().b, stream_));
  } else if (launches_since_set() == 0) {   // nothing was launched (empty phase): give the events a defined state
    CPX_HIP(hipEventRecord(pending_.back().a, stream_));
    CPX_HIP(hipEventRecord(pending_.back().b, stream_));
  }
  set_launch_events(nullptr, nullptr);
  span_ = false;
}
void Engine::flush_timers() {
  if (pending_.empty()) return;
  CPX_HIP(hipStreamSynchronize(stream_));
  for (auto& t : pending_) {
    float ms = 0;
    CPX_HIP(hipEventElapsedTime(&ms, t.a, t.b));
    KernelStat& st = stats_[t.name];
    st.launches++;
    st.ms += ms;
    st.alg_bytes += t.bytes;
    st.units += t.units;
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  pending_.clear();
}

Engine::TeamScope::TeamScope(Engine* e, size_t batch) {
  if (!e->opt_.spin_team || batch < 2) return;
  const size_t team_max = (size_t)e->opt_.spin_team_threads;   // size of the team when the context's host-thread count is not set
  // busy-waiting helpers only pay while they have cores of their own: the team is bounded by the cores this process may use
  // (affinity mask and cgroup CPU quota) divided by the engine contexts alive in the process
  const size_t fair = std::max<size_t>(1, effective_host_cores() / std::max<size_t>(1, (size_t)live_engines().load()));
  const size_t want = std::min({batch, e->host_threads_ > 0 ? (size_t)e->host_threads_ : team_max, fair});
  if (want < 2) return;
  if (!e->team_ || e->team_->size() < want) e->team_.reset(new SpinTeam(want - 1));
  t = e->team_.get();
  t->engage();
}

template <class F> void Engine::parallel_for(size_t n, F&& f) {
  if (team_ && team_->engaged() && n >= 2) {   // a small batch's call: spinning helpers (TeamScope)
    const std::function<void(size_t)> fn = [&](size_t i) { f(i); };
    HostSpan w(this, "host_parallel_for");
    team_->run(n, fn);
    return;
  }
  const size_t inline_below = (size_t)opt_.inline_below;
  if (n < inline_below) {   // a handful of items: waking the pool (tens of sleeping threads) costs more than the work
    for (size_t i = 0; i < n; i++) f(i);
    return;
  }
  if (!pool_) {
    size_t T = host_threads_ > 0 ? (size_t)host_threads_ : std::min<size_t>(std::max(1u, std::thread::hardware_concurrency()), 64);
    pool_.reset(new WorkerPool(T));
  }
  const std::function<void(size_t)> fn = [&](size_t i) { f(i); };
  HostSpan w(this, "host_parallel_for");
  pool_->run(n, fn);
}

// wall-clock spans of host work, reported next to the kernel statistics when profiling is on
Engine::HostSpan::HostSpan(Engine* e, const char* name) : e_(e), name_(name), t0_(std::chrono::steady_clock::now()) {}
Engine::HostSpan::~HostSpan() {
  if (!e_->profiling_) return;
  KernelStat& st = e_->stats_[name_];
  st.launches++;
  st.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0_).count();
}
void Engine::wait_stream() {
  HostSpan w(this, "host_wait_device");
  CPX_HIP(hipStreamSynchronize(stream_));
}

// Batches of at least CPX_DEVICE_MIN_BATCH proofs (default 96: measured cross-over with the spin team of the host-driven path,
// 21.9 against 35.1 ms per prove + verify pass at 32 proofs, 36.3 against 43.6 ms at 96, 59 against 54 ms at 192) run the whole protocol on the GPU (engine_device.cpp).  Smaller
// batches are driven from the host: a lone transcript is latency-bound on a GPU wave (~4 us per Keccak permutation against
// ~0.25 us on a host core, ~1000 permutations per proof), and the host has idle cores.  In the host-driven mode the
// transcript prefix of every loaded proof is hashed on the host as well.
bool Engine::device_prefix(size_t B) const {
  return B >= (size_t)opt_.device_min_batch;
}
Engine::LateShape Engine::late_shape(size_t B) const {
  LateShape lt;
  const size_t n = n_;
  lt.m = opt_.late_m ? (int)opt_.late_m : n >= 512 ? 32 : 16;
  while (lt.m > 16 && !late_supported((int)n, lt.m)) lt.m /= 2;
  lt.nr = 0;
  while ((1 << lt.nr) < lt.m) lt.nr++;
  // (late_min_batch is stated for n <= 256; larger proofs have larger grids per proof: the threshold shrinks with 256 / n)
  const size_t late_min = n <= 256 ? (size_t)opt_.late_min_batch : std::max<size_t>(1, (size_t)opt_.late_min_batch * 256 / n);
  lt.on = opt_.late_rounds != 0 && L_ >= (size_t)lt.nr + 1 && B >= late_min && late_supported((int)n, lt.m);
  return lt;
}
bool Engine::smsm_may_fuse(size_t B) const {
  const size_t fused_smsm_max = n_ <= 256 ? (size_t)opt_.fused_smsm_max : (size_t)opt_.fused_smsm_max * 256 / n_;
  return !late_shape(B).on && fix_bits_ == 16 && !opt_.serial_streams && opt_.fused_smsm_max > 0 && B <= fused_smsm_max;
}
int Engine::tbl_segments_for(size_t B) const {
  // option 0: two segments up to n = 256 (the A/B of profiles/r10_tbl_segments.md); larger proofs keep one until they are measured
  const long want = opt_.tbl_segments ? opt_.tbl_segments : (n_ <= 256 ? 2 : 1);
  return want == 2 && n_ && device_prefix(B) && !smsm_may_fuse(B) ? 2 : 1;
}
// hipStreamSynchronize spins on a host core; an event created with hipEventBlockingSync puts the thread to sleep instead.  With
// one thread per engine context and per rank, and hosts that give a container a small CPU quota, that matters.
void Engine::wait_stream_blocking() {
  if (!ev_block_) CPX_HIP(hipEventCreateWithFlags(&ev_block_, hipEventBlockingSync | hipEventDisableTiming));
  CPX_HIP(hipEventRecord(ev_block_, stream_));
  HostSpan w(this, "host_wait_device");
  CPX_HIP(hipEventSynchronize(ev_block_));
}

void Engine::transcript_prefix_async(size_t B) {
  if (!side_.ev2) CPX_HIP(hipEventCreateWithFlags(&side_.ev2, hipEventDisableTiming));
  CPX_HIP(hipEventRecord(side_.ev2, stream_));
  CPX_HIP(hipStreamWaitEvent(side_.stream, side_.ev2, 0));
  CPX_HIP(hipMemcpyAsync(h_inst_comp_.p, d_bytes_.p, B * 4 * ell_ * 48, hipMemcpyDeviceToHost, side_.stream));
  CPX_HIP(hipMemcpyAsync(h_mcomp_.p, d_mcomp_.p, B * 48, hipMemcpyDeviceToHost, side_.stream));
  CPX_HIP(hipEventRecord(side_.ev, side_.stream));
}
void Engine::wait_side() {
  HostSpan w(this, "host_wait_device");
  CPX_HIP(hipEventSynchronize(side_.ev));
}

const uint32_t* Engine::idx_list(const std::vector<uint32_t>& v) {
  auto it = idx_cache_.find(v);
  if (it != idx_cache_.end()) return it->second;
  uint32_t* d = nullptr;
  CPX_HIP(hipMalloc(&d, v.size() * sizeof(uint32_t)));
  CPX_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  idx_allocs_.push_back(d);
  idx_cache_[v] = d;
  return d;
}

// ---------------------------------------------------------------- generic phases
// Uploads the scalars of all requests, runs accumulate + tails + finalize; affine results are
// scattered to d_pp_[dst]; compressed results (48 B each, request order) returned if comp_out != null.
void Engine::run_msm_phase(const std::vector<MsmReq>& reqs, std::vector<uint8_t>* comp_out) {
  const size_t nt = reqs.size();
  if (!nt) return;
  size_t total = 0;
  for (auto& r : reqs) total += r.n;
  d_scal_.ensure(total);
  d_tasks_.ensure(nt);
  d_wsum_.ensure(nt * 64);
  d_part_.ensure(nt * 8);
  d_res_.ensure(nt);
  d_dst_.ensure(nt);
  d_comp_.ensure(nt * 48);
  const size_t stage_bytes = total * sizeof(Fr) + nt * sizeof(MsmTask) + nt * sizeof(uint32_t);
  h_stage_.ensure(stage_bytes);
  Fr* hs = reinterpret_cast<Fr*>(h_stage_.p);
  MsmTask* ht = reinterpret_cast<MsmTask*>(h_stage_.p + total * sizeof(Fr));
  uint32_t* hd = reinterpret_cast<uint32_t*>(h_stage_.p + total * sizeof(Fr) + nt * sizeof(MsmTask));
  std::vector<size_t> soff(nt);
  size_t off = 0;
  for (size_t i = 0; i < nt; i++) {
    soff[i] = off;
    off += reqs[i].n;
  }
  const double alg = 128.0 * (double)total;   // 96 B affine base + 32 B scalar per MSM point
  parallel_for(nt, [&](size_t i) {
    const MsmReq& r = reqs[i];
    Fr* d = hs + soff[i];
    for (uint32_t j = 0; j < r.n; j++) d[j] = r.scalars[j].f;
    ht[i] = MsmTask{r.bases, r.idx, d_scal_.p + soff[i], r.n, 0, (uint32_t)soff[i]};
    hd[i] = r.dst;
  });
  CPX_HIP(hipMemcpyAsync(d_scal_.p, hs, total * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_tasks_.p, ht, nt * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_dst_.p, hd, nt * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  uint32_t max_n = 0;
  for (auto& r : reqs) max_n = std::max(max_n, r.n);
  d_conv_.ensure(std::max<size_t>(total, 1));
  tick("k_msm_accw", alg, (double)total);
  launch_msm_accum(d_tasks_.p, (int)nt, (int)max_n, d_conv_.p, d_wsum_.p, stream_);
  tock();
  tick("k_msm_tail", 0, (double)nt * 8);
  launch_msm_tail(opt_, d_wsum_.p, d_part_.p, nullptr, (int)nt * 8, 8, 4, stream_);
  tock();
  tick("k_msm_tail", 0, (double)nt);
  launch_msm_tail(opt_, d_part_.p, nullptr, d_res_.p, (int)nt, 8, 32, stream_);
  tock();
  tick("k_finalize", 0, (double)nt);
  launch_finalize(d_res_.p, (int)nt, d_pp_.p, d_dst_.p, d_comp_.p, stream_);
  tock();
  if (comp_out) {
    h_comp_.ensure(nt * 48);
    CPX_HIP(hipMemcpyAsync(h_comp_.p, d_comp_.p, nt * 48, hipMemcpyDeviceToHost, stream_));
    wait_stream();
    comp_out->assign(h_comp_.p, h_comp_.p + nt * 48);
  }
}

// tasks[i].scalars must already point into d_scal_ (offsets in Fr units from its base are set by the caller
// through `scalars`/`nscalars`, uploaded here).
void Engine::run_smul(const std::vector<SmulTask>& tasks, int cnt, const S* scalars, size_t nscalars, double alg_bytes) {
  if (tasks.empty() || cnt <= 0) return;
  d_stasks_.ensure(tasks.size());
  h_stage_.ensure(nscalars * sizeof(Fr) + tasks.size() * sizeof(SmulTask));
  Fr* hs = reinterpret_cast<Fr*>(h_stage_.p);
  for (size_t i = 0; i < nscalars; i++) hs[i] = scalars[i].f;
  SmulTask* ht = reinterpret_cast<SmulTask*>(h_stage_.p + nscalars * sizeof(Fr));
  memcpy(ht, tasks.data(), tasks.size() * sizeof(SmulTask));
  // the staging buffer may still be in flight from a previous async copy on this stream only if the caller
  // did not synchronise; every phase ends with a synchronising D2H or the explicit sync below.
  CPX_HIP(hipMemcpyAsync(d_scal_.p, hs, nscalars * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_stasks_.p, ht, tasks.size() * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
  tick("k_smul", alg_bytes, (double)tasks.size() * cnt);
  launch_smul(d_stasks_.p, (int)tasks.size(), cnt, stream_);
  tock();
  wait_stream();   // staging buffer reuse safety
}

// the raw lane accumulators of `sc` (kernels.h) reduced to partial sums, in sc.part unless told otherwise
void Engine::reduce_sets(hipStream_t st, MsmScratch& sc, size_t nplain, size_t nweighted, TJac* part) {
  const bool span = st == stream_;   // up to four launches (groups of 8 lanes, then the groups of a set; plain / bucket sets): a span is bracketed on the main stream, another stream's is not timed
  if (span) tick("k_reduce_sets", 0, (double)(nplain + nweighted), true);
  launch_reduce_sets(opt_, sc.raw.p, sc.rawslot.p, (int)nplain, (int)nweighted, sc.mid.p, part ? part : sc.part.p, st, (int)B_);
  if (span) tock();
}

// Table-backed MSM phase: the CRS segments of a request go to k_msm_fix, the per-proof segments to k_msm_tblw (one
// wave per task and window group); k_reduce_sets turns the raw lane accumulators into partial sums, k_finalize_ranges
// adds them per request, normalises, scatters the affine point and writes the compressed bytes to d_comp (slot
// comp_index[i] of it where the per-request arrays carry one).  `sc` must hold sh.fix_sets + sh.tbl_sets sets and sh.nparts partial sums.
void Engine::launch_tbl_phase(const TblShape& sh, const TblTask* d_tt, const FixTask* d_ft, const uint32_t* d_meta, uint8_t* d_comp, hipStream_t st, MsmScratch& sc,
                              bool timed) {
  if (!sh.nt) return;
  Untimed quiet(this, timed);
  uint32_t* const traw = sc.raw.p + sh.fix_sets * raw_set_words();
  if (sh.one_launch && sh.tbl_segments != 1) throw std::logic_error("the one-launch phase of a lone proof reads one-segment tables");
  if (sh.one_launch) {   // a lone proof: both MSM kernels of the phase in one launch
    tick("k_msm_fix_tblw", 128.0 * (sh.pts_fix + sh.pts_tbl), sh.pts_fix + sh.pts_tbl);
    launch_msm_fix_tblw(d_ft, (int)sh.nft, fixtab(), (int)nc(), sc.raw.p, sc.rawslot.p, d_tt, (int)sh.ntt, sh.tbl_slices, traw, sc.rawslot.p + sh.fix_sets, st);
    tock();
  } else {
    if (sh.nft) {
      tick(fix_kernel_name(fix_bits_, sh.fix_wpw), 128.0 * sh.pts_fix, sh.pts_fix);
      launch_msm_fix(d_ft, (int)sh.nft, fixtab(), fix_bits_, sh.fix_wpw, (int)nc(), sc.raw.p, sc.rawslot.p, st);
      tock();
    }
    if (sh.ntt) {
      tick(tblw_kernel_name(sh.tbl_wpw), 128.0 * sh.pts_tbl, sh.pts_tbl);   // (the statistics keep one name per window grouping, whichever table layout)
      launch_msm_tblw(d_tt, (int)sh.ntt, sh.tbl_wpw, traw, sc.rawslot.p + sh.fix_sets, st, sh.tbl_slices, sh.tbl_segments);
      tock();
    }
  }
  reduce_sets(st, sc, sh.fix_sets, sh.tbl_sets);
  const uint32_t* m = d_meta;
  tick("k_finalize_ranges", 0, (double)sh.nt);
  launch_finalize_ranges(opt_, sc.part.p, m, m + sh.nt, (int)sh.nt, d_pp_.p, m + 2 * sh.nt, d_comp, st, sh.any_add ? m + sh.add_offset() : nullptr, sh.has_comp ? m + 3 * sh.nt : nullptr);
  tock();
}

// Plans a host-driven phase and brings it to the device: everything the phase's kernels read — scalars, task descriptors, partial
// ranges, destinations, addends — is staged in ONE pinned buffer with the layout [Fr scalars | TblTask | FixTask | u32 arrays] and
// uploaded with ONE copy into a device blob of the same layout (a handful of separate small copies cost ~30 us of host time per
// phase, which a lone proof waits for); then the launches, on stream `st` in scratch `sc`; compressed results (48 B each, request order) in `comp`.
void Engine::enqueue_tbl_phase(const std::vector<TblReq>& reqs, uint32_t dummy_dst, PinBuf<uint8_t>& stage, DevBuf<uint8_t>& blob, DevBuf<uint8_t>& comp, hipStream_t st,
                               MsmScratch& sc, bool timed) {
  const size_t nt = reqs.size();
  TblShape sh;
  const bool fix = fix_bits_ && fixtab();
  const CrsRange crs{fix ? ctab() : nullptr, fix ? ctab() + (size_t)copies_ * nc() : nullptr};
  tbl_count(reqs, crs, sh);
  sh.fix_wpw = fix ? msm_fix_windows_per_wave(opt_, (int)sh.nft, fix_bits_) : 16;
  sh.tbl_wpw = msm_tblw_windows_per_wave(opt_, (int)sh.ntt);   // windows per wave of the shifted-table kernel
  sh.tbl_slices = msm_tblw_slices(opt_, (int)sh.ntt, sh.tbl_wpw, (int)sh.tbl_max_n);   // a lone proof: several waves share a task's points
  sh.one_launch = sh.nft && sh.ntt && fix_bits_ == 16 && sh.fix_wpw == 2 && sh.tbl_wpw == 2;
  const size_t b_scal = sh.nscal * sizeof(Fr), b_tt = sh.ntt * sizeof(TblTask), b_ft = sh.nft * sizeof(FixTask);
  static_assert(sizeof(TblTask) % 8 == 0 && sizeof(FixTask) % 8 == 0 && sizeof(Fr) % 8 == 0, "blob sections keep pointer alignment");
  const size_t b_blob = b_scal + b_tt + b_ft + 6 * nt * sizeof(uint32_t);
  stage.ensure(b_blob);
  blob.ensure(b_blob);
  Fr* hs = reinterpret_cast<Fr*>(stage.p);
  std::vector<size_t> soff(nt);
  tbl_plan(reqs, crs, fix ? (uint32_t)msm_fix_parts(fix_bits_, sh.fix_wpw) : 0, (uint32_t)(msm_tblw_parts(sh.tbl_wpw) * sh.tbl_slices), dummy_dst,
           reinterpret_cast<const Fr*>(blob.p), nullptr, sh, reinterpret_cast<TblTask*>(stage.p + b_scal), reinterpret_cast<FixTask*>(stage.p + b_scal + b_tt),
           reinterpret_cast<uint32_t*>(stage.p + b_scal + b_tt + b_ft), soff.data());
  parallel_for(nt, [&](size_t i) {
    const TblReq& r = reqs[i];
    if (r.dev) return;
    Fr* d = hs + soff[i];
    for (uint32_t j = 0; j < r.seg0.n; j++) d[j] = r.s0[j].f;
    for (uint32_t j = 0; j < r.seg1.n; j++) d[r.seg0.n + j] = r.s1[j].f;
  });
  CPX_HIP(hipMemcpyAsync(blob.p, stage.p, b_blob, hipMemcpyHostToDevice, st));
  comp.ensure(nt * 48);
  sc.ensure(sh.fix_sets + sh.tbl_sets, sh.nparts);
  launch_tbl_phase(sh, reinterpret_cast<const TblTask*>(blob.p + b_scal), reinterpret_cast<const FixTask*>(blob.p + b_scal + b_tt),
                   reinterpret_cast<const uint32_t*>(blob.p + b_scal + b_tt + b_ft), comp.p, st, sc, timed);
}

// affine results are scattered to d_pp_[dst]; compressed results (48 B each, request order) returned if comp_out != null
void Engine::run_tbl_phase(const std::vector<TblReq>& reqs, std::vector<uint8_t>* comp_out) {
  const size_t nt = reqs.size();
  if (!nt) return;
  enqueue_tbl_phase(reqs, slot_index(0, SlotMap(L_).TMP(7)), h_stage_, d_blob_, d_comp_, stream_, main_, true);   // results nobody reads land in a scratch slot
  if (comp_out) {
    h_comp_.ensure(nt * 48);
    CPX_HIP(hipMemcpyAsync(h_comp_.p, d_comp_.p, nt * 48, hipMemcpyDeviceToHost, stream_));
    wait_stream();
    comp_out->assign(h_comp_.p, h_comp_.p + nt * 48);
  }
}

// The requests of a phase as prove_reqs.hpp describes them, for every loaded proof: the gather lists of the list are resolved once, the
// rest per proof.  The ONE place where a request of the protocol becomes a TblReq.
std::vector<TblReq> Engine::make_reqs(const ReqList& list, const ScalAt& scal_at, std::vector<uint32_t>* comp_index) {
  const SlotMap sm(L_);
  const uint32_t* idx[ReqList::MAX][2];
  std::vector<uint32_t> g(n_ + 1);
  for (int i = 0; i < list.n; i++)
    for (int h = 0; h < 2; h++) {
      const ReqSeg& sg = h ? list.r[i].seg1 : list.r[i].seg0;
      const int cnt = gather_list((int)n_, sg.gather, sg.arg, g.data());
      idx[i][h] = cnt ? idx_list(std::vector<uint32_t>(g.begin(), g.begin() + cnt)) : nullptr;
    }
  auto seg = [&](size_t p, const ReqSeg& sg, const uint32_t* ix) {
    return sg.kind == SEG_CRS ? cseg((size_t)sg.off, (uint32_t)sg.n, ix) : sg.kind == SEG_PTAB ? pseg(p, (size_t)sg.off, (uint32_t)sg.n, ix) : TblSeg{nullptr, nullptr, 0, 0};
  };
  std::vector<TblReq> reqs;
  reqs.reserve(B_ * (size_t)list.n);
  for (size_t p = 0; p < B_; p++)
    for (int i = 0; i < list.n; i++) {
      const ReqDesc& d = list.r[i];
      TblReq r{seg(p, d.seg0, idx[i][0]), nullptr, seg(p, d.seg1, idx[i][1]), nullptr};
      if (d.keep >= 0) r.dst = slot_index(p, d.keep);
      for (int j = 0; j < 3; j++)
        if (d.add[j] >= 0) r.add[j] = slot_index(p, d.add[j]);
      if (d.scal.kind == SCAL_ROUND) r.dev = d_rout_.p + p * (size_t)list.round_stride + d.scal.at;
      else if (d.scal.kind != SCAL_NONE) {
        const ScalAddr a = scal_at(p, d.scal);
        r.s0 = a.host;
        r.s1 = a.host ? a.host + d.seg0.n : nullptr;
        r.dev = a.dev;
      }
      reqs.push_back(r);
      // (a request without an output: its compressed bytes go to TMP(6), which nobody reads)
      if (comp_index) comp_index->push_back((uint32_t)(p * sm.count() + (d.out >= 0 ? d.out : sm.TMP(6))));
    }
  return reqs;
}

// R = a x vec_R, S = a x vec_S (curdleproofs.rs:112-113) and whatever further tasks over the same points side_.tasks holds: the
// endomorphism bucket-list kernel (pairs: R and S of a proof share the scalars vec_a — one wave per (proof, window) serves both,
// kernels.h launch_msm_endo_pairs), reduction and Horner tail in the side scratch on stream `st`; the first nfinal results go to
// their slots (side_.dst)
void Engine::launch_rs(size_t ntasks, size_t nfinal, int slices, bool pairs, hipStream_t st, bool timed) {
  Untimed quiet(this, timed);
  MsmScratch& sc = side_.scr;
  tick(pairs ? "k_msm_tblw_pair" : "k_msm_tblw<2, true>", 128.0 * ntasks * ell_, (double)(ntasks * ell_));
  if (pairs) launch_msm_endo_pairs(side_.tasks.p, (int)(ntasks / 2), (int)ell_, side_.conv.p, side_.digits.p, side_.ttasks.p, sc.raw.p, sc.rawslot.p, st);
  else launch_msm_endo(side_.tasks.p, (int)ntasks, (int)ell_, side_.conv.p, side_.digits.p, side_.ttasks.p, sc.raw.p, sc.rawslot.p, st, slices);
  tock();
  reduce_sets(st, sc, 0, ntasks * 32 * slices);
  tick("k_msm_tail", 0, (double)ntasks);
  launch_msm_tail(opt_, sc.part.p, nullptr, side_.res.p, (int)ntasks, 16, 8, st, nullptr, 0, 2 * slices);
  tock();
  launch_finalize(side_.res.p, (int)nfinal, d_pp_.p, side_.dst.p, nullptr, st);
}

// The verifier's accumulated check of every proof as ONE sum: the CRS part on the fixed-base table (d_ft: one task of n scalars per
// proof, fix_parts partial sums each), all the per-proof points (d_mt: R | S | T | U and the slots, NPT per proof; used once, so no
// shifted tables — endomorphism split + radix-256 buckets per window) in one bucket MSM; the Horner tail adds the two.  The compressed
// sums arrive in h_comp_: check_passed(p) once the caller has waited for the stream.
void Engine::launch_check(const MsmTask* d_mt, const FixTask* d_ft, size_t B, size_t NPT, int fix_wpw, int fix_parts, size_t slices) {
  d_conv_.ensure(2 * B * NPT);   // points and their endomorphism images
  d_digits_.ensure(9 * B * NPT);
  d_ttasks_.ensure(B);
  d_part_.ensure(B * 32 * slices);
  d_res_.ensure(B);
  d_comp_.ensure(B * 48);
  h_comp_.ensure(B * 48);
  main_.ensure(B * std::max<size_t>(fix_parts, 32 * slices), B * (size_t)fix_parts);
  tick(fix_kernel_name(fix_bits_, fix_wpw), 128.0 * n_ * B, (double)(n_ * B));
  launch_msm_fix(d_ft, (int)B, fixtab(), fix_bits_, fix_wpw, (int)nc(), main_.raw.p, main_.rawslot.p, stream_);
  tock();
  reduce_sets(stream_, main_, B * fix_parts, 0);
  tick("k_msm_tblw<2, true>", 128.0 * NPT * B, (double)(NPT * B));
  launch_msm_endo(d_mt, (int)B, (int)NPT, d_conv_.p, d_digits_.p, d_ttasks_.p, main_.raw.p, main_.rawslot.p, stream_, (int)slices);
  tock();
  reduce_sets(stream_, main_, 0, B * 32 * slices, d_part_.p);
  tick("k_msm_tail", 0, (double)B);
  launch_msm_tail(opt_, d_part_.p, nullptr, d_res_.p, (int)B, 16, 8, stream_, main_.part.p, fix_parts, (int)(2 * slices));
  tock();
  tick("k_finalize", 0, (double)B);
  launch_finalize(d_res_.p, (int)B, nullptr, nullptr, d_comp_.p, stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(h_comp_.p, d_comp_.p, B * 48, hipMemcpyDeviceToHost, stream_));
}

// BASELINE config 5: one MSM over the CRS (d_ft: ONE task, the scalars summed over the proofs) and the N = B * NPT per-proof points
// of NT groups of G proofs (d_gt) through the endomorphism bucket-list kernel (32 additions per point like the per-proof verifier,
// but one bucket reduction and one Horner tail per GROUP of proofs), then two plain summation levels; the last one adds the
// fixed-base part and hands the sum over in the standard form: a Jac in h_comp_.
void Engine::launch_check_fused(const MsmTask* d_gt, const FixTask* d_ft, size_t NT, size_t G, size_t NPT, size_t N, int fix_wpw, int fix_parts) {
  const size_t NT16 = (NT + 15) / 16 * 16;
  d_ttasks_.ensure(NT);
  d_conv_.ensure(2 * N);
  d_digits_.ensure(9 * N);
  d_part_.ensure(NT * 32);
  d_wsum_.ensure(NT16 + NT16 / 16);
  d_res_.ensure(1);
  h_comp_.ensure(sizeof(Jac));
  main_.ensure(std::max<size_t>(NT * 32, fix_parts), fix_parts);
  launch_msm_fix(d_ft, 1, fixtab(), fix_bits_, fix_wpw, (int)nc(), main_.raw.p, main_.rawslot.p, stream_);
  reduce_sets(stream_, main_, fix_parts, 0);
  CPX_HIP(hipMemsetAsync(d_wsum_.p, 0, (NT16 + NT16 / 16) * sizeof(TJac), stream_));   // all-zero = identity: pads the summation levels
  tick("k_msm_tblw<2, true>", 128.0 * N, (double)N);
  launch_msm_endo(d_gt, (int)NT, (int)(G * NPT), d_conv_.p, d_digits_.p, d_ttasks_.p, main_.raw.p, main_.rawslot.p, stream_);
  tock();
  reduce_sets(stream_, main_, 0, NT * 32, d_part_.p);
  tick("k_msm_tail", 0, (double)NT, true);
  launch_msm_tail(opt_, d_part_.p, d_wsum_.p, nullptr, (int)NT, 16, 8, stream_, nullptr, 0, 2);                            // windows of a group
  launch_msm_tail(opt_, d_wsum_.p, d_wsum_.p + NT16, nullptr, (int)(NT16 / 16), 16, 0, stream_);                           // 16 groups each
  launch_msm_tail(opt_, d_wsum_.p + NT16, nullptr, d_res_.p, 1, (int)(NT16 / 16), 0, stream_, main_.part.p, fix_parts);    // + the fixed-base part
  tock();
  CPX_HIP(hipMemcpyAsync(h_comp_.p, d_res_.p, sizeof(Jac), hipMemcpyDeviceToHost, stream_));
}

size_t Engine::located_check(const CheckPlan& cp, const LocatePlan& lp, const LocateTasks& t, const uint32_t* flags, bool resident, int* verdict) {
  auto slices = [&](size_t tasks, size_t max_n) { return resident ? (size_t)1 : (size_t)msm_tblw_slices(opt_, (int)tasks, 2, (int)max_n); };
  auto wait = [&] { resident ? wait_stream_blocking() : wait_stream(); };
  // ---- stage 1: every group's sum tested for the identity
  launch_check(t.mt1, t.ft1, lp.NT, lp.s1_max_n(cp.NPT), t.fix_wpw, t.fix_parts, slices(lp.NT, lp.s1_max_n(cp.NPT)));
  wait();
  std::vector<uint8_t> group_ok(lp.NT), recheck_ok;
  for (size_t g = 0; g < lp.NT; g++) group_ok[g] = check_passed(g) ? 1 : 0;   // (before stage 2 overwrites h_comp_)
  std::vector<uint32_t> list;
  locate_stage2(lp, group_ok.data(), flags, list);   // empty with one proof per group: stage 1 was the per-proof check
  // ---- stage 2: the suspects' own checks from the scalars stage 1 left in place; nothing when every group passed
  const size_t S = list.size();
  if (S) {
    const int fix_wpw = msm_fix_windows_per_wave(opt_, (int)S, fix_bits_), fix_parts = msm_fix_parts(fix_bits_, fix_wpw);
    std::vector<MsmTask> mt(S);   // (copied asynchronously: alive until the wait below)
    std::vector<FixTask> ft(S);
    cp.suspect_tasks(list, (size_t)fix_parts, mt.data(), ft.data());
    CPX_HIP(hipMemcpyAsync(t.mt2, mt.data(), S * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(t.ft2, ft.data(), S * sizeof(FixTask), hipMemcpyHostToDevice, stream_));
    launch_check(t.mt2, t.ft2, S, cp.NPT, fix_wpw, fix_parts, slices(S, cp.NPT));
    wait();
    recheck_ok.resize(S);
    for (size_t s = 0; s < S; s++) recheck_ok[s] = check_passed(s) ? 1 : 0;
  }
  locate_verdicts(lp, group_ok.data(), flags, list, recheck_ok.data(), verdict);
  return S;
}

// ---------------------------------------------------------------- CRS
void Engine::set_crs(size_t ell, const uint8_t* points) {
  const size_t n = ell + N_BLINDERS;
  if (ell == 0 || (n & (n - 1))) throw std::invalid_argument("ell + 4 must be a power of two");
  // the cached device plans were laid out for the previous CRS (they embed its compressed H and table addresses, which a new
  // allocation of the same size may reuse): a new CRS — also a refused one — starts from no plans
  dprove_.signature.clear();
  dverify_.signature.clear();
  try {
    set_crs_impl(ell, points);
  } catch (...) {   // e.g. out of device memory while building the tables: the context is left without a CRS, not half-initialised
    ell_ = n_ = L_ = 0;
    B_ = 0;
    consts_rows_ = 0;
    crs_tab_.reset();
    throw;
  }
}
void Engine::set_crs_impl(size_t ell, const uint8_t* points) {
  const size_t n = ell + N_BLINDERS;
  CPX_HIP(hipSetDevice(device_));
  ell_ = ell;
  n_ = n;
  L_ = 0;
  while ((size_t(1) << L_) < n) L_++;
  const Aff* pts = reinterpret_cast<const Aff*>(points);
  crs_host_.assign(pts, pts + ell + 7);
  const CtabCols cc(n);   // (the CRS table columns up to G_u are the indices of the input points)
  std::vector<Aff> crs(n + 1), gb(n);
  for (size_t i = 0; i < n; i++) crs[i] = pts[i];   // G | Hvec
  crs[n] = pts[cc.H()];                             // H
  std::vector<uint32_t> gb_cols(n);
  cc.same_msm_basis(gb_cols.data());
  for (size_t i = 0; i < n; i++) gb[i] = pts[gb_cols[i]];
  d_crs_.ensure(n + 1);
  d_crs_gb_.ensure(n);
  CPX_HIP(hipMemcpy(d_crs_.p, crs.data(), (n + 1) * sizeof(Aff), hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(d_crs_gb_.p, gb.data(), n * sizeof(Aff), hipMemcpyHostToDevice));
  crs_single_[0] = pts[cc.H()];
  crs_single_[1] = pts[cc.G_t()];
  crs_single_[2] = pts[cc.G_u()];
  // G_sum, H_sum (crs.rs:46-47) as unit-scalar MSMs on the device
  B_ = 0;
  consts_rows_ = 0;
  pp_stride_ = 4 * ell_ + SlotMap(L_).count();
  d_pp_.ensure(pp_stride_);
  SVec ones(ell, S::one());
  std::vector<MsmReq> reqs;
  reqs.push_back(MsmReq{d_crs_.p, nullptr, ones.data(), (uint32_t)ell, 0});
  reqs.push_back(MsmReq{d_crs_.p + ell, nullptr, ones.data(), (uint32_t)N_BLINDERS, 1});
  std::vector<uint8_t> comp;
  run_msm_phase(reqs, &comp);
  Aff sums[2];
  CPX_HIP(hipMemcpy(sums, d_pp_.p, 2 * sizeof(Aff), hipMemcpyDeviceToHost));
  crs_single_[3] = sums[0];
  crs_single_[4] = sums[1];
  // compressed H (needed for the vec_T/vec_U blinder slots in the transcript)
  d_comp_.ensure(48);
  CPX_HIP(hipMemcpy(d_pp_.p, &crs_single_[0], sizeof(Aff), hipMemcpyHostToDevice));
  launch_compress(d_pp_.p, 1, 1, 1, d_comp_.p, stream_);
  CPX_HIP(hipMemcpyAsync(crs_H_comp_, d_comp_.p, 48, hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipStreamSynchronize(stream_));
  // shifted-base table + fixed-base table of multiples: built once per (device, CRS), shared by every proof and
  // by every engine of this process on the device
  {
    static std::mutex reg_mu;
    static std::vector<std::weak_ptr<CrsTables>> registry;
    std::lock_guard<std::mutex> lk(reg_mu);
    const size_t NC = nc();
    int want_fix = fix_bits_cfg_;
    // 19 bits: 14 windows x 2^18 multiples = 122 GB at ell = 252 (leave room for the batches: at most 45 % of the HBM); 16 bits: 17.5 GB
    // at ell = 252, 70 GB at ell = 1020; fall back 19 -> 16 -> 8 (0.1 GB / 0.4 GB) when HBM is short
    for (int cand : {19, 16}) {
      if (want_fix != cand) continue;
      size_t free_b = 0, total_b = 0;
      CPX_HIP(hipMemGetInfo(&free_b, &total_b));
      const size_t Wc = (size_t)msm_fix_windows(cand), segs = cand == 19 ? 8 : 1;
      const size_t need = Wc * ((size_t)1 << (cand - 1)) * NC * sizeof(TFix) + (Wc * NC * segs + 63) * 256 * sizeof(TblTmp);
      bool have = false;   // an existing shared table costs nothing
      for (auto& w : registry)
        if (auto sp = w.lock()) have |= sp->device == device_ && sp->fix_bits == cand && sp->key.size() == (ell + 7) * sizeof(Aff) && !memcmp(sp->key.data(), points, sp->key.size());
      if (!have && (need + (need >> 3) > free_b || (cand == 19 && need > total_b / 20 * 9))) want_fix = cand == 19 ? 16 : 8;
    }
    fix_bits_ = want_fix;
    std::vector<uint8_t> key(points, points + (ell + 7) * sizeof(Aff));
    crs_tab_.reset();
    for (auto it = registry.begin(); it != registry.end();) {
      auto sp = it->lock();
      if (!sp) {
        it = registry.erase(it);
        continue;
      }
      if (sp->device == device_ && sp->fix_bits == want_fix && sp->key == key) crs_tab_ = sp;
      ++it;
    }
    if (!crs_tab_) {
      auto tab = std::make_shared<CrsTables>();
      tab->device = device_;
      tab->fix_bits = want_fix;
      tab->key = std::move(key);
      tab->ctab.ensure((size_t)copies_ * NC);
      std::vector<Aff> row(NC);
      for (int i = 0; i <= cc.G_u(); i++) row[i] = pts[i];   // G | Hvec | H | G_t | G_u
      row[cc.G_sum()] = crs_single_[3];                      // G_sum, H_sum (crs.rs:46-47): B, D are built from them
      row[cc.H_sum()] = crs_single_[4];
      DevBuf<Aff> d_row;
      d_row.ensure(NC);
      CPX_HIP(hipMemcpy(d_row.p, row.data(), NC * sizeof(Aff), hipMemcpyHostToDevice));
      DevBuf<TblTmp> tmp;   // build scratch, released afterwards
      tmp.ensure(NC * (size_t)(copies_ - 1));
      launch_table_build(opt_, d_row.p, 0, tab->ctab.p, 1, 0, (int)NC, (int)NC, copies_, true, tmp.p, stream_);
      CPX_HIP(hipStreamSynchronize(stream_));
      if (want_fix) {
        // multiples m * 2^(c w) * P, m <= 2^(c-1): shifted copies first, then the multiples
        const int W = msm_fix_windows(want_fix);
        const size_t M = size_t(1) << (want_fix - 1);
        DevBuf<TAff> d_shift;
        d_shift.ensure((size_t)W * NC);
        launch_table_build(opt_, d_row.p, 0, d_shift.p, 1, 0, (int)NC, (int)NC, W, false, tmp.p, stream_, want_fix);   // copy w = 2^(want_fix w) P
        tab->fixtab.ensure((size_t)W * M * NC);
        const int chunk = (int)std::min<size_t>(256, M);
        const int segs = want_fix == 19 ? 8 : 1;   // 2^18 multiples per (window, base): eight threads of 2^15 each
        const size_t threads = ((size_t)W * NC * segs + 63) / 64 * 64;
        tmp.ensure(threads * chunk);
        launch_fix_build(d_shift.p, (int)NC, want_fix, tab->fixtab.p, tmp.p, chunk, stream_, segs);
        CPX_HIP(hipStreamSynchronize(stream_));
      }
      registry.push_back(tab);
      crs_tab_ = tab;
    }
  }
}
void Engine::crs_sums(uint8_t* g_sum, uint8_t* h_sum) const {
  memcpy(g_sum, &crs_single_[3], sizeof(Aff));
  memcpy(h_sum, &crs_single_[4], sizeof(Aff));
}

// ---------------------------------------------------------------- tier 0
Engine::CallScope::CallScope(Engine* e) : e_(e), uncaught_(std::uncaught_exceptions()) {
  if (e->in_call_) throw std::logic_error("a tier-0 call inside a tier-0 call: their scratch scopes do not nest");
  CPX_HIP(hipSetDevice(e->device_));
  e->in_call_ = true;
}
void Engine::CallScope::finish() {
  CPX_HIP(hipStreamSynchronize(e_->stream_));   // the results are in the caller's buffers; the scratch may be reused by the next call
  e_->flush_timers();
}
Engine::CallScope::~CallScope() {
  if (std::uncaught_exceptions() != uncaught_) {   // the call threw: nothing it enqueued may outlive it, none of its timings is read
    (void)hipStreamSynchronize(e_->stream_);
    set_launch_events(nullptr, nullptr);
    e_->span_ = false;
    for (auto& t : e_->pending_) {
      (void)hipEventDestroy(t.a);
      (void)hipEventDestroy(t.b);
    }
    e_->pending_.clear();
  }
  const auto trim = [](auto& b) {
    if (b.bytes() > kTier0Keep) b.release();
  };
  Tier0::each(e_->t0_, trim);
  ShuffleBufs::each(e_->sh_, trim);
  if (!e_->t0_.gen.p) e_->t0_.gen_n = 0;
  e_->in_call_ = false;
}

void Engine::msm(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out_jac) {
  if ((long)n >= opt_.msm_endo_min && n) {   // endomorphism split + radix-256 bucket lists (the verifier's kernel): 32 additions per point
    const uint32_t len = (uint32_t)n;
    Tier0MsmPlan pl;   // msm_many's plan of one task, without its limits
    pl.count = 1;
    pl.points = n;
    pl.max_n = len;
    pl.conv_off.assign(1, 0);
    msm_lists(pl, &len, bases, scalars, out_jac, nullptr);
    return;
  }
  MsmTask t;
  CallScope call(this);
  DevBuf<Aff>& db = t0_.a0;   // (tier-0 scratch of the engine, engine.hpp: no allocation on the call path once warm)
  DevBuf<Fr>& ds = t0_.fr;
  DevBuf<MsmTask>& dt = t0_.mtask;
  DevBuf<TJac>&w = t0_.w, &pt = t0_.pt;
  DevBuf<Jac>& res = t0_.res;
  DevBuf<TAff>& conv = t0_.conv;
  db.ensure(std::max<size_t>(n, 1));
  ds.ensure(std::max<size_t>(n, 1));
  dt.ensure(1);
  w.ensure(64);
  pt.ensure(8);
  res.ensure(1);
  conv.ensure(2 * std::max<size_t>(n, 1));
  if (n) {
    CPX_HIP(hipMemcpyAsync(db.p, bases, n * sizeof(Aff), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(ds.p, scalars, n * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  t = MsmTask{db.p, nullptr, ds.p, (uint32_t)n, 0, 0};
  CPX_HIP(hipMemcpyAsync(dt.p, &t, sizeof t, hipMemcpyHostToDevice, stream_));
  tick("k_msm_accw", 128.0 * n, (double)n);
  launch_msm_accum(dt.p, 1, (int)n, conv.p, w.p, stream_);
  tock();
  launch_msm_tail(opt_, w.p, pt.p, nullptr, 8, 8, 4, stream_);
  launch_msm_tail(opt_, pt.p, nullptr, res.p, 1, 8, 32, stream_);
  CPX_HIP(hipMemcpyAsync(out_jac, res.p, sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  call.finish();
}
void Engine::normalize(const uint8_t* jac, size_t n, uint8_t* out_aff, uint8_t* out_comp) {
  if (!n) return;
  CallScope call(this);
  DevBuf<Jac>& dj = t0_.jin;
  DevBuf<Aff>& da = t0_.a0;
  DevBuf<uint8_t>& dc = t0_.bytes;
  dj.ensure(n);
  da.ensure(n);
  dc.ensure(n * 48);
  CPX_HIP(hipMemcpyAsync(dj.p, jac, n * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  launch_finalize(dj.p, (int)n, da.p, nullptr, dc.p, stream_);
  if (out_aff) CPX_HIP(hipMemcpyAsync(out_aff, da.p, n * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  if (out_comp) CPX_HIP(hipMemcpyAsync(out_comp, dc.p, n * 48, hipMemcpyDeviceToHost, stream_));
  call.finish();
}
bool Engine::sum_jac(const uint8_t* points_jac, size_t n, uint8_t* out_jac) {
  int flag = 0;
  CallScope call(this);
  DevBuf<Jac>&din = t0_.jin, &dout = t0_.res;
  DevBuf<int>& dflag = t0_.flag;
  din.ensure(std::max<size_t>(n, 1));
  dout.ensure(1);
  dflag.ensure(1);
  if (n) CPX_HIP(hipMemcpyAsync(din.p, points_jac, n * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  launch_sum_jac(din.p, (int)n, dout.p, dflag.p, stream_);
  CPX_HIP(hipMemcpyAsync(out_jac, dout.p, sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(&flag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
  call.finish();
  return flag != 0;
}
void Engine::msm_jac(const uint8_t* bases_jac, const uint8_t* scalars, size_t n, uint8_t* out_jac) {   // (two calls, one scope after the other)
  std::vector<uint8_t> aff(std::max<size_t>(n, 1) * sizeof(Aff));
  normalize(bases_jac, n, aff.data(), nullptr);
  msm(aff.data(), scalars, n, out_jac);
}
void Engine::fold(uint8_t* PL, const uint8_t* PR, const uint8_t* gamma, size_t half) {
  if (half) fold_lanes(1, half, PL, PR, gamma, 0);   // quad_max 0: cpx_g1_fold keeps the one-lane k_smul (kernels.h, option fold_quad_max)
}
void Engine::scale(const uint8_t* P, const uint8_t* scalars, size_t scalar_stride, size_t n, uint8_t* out) {
  if (!n) return;
  SmulTask t;
  CallScope call(this);
  DevBuf<Aff>&dp = t0_.a0, &dout = t0_.a1;
  DevBuf<Fr>& dsc = t0_.fr;
  DevBuf<SmulTask>& dt = t0_.stask;
  const size_t ns = scalar_stride ? n : 1;
  dp.ensure(n);
  dout.ensure(n);
  dsc.ensure(ns);
  dt.ensure(1);
  CPX_HIP(hipMemcpyAsync(dp.p, P, n * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dsc.p, scalars, ns * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  t = SmulTask{nullptr, dp.p, dout.p, dsc.p, scalar_stride ? 1u : 0u, opt_.scale_any_point ? SMUL_PLAIN : 0u};
  CPX_HIP(hipMemcpyAsync(dt.p, &t, sizeof t, hipMemcpyHostToDevice, stream_));
  tick("k_smul", 224.0 * n, (double)n);
  launch_smul(dt.p, 1, (int)n, stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(out, dout.p, n * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  call.finish();
}
// The cross terms of one log round (inner_product_argument.rs:158-161: 4, same_multiscalar_argument.rs:107-112: 6) as ONE call: `count`
// independent MSMs of ragged lengths, all of them tasks of the endomorphism bucket-list path in one launch each — k_to_table_endo +
// k_msm_tblw<2, true> over count tasks, k_reduce_sets over their count * 32 * slices bucket sets, k_msm_tail with one output per task,
// k_finalize for the compressed form — between one upload and one download, with one stream synchronisation whatever the count.  Where
// every task lives in the scratch is written down in tier0_plan.hpp; option msm_endo_min is not consulted (the windowed accumulation
// has no place in a call whose point is the shared launch).
void Engine::msm_many(size_t count, const uint32_t* lens, const uint8_t* bases, const uint8_t* scalars, uint8_t* out_jac, uint8_t* out_comp) {
  if (!count) return;
  Tier0MsmPlan pl;
  if (!tier0_msm_plan(count, lens, pl)) throw ArgError("cpx_g1_msm_many: at most 2^16 MSMs and 2^24 points per call");
  if (!out_jac && !out_comp) return;
  msm_lists(pl, lens, bases, scalars, out_jac, out_comp);
}
// ... and its body, which cpx_g1_msm takes with a plan of one task: the upload, the device chain below, the download
void Engine::msm_lists(Tier0MsmPlan& pl, const uint32_t* lens, const uint8_t* bases, const uint8_t* scalars, uint8_t* out_jac, uint8_t* out_comp) {
  const size_t count = pl.count, np = pl.points;
  std::vector<MsmTask> tasks;
  CallScope call(this);
  pl.slices = msm_tblw_slices(opt_, (int)count, 2, (int)pl.max_n);   // one value for every task of the call
  DevBuf<Aff>&db = t0_.a0, &daff = t0_.a1;
  DevBuf<Fr>& ds = t0_.fr;
  DevBuf<Jac>& res = t0_.res;
  DevBuf<uint8_t>& dcomp = t0_.bytes;
  db.ensure(std::max<size_t>(np, 1));
  ds.ensure(std::max<size_t>(np, 1));
  res.ensure(count);
  msm_chain_reserve(pl);
  if (np) {
    CPX_HIP(hipMemcpyAsync(db.p, bases, np * sizeof(Aff), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(ds.p, scalars, np * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  msm_chain(pl, lens, db.p, ds.p, res.p, tasks);
  if (out_jac) CPX_HIP(hipMemcpyAsync(out_jac, res.p, count * sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  if (out_comp) {
    daff.ensure(count);
    dcomp.ensure(count * 48);
    tick("k_finalize", 0, (double)count);
    launch_finalize(res.p, (int)count, daff.p, nullptr, dcomp.p, stream_);
    tock();
    CPX_HIP(hipMemcpyAsync(out_comp, dcomp.p, count * 48, hipMemcpyDeviceToHost, stream_));
  }
  call.finish();
}
// The device half of the bucket-list MSM for a plan whose slices are set, inside the caller's scope: the scratch every task of the plan
// needs beside its bases, scalars and results (reserved before the call's first launch: ensure() may free a buffer) ...
void Engine::msm_chain_reserve(const Tier0MsmPlan& pl) {
  t0_.mtask.ensure(pl.count);
  t0_.ttask.ensure(pl.count);
  t0_.conv.ensure(std::max<size_t>(pl.conv_entries(), 1));
  t0_.dig.ensure(std::max<size_t>(pl.digit_words(), 1));
  t0_.part.ensure(pl.sets());
  main_.ensure(pl.sets(), 0);
}
// ... and the chain launch_msm_endo -> reduce_sets -> launch_msm_tail on bases and scalars that are on the device already, task i of lens[i]
// points at offset pl.conv_off[i] of both; d_res receives pl.count sums in Jacobian standard form.  `tasks` is the caller's, declared above
// its scope (an enqueued copy reads it).
void Engine::msm_chain(const Tier0MsmPlan& pl, const uint32_t* lens, const Aff* d_bases, const Fr* d_scalars, Jac* d_res, std::vector<MsmTask>& tasks) {
  const size_t count = pl.count;
  tasks.resize(count);
  for (size_t i = 0; i < count; i++) tasks[i] = MsmTask{d_bases + pl.conv_off[i], nullptr, d_scalars + pl.conv_off[i], lens[i], 0, pl.conv_off[i]};
  CPX_HIP(hipMemcpyAsync(t0_.mtask.p, tasks.data(), count * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
  msm_chain_run(pl, t0_.mtask.p, d_res);
}
// ... whose launches take any pl.count uploaded tasks laid out by the plan (task i's conv_off = pl.conv_off[i]; gather lists allowed)
void Engine::msm_chain_run(const Tier0MsmPlan& pl, const MsmTask* d_tasks, Jac* d_res) {
  const size_t count = pl.count, np = pl.points;
  tick("k_msm_tblw<2, true>", 128.0 * np, (double)np);
  launch_msm_endo(d_tasks, (int)count, (int)pl.max_n, t0_.conv.p, t0_.dig.p, t0_.ttask.p, main_.raw.p, main_.rawslot.p, stream_, pl.slices);
  tock();
  reduce_sets(stream_, main_, 0, pl.sets(), t0_.part.p);
  tick("k_msm_tail", 0, (double)count);
  launch_msm_tail(opt_, t0_.part.p, nullptr, d_res, (int)count, 16, 8, stream_, nullptr, 0, pl.tail_dup());
  tock();
}
// The basis folds of one log round (inner_product_argument.rs:177-178: 2 families, same_multiscalar_argument.rs:128-130: 3) as ONE call:
// a SmulTask per family, each with its own gamma shared by its `half` elements, in one launch_smul.  A round's folds are small (3 x 128
// elements at ell = 252), so up to option fold_quad_max elements the launch takes the quad-per-element form (tier0_plan.hpp).
void Engine::fold_many(size_t families, size_t half, uint8_t* PL, const uint8_t* PR, const uint8_t* gammas) {
  if (!families || !half) return;
  if (!tier0_fold_fits(families, half)) throw ArgError("cpx_g1_fold_many: at most 2^24 elements per call");
  fold_lanes(families, half, PL, PR, gammas, tier0_fold_quad_max(families * half, opt_.fold_quad_max, opt_.scale_any_point != 0));
}
// ... and its body, which cpx_g1_fold takes with one family
void Engine::fold_lanes(size_t families, size_t half, uint8_t* PL, const uint8_t* PR, const uint8_t* gammas, long quad_max) {
  const size_t total = families * half;
  std::vector<SmulTask> tasks;
  CallScope call(this);
  DevBuf<Aff>&dl = t0_.a0, &dr = t0_.a1;
  DevBuf<Fr>& dg = t0_.fr;
  DevBuf<SmulTask>& dt = t0_.stask;
  dl.ensure(total);
  dr.ensure(total);
  dg.ensure(families);
  dt.ensure(families);
  const uint32_t fl = opt_.scale_any_point ? SMUL_PLAIN : 0u;
  tasks.resize(families);
  for (size_t f = 0; f < families; f++) tasks[f] = SmulTask{dl.p + f * half, dr.p + f * half, dl.p + f * half, dg.p + f, 0, fl};
  CPX_HIP(hipMemcpyAsync(dl.p, PL, total * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dr.p, PR, total * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dg.p, gammas, families * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dt.p, tasks.data(), families * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
  tick("k_smul", 288.0 * total, (double)total);
  count_smul_quad(launch_smul(dt.p, (int)families, (int)half, stream_, false, quad_max));
  tock();
  CPX_HIP(hipMemcpyAsync(PL, dl.p, total * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  call.finish();
}
// option strict_infinity = 0: the rewrite rule of canon_infinity.hpp into the caller's `store`; with the option set the bytes go through untouched
const uint8_t* Engine::canonical_infinities(const uint8_t* bytes, size_t nbytes, size_t nrec, size_t rec_stride, const std::vector<size_t>& offsets,
                                            std::vector<uint8_t>& store) const {
  return opt_.strict_infinity ? bytes : cpx::canonical_infinities(bytes, nbytes, nrec, rec_stride, offsets, store);
}

int Engine::decompress(const uint8_t* comp, size_t n, uint8_t* out_aff, int check_subgroup, uint8_t* status_out) {
  if (!n) return CPX_OK;
  std::vector<uint8_t> st, canon;
  comp = canonical_infinities(comp, n * 48, n, 48, {0}, canon);
  CallScope call(this);
  DevBuf<uint8_t>&dc = t0_.bytes, &dst = t0_.status;
  DevBuf<Aff>& da = t0_.a0;
  dc.ensure(n * 48);
  dst.ensure(n);
  da.ensure(n);
  CPX_HIP(hipMemcpyAsync(dc.p, comp, n * 48, hipMemcpyHostToDevice, stream_));
  launch_decompress(opt_, dc.p, (int)n, da.p, nullptr, dst.p, check_subgroup, stream_);
  st.resize(n);
  CPX_HIP(hipMemcpyAsync(out_aff, da.p, n * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(st.data(), dst.p, n, hipMemcpyDeviceToHost, stream_));
  call.finish();
  if (status_out) {   // per-point verdicts: the call itself succeeds
    memcpy(status_out, st.data(), n);
    return CPX_OK;
  }
  for (auto s : st)
    if (s) return CPX_ERR_DESERIALIZE;
  return CPX_OK;
}

double Engine::bench_fpmul(int blocks, int iters, int reps) {
  CPX_HIP(hipSetDevice(device_));
  const size_t nth = (size_t)blocks * 256;
  DevBuf<Fp> d;
  d.ensure(2 * nth);
  std::vector<Fp> h(2 * nth);
  for (size_t i = 0; i < 2 * nth; i++) {
    h[i] = Fp::one();
    h[i].v[0] ^= (uint32_t)(i * 2654435761u);
    h[i].v[5] ^= (uint32_t)(i * 40503u);
    h[i].v[11] &= 0x0fffffffu;
  }
  CPX_HIP(hipMemcpy(d.p, h.data(), 2 * nth * sizeof(Fp), hipMemcpyHostToDevice));
  hipEvent_t a, b;
  CPX_HIP(hipEventCreate(&a));
  CPX_HIP(hipEventCreate(&b));
  auto launch = opt_.bench_field == 28 ? launch_bench_f28mul : launch_bench_fpmul;
  launch(d.p, blocks, iters, stream_);   // warm-up
  CPX_HIP(hipEventRecord(a, stream_));
  for (int r = 0; r < reps; r++) launch(d.p, blocks, iters, stream_);
  CPX_HIP(hipEventRecord(b, stream_));
  CPX_HIP(hipStreamSynchronize(stream_));
  float ms = 0;
  CPX_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return (double)nth * 2.0 * iters * reps / (ms * 1e-3);
}

// ---------------------------------------------------------------- batch load
// The public instance of `batch` proofs -> the engine's instance buffers, from host memory (batch_load) or from the device staging area of
// batch_load_begin (batch_load_end: device-to-device, a few hundred microseconds per GB).  Everything is enqueued on the main stream.
void Engine::load_rows(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M, bool from_device) {
  if (!ell_) throw std::logic_error("set_crs first");
  CPX_HIP(hipSetDevice(device_));
  const hipMemcpyKind kind = from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  const SlotMap sm(L_);
  pp_stride_ = 4 * ell_ + sm.count();
  const Aff* pp_before = d_pp_.p;
  const Aff* psrc_before = d_psrc_.p;
  d_pp_.ensure(batch * pp_stride_);
  d_Mjac_.ensure(batch);
  B_ = batch;
  const size_t vb = ell_ * sizeof(Aff);
  // strided 2-D copies: one per instance vector instead of one per proof
  const size_t pitch = pp_stride_ * sizeof(Aff);
  auto rows = [&](Aff* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width, hipMemcpyKind k) {
    CPX_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, batch, k, stream_));
  };
  rows(pp(0), pitch, vec_R, vb, vb, kind);
  rows(pp(0) + ell_, pitch, vec_S, vb, vb, kind);
  rows(pp(0) + 2 * ell_, pitch, vec_T, vb, vb, kind);
  rows(pp(0) + 3 * ell_, pitch, vec_U, vb, vb, kind);
  CPX_HIP(hipMemcpyAsync(d_Mjac_.p, M, batch * sizeof(Jac), kind, stream_));
  // copy 0 of the per-proof tables: M (filled at prove time) | T || O O H O | U || O O O H  (curdleproofs.rs:141-155)
  const size_t NP = np();
  d_ptab_.ensure(batch * (size_t)pcopies_for(batch) * NP);   // (a prove under other options makes sure of its own layout)
  d_psrc_.ensure(batch * NP);
  // build scratch: the 15 doubled copies of every point — of one chunk of the device prover's table build (engine_device.cpp); the host-driven
  // prover, which builds all rows at once, makes sure of its own (batch_prove_tables)
  d_tbltmp_.ensure(table_chunk_rows(batch) * NP * (size_t)(pcopies_for(batch) / 2 - 1));
  const size_t spitch = NP * sizeof(Aff);
  Aff* t = d_psrc_.p;
  rows(t + 1, spitch, vec_T, vb, vb, kind);
  rows(t + 1 + n_, spitch, vec_U, vb, vb, kind);
  // The constants every proof's row carries (the CRS's single points in five slots; the blinder tails O O H O / O O O H behind T and U) are the
  // same for every batch of this CRS: written when the buffers are new, have grown, or the CRS has changed — not on every load
  if (consts_rows_ < batch || pp_before != d_pp_.p || psrc_before != d_psrc_.p) {
    std::vector<Aff> rep(batch * 5);   // (a pitch of 0 is not a valid 2-D copy)
    for (size_t p = 0; p < batch; p++) memcpy(&rep[5 * p], crs_single_, 5 * sizeof(Aff));
    rows(slot(0, SL_H), pitch, reinterpret_cast<const uint8_t*>(rep.data()), 5 * sizeof(Aff), 5 * sizeof(Aff), hipMemcpyHostToDevice);
    std::vector<Aff> tails(batch * 8, Aff::identity());
    for (size_t p = 0; p < batch; p++) tails[8 * p + 2] = tails[8 * p + 7] = crs_single_[0];
    rows(t + 1 + ell_, spitch, reinterpret_cast<const uint8_t*>(tails.data()), 8 * sizeof(Aff), 4 * sizeof(Aff), hipMemcpyHostToDevice);
    rows(t + 1 + n_ + ell_, spitch, reinterpret_cast<const uint8_t*>(tails.data() + 4), 8 * sizeof(Aff), 4 * sizeof(Aff), hipMemcpyHostToDevice);
    CPX_HIP(hipStreamSynchronize(stream_));   // rep / tails leave scope
    consts_rows_ = batch;
  }
}
void Engine::batch_load(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M) {
  load_rows(batch, vec_R, vec_S, vec_T, vec_U, M, false);
  CPX_HIP(hipStreamSynchronize(stream_));   // the caller's buffers are free again
}
// cpx_batch_load_begin / _end (include/cpx.h): the NEXT batch's instance crosses PCIe on an upload stream of its own while the loaded batch is
// being proven and verified; _end makes it the loaded batch with device-to-device copies behind the main stream's last kernel.
void Engine::batch_load_begin(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M) {
  if (!ell_) throw std::logic_error("set_crs first");
  CPX_HIP(hipSetDevice(device_));
  if (!stage_.stream) {
    CPX_HIP(hipStreamCreateWithFlags(&stage_.stream, hipStreamNonBlocking));
    CPX_HIP(hipEventCreateWithFlags(&stage_.uploaded, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&stage_.consumed, hipEventDisableTiming));
  }
  const size_t pts = batch * ell_;
  for (auto* b : {&stage_.R, &stage_.S, &stage_.T, &stage_.U}) b->ensure(pts);
  stage_.M.ensure(batch);
  if (stage_.have_consumed) CPX_HIP(hipStreamWaitEvent(stage_.stream, stage_.consumed, 0));   // the previous staged batch has been copied out
  CPX_HIP(hipMemcpyAsync(stage_.R.p, vec_R, pts * sizeof(Aff), hipMemcpyHostToDevice, stage_.stream));
  CPX_HIP(hipMemcpyAsync(stage_.S.p, vec_S, pts * sizeof(Aff), hipMemcpyHostToDevice, stage_.stream));
  CPX_HIP(hipMemcpyAsync(stage_.T.p, vec_T, pts * sizeof(Aff), hipMemcpyHostToDevice, stage_.stream));
  CPX_HIP(hipMemcpyAsync(stage_.U.p, vec_U, pts * sizeof(Aff), hipMemcpyHostToDevice, stage_.stream));
  CPX_HIP(hipMemcpyAsync(stage_.M.p, M, batch * sizeof(Jac), hipMemcpyHostToDevice, stage_.stream));
  CPX_HIP(hipEventRecord(stage_.uploaded, stage_.stream));
  stage_.batch = batch;
  stage_.ell = ell_;
}
void Engine::batch_load_end() {
  if (!stage_.batch) throw std::logic_error("batch_load_begin first");
  if (stage_.ell != ell_) {
    stage_.batch = 0;
    throw std::logic_error("the CRS changed between batch_load_begin and batch_load_end");
  }
  CPX_HIP(hipSetDevice(device_));
  CPX_HIP(hipEventSynchronize(stage_.uploaded));   // the caller's host buffers are free again when this call returns
  const size_t batch = stage_.batch;
  stage_.batch = 0;
  load_rows(batch, reinterpret_cast<const uint8_t*>(stage_.R.p), reinterpret_cast<const uint8_t*>(stage_.S.p), reinterpret_cast<const uint8_t*>(stage_.T.p),
            reinterpret_cast<const uint8_t*>(stage_.U.p), reinterpret_cast<const uint8_t*>(stage_.M.p), true);
  CPX_HIP(hipEventRecord(stage_.consumed, stream_));
  stage_.have_consumed = true;
}

// ---------------------------------------------------------------- prover
void Engine::batch_prove(const uint32_t* permutation, const uint8_t* k_in, const uint8_t* m_blinders, const uint8_t* rand, uint8_t* proofs_out) {
  if (!B_) throw std::logic_error("batch_load first");
  if (device_prefix(B_)) batch_prove_device(ProveDraws{permutation, k_in, m_blinders, hipMemcpyHostToDevice, rand, nullptr, nullptr}, proofs_out);   // the whole protocol on the GPU (engine_device.cpp)
  else batch_prove_tables(permutation, k_in, m_blinders, rand, proofs_out);                  // a few proofs: host-driven Fiat-Shamir
}

// ---------------------------------------------------------------- all-MSM prover over shifted-base tables
// Same protocol, same outputs, different evaluation order of the group arithmetic.  The reference folds the
// bases every round (inner_product_argument.rs:174-179, same_multiscalar_argument.rs:126-131) and takes MSMs
// over the folded bases.  A folded base is a known linear combination of ORIGINAL bases,
//     G^(j)_i = sum_t S^(j)_t * G_(t * n/2^j + i),   S^(j)_t = prod_{m<=j} gamma_m^(bit_(j-m) of t)
// (doc/optimizations.md "IPA verification scalars"), so every cross term L/R of round j is an MSM over the n/2
// original bases whose index has bit (L-j) set / clear, with scalars  vector_entry * S  (and * u_k for the
// rescaled basis G' = u o G of grand_product_argument.rs:90-102, which is never materialised).  Likewise every
// commitment (B, D, cm_T, cm_A, A', ...) expands into an MSM over CRS / instance points.  Hence: no basis
// folds, no per-round normalisation, every MSM runs on pre-shifted tables (k_msm_tbl) without a doubling tail.
// The side and table streams of the host-driven prover: their kernels (a few long single-wave groups: the doubling chains of the table
// build and of the MSM tails) run BESIDE the phases of the main stream, and the dispatcher likes to put the main stream's single-wave
// groups onto the very SIMDs those long waves occupy — two 200-VGPR waves then time-share one SIMD and a 120 us reduction took
// 370 us.  The queues of these streams are therefore confined to the upper half of the CU mask (hipExtStreamCreateWithCUMask); the
// main stream, unconfined, fills the GPU from the low end.  Option cu_mask = 0 creates plain streams (A/B runs).
hipStream_t Engine::create_masked_stream(bool upper) {
  hipStream_t st = nullptr;
  hipDeviceProp_t prop;
  CPX_HIP(hipGetDeviceProperties(&prop, device_));
  const int ncu = prop.multiProcessorCount;
  if (!opt_.cu_mask || ncu < 64) {
    CPX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    return st;
  }
  std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
  for (int cu = upper ? ncu / 2 : 0; cu < (upper ? ncu : ncu / 2); cu++) mask[(size_t)cu / 32] |= 1u << (cu % 32);
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) {
    (void)hipGetLastError();
    CPX_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  }
  return st;
}
namespace {
// the engine's main stream replaced for the lifetime of the guard; work already queued on the old stream is waited for, and the old
// stream waits for the new one at the end
struct StreamSwap {
  hipStream_t& ref;
  hipStream_t saved;
  hipEvent_t ev;
  StreamSwap(hipStream_t& r, hipStream_t s, hipEvent_t e) : ref(r), saved(r), ev(e) {
    if (!s) return;
    (void)hipEventRecord(ev, saved);
    (void)hipStreamWaitEvent(s, ev, 0);
    ref = s;
  }
  ~StreamSwap() {
    if (ref == saved) return;
    (void)hipEventRecord(ev, ref);
    (void)hipStreamWaitEvent(saved, ev, 0);
    ref = saved;
  }
};
}  // namespace

void Engine::batch_prove_tables(const uint32_t* permutation, const uint8_t* k_in, const uint8_t* m_blinders, const uint8_t* rand, uint8_t* proofs_out) {
  HostSpan wall(this, "host_prove_wall");
  CPX_HIP(hipSetDevice(device_));
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  if (!side_.lat_stream) {
    side_.lat_stream = create_masked_stream(true);
    side_.lat_main = create_masked_stream(false);
    CPX_HIP(hipEventCreateWithFlags(&side_.lat_ev, hipEventDisableTiming));
  }
  const hipStream_t sside = side_.lat_stream;
  TeamScope team(this, B);   // 2 ... device_min_batch - 1 (55) proofs: the host loops between the phases on spinning helper threads
  StreamSwap lat_main(stream_, B <= 8 ? side_.lat_main : nullptr, side_.lat_ev);   // a few proofs: the phases on the lower half of the CUs
  const SlotMap sm(L);
  const RandIdx ri((int)n);
  const PtabRow row(n);
  const size_t nrand = ri.count();
  const size_t NP = np();
  std::vector<host::ProveState> st(B);
  std::vector<uint8_t> comp;
  const int ni = (int)n, Li = (int)L;
  // where a request's scalars are staged from: the proof's host state (make_reqs points the round phases at d_rout_ itself)
  const ScalAt scal = [&](size_t p, const ReqScal& sc) {
    const host::ProveState& s = st[p];
    return ScalAddr{sc.kind == SCAL_RAND ? &s.rnd[(size_t)sc.at] : sc.kind == SCAL_VEC ? s.vec[sc.at].data() : &s.sc[sc.at], nullptr};
  };
  int side_slots[6];   // R, S and the four T_2 commitments: the side stream's
  side_stream_slots(Li, side_slots);

  // -- P0: compressed instance vectors, M -> affine (into table slot 0), then the per-proof tables.  The transcript
  //    prefix (instance + M absorbed, vec_a drawn) is hashed on the side stream while the tables are built.
  h_inst_comp_.ensure(B * 4 * ell * 48);   // pinned and persistent: no page faults, true async copies
  h_mcomp_.ensure(B * 48);
  h_u32_.ensure(B);
  const uint8_t* inst_comp = h_inst_comp_.p;
  {
    d_bytes_.ensure(B * 4 * ell * 48);
    tick("k_compress", 0, (double)(4 * ell * B));
    launch_compress(d_pp_.p, (int)(4 * ell), (int)pp_stride_, (int)B, d_bytes_.p, stream_);
    tock();
    d_dst_.ensure(B);
    d_mcomp_.ensure(B * 48);
    uint32_t* dst = h_u32_.p;
    for (size_t p = 0; p < B; p++) dst[p] = (uint32_t)(p * NP + row.M());
    CPX_HIP(hipMemcpyAsync(d_dst_.p, dst, B * 4, hipMemcpyHostToDevice, stream_));
    launch_finalize(d_Mjac_.p, (int)B, d_psrc_.p, d_dst_.p, d_mcomp_.p, stream_);
    transcript_prefix_async(B);   // side stream: copies of the compressed bytes for the host's transcripts
    // the per-proof tables on the table stream: M's row first (phase 2 needs it: B = A + alpha M + ...), then T and U (needed from
    // SameMSM step 1 on), beside phase 1 instead of in front of it
    if (!tab_.stream) {
      tab_.stream = create_masked_stream(true);
      CPX_HIP(hipEventCreateWithFlags(&tab_.ev_start, hipEventDisableTiming));
      CPX_HIP(hipEventCreateWithFlags(&tab_.ev_m, hipEventDisableTiming));
      CPX_HIP(hipEventCreateWithFlags(&tab_.ev_done, hipEventDisableTiming));
    }
    // (the host-driven prover reads its tables through the lone-proof and small-batch kernels: one-segment tables of copies_ copies, whatever
    // layout batch_load sized the buffer for)
    pcopies_ = copies_;
    d_ptab_.ensure(B * (size_t)copies_ * NP);
    d_tbltmp_.ensure(B * NP * (size_t)(copies_ / 2 - 1));   // (all rows in two launches; load_batch sized the scratch for the device prover's chunks: a no-op below 3072 proofs)
    CPX_HIP(hipEventRecord(tab_.ev_start, stream_));
    CPX_HIP(hipStreamWaitEvent(tab_.stream, tab_.ev_start, 0));
    const size_t tmp_m = B * (size_t)(copies_ / 2 - 1);   // scratch entries of the M launch; the T | U launch takes the rest
    launch_table_build(opt_, d_psrc_.p, NP, d_ptab_.p, (int)B, (size_t)copies_ * NP, 1, (int)NP, copies_, true, d_tbltmp_.p, tab_.stream);
    CPX_HIP(hipEventRecord(tab_.ev_m, tab_.stream));
    launch_table_build(opt_, d_psrc_.p + row.T(), NP, d_ptab_.p + row.T(), (int)B, (size_t)copies_ * NP, (int)(2 * n), (int)NP, copies_, true, d_tbltmp_.p + tmp_m, tab_.stream);
    const uint8_t* mcomp = h_mcomp_.p;
    wait_side();
    parallel_for(B, [&](size_t p) {
      host::prove_begin(st[p], ell, L, rand + p * nrand * 32, k_in + 32 * p, permutation + p * ell, &inst_comp[p * 4 * ell * 48], &mcomp[p * 48]);
    });
  }

  // -- side stream: R = a x vec_R and S = a x vec_S (curdleproofs.rs:112-113).  The instance points R_i, S_i are
  //    used by exactly these MSMs, so they get no table: the endomorphism bucket-list kernel (the verifier's) + tails off the
  //    critical path; the affine results land in the slots SL_R / SL_S.
  //    The four scalar multiplications k R, k S (curdleproofs.rs:115-116), r_k R, r_k S (same_scalar_argument.rs:60-61) ride along
  //    as four more MSMs over the same points with the scalars k a and r_k a: k (a x vec_R) = (k a) x vec_R.  A 255-bit
  //    double-and-add chain of one lane (k_smul: 4.6 ms) was what a lone proof waited for at the SameScalar step; as MSM tasks
  //    they run beside R and S and finish with them.
  const int CW0 = SL_CMT1, CWN = sm.CMB2() - SL_CMT1 + 1;   // slot window compressed on the side stream
  {
    const size_t nt = 6 * B, total = B * ell;
    side_.scal.ensure(3 * total);
    side_.tasks.ensure(nt);
    side_.res.ensure(nt);
    side_.dst.ensure(2 * nt);
    side_.comp.ensure(B * (size_t)CWN * 48);
    side_.hcomp.ensure(B * (size_t)CWN * 48);
    const size_t o_tasks = 3 * total * sizeof(Fr), o_dst = o_tasks + nt * sizeof(MsmTask);
    side_.stage.ensure(o_dst + 2 * nt * sizeof(uint32_t));
    Fr* hs = reinterpret_cast<Fr*>(side_.stage.p);
    MsmTask* ht = reinterpret_cast<MsmTask*>(side_.stage.p + o_tasks);
    uint32_t* hd = reinterpret_cast<uint32_t*>(side_.stage.p + o_dst);   // [nt] destination slots, [nt] addend slots
    parallel_for(B, [&](size_t p) {
      host::prove_side_scalars(st[p], ell, hs + p * ell, hs + total + p * ell, hs + 2 * total + p * ell);
      // tasks [0, 2B): R, S; tasks [2B, 6B): k R, k S, r_k R, r_k S (finalised later, on top of the r H points of phase 1)
      for (int j = 0; j < 6; j++) {
        const size_t t = j < 2 ? 2 * p + j : 2 * B + 4 * p + (j - 2);
        const Fr* sc = side_.scal.p + (size_t)(j / 2) * total + p * ell;
        ht[t] = MsmTask{pp(p) + (j & 1) * ell, nullptr, sc, (uint32_t)ell, 0, (uint32_t)(t * ell)};
        hd[t] = slot_index(p, side_slots[j]);
        hd[nt + t] = j < 2 ? ~0u : slot_index(p, sm.TMP(j - 2));
      }
    });
    CPX_HIP(hipMemcpyAsync(side_.scal.p, hs, 3 * total * sizeof(Fr), hipMemcpyHostToDevice, sside));
    CPX_HIP(hipMemcpyAsync(side_.tasks.p, ht, nt * sizeof(MsmTask), hipMemcpyHostToDevice, sside));
    CPX_HIP(hipMemcpyAsync(side_.dst.p, hd, 2 * nt * sizeof(uint32_t), hipMemcpyHostToDevice, sside));
    const int slices = msm_tblw_slices(opt_, (int)nt, 2, (int)ell);
    side_.conv.ensure(2 * nt * ell);   // per task: points and images
    side_.ttasks.ensure(nt);
    side_.digits.ensure(9 * nt * ell);
    side_.scr.ensure(nt * 32 * slices, nt * 32 * slices);
    launch_rs(nt, 2 * B, slices, false, sside, false);
  }

  // -- table stream: B_t = msm(T_b, vec_r), B_u = msm(U_b, vec_r) (same_multiscalar_argument.rs:81-82) right behind the tables of T and U
  const ReqList p1t = prove_phase1t(ni, Li);
  {
    const size_t nt = p1t.n * B;
    enqueue_tbl_phase(make_reqs(p1t, scal), slot_index(0, sm.TMP(7)), tab_.stage, tab_.blob, tab_.comp, tab_.stream, tab_.scr, false);
    tab_.hcomp.ensure(nt * 48);
    CPX_HIP(hipMemcpyAsync(tab_.hcomp.p, tab_.comp.p, nt * 48, hipMemcpyDeviceToHost, tab_.stream));
    CPX_HIP(hipEventRecord(tab_.ev_done, tab_.stream));
  }

  // -- P1: everything that depends only on vec_a and the prover's randomness
  {
    const ReqList p1 = prove_phase1b(ni, Li).then(prove_phase1(ni, Li));   // A, then what depends on the randomness only
    run_tbl_phase(make_reqs(p1, scal), &comp);
    parallel_for(B, [&](size_t p) {
      host::take(st[p], p1, &comp[p * (size_t)p1.n * 48]);
      host::prove_after_phase1(st[p], ell, permutation + p * ell);
    });
  }

  // -- side stream: cm_T.T_2 = k R + r_t H, cm_U.T_2 = k S + r_u H (curdleproofs.rs:115-116), cm_A.T_2 = r_k R + r_a H,
  //    cm_B.T_2 = r_k S + r_b H (same_scalar_argument.rs:60-61): the four MSM results of the side stream on top of the r*H points
  //    phase 1 left in TMP0..3 (complete by now: the host has taken phase 1's results); needed only at the SameScalar transcript step.
  {
    const size_t nt = 6 * B;
    launch_finalize(side_.res.p + 2 * B, (int)(4 * B), d_pp_.p, side_.dst.p + 2 * B, nullptr, sside, side_.dst.p + nt + 2 * B);
    launch_compress(d_pp_.p + 4 * ell + CW0, CWN, (int)pp_stride_, (int)B, side_.comp.p, sside);
    CPX_HIP(hipMemcpyAsync(side_.hcomp.p, side_.comp.p, B * (size_t)CWN * 48, hipMemcpyDeviceToHost, sside));
    CPX_HIP(hipEventRecord(side_.ev, sside));
  }

  // -- P2: B, A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.rs:134) as a sum of three points of phase 1, and C = msm(G | Hvec, c)
  //    (grand_product_argument.rs:76).
  {
    const ReqList p2 = prove_phase2(ni, Li, false);
    CPX_HIP(hipStreamWaitEvent(stream_, tab_.ev_m, 0));   // M's table row (table stream)
    run_tbl_phase(make_reqs(p2, scal), &comp);
    parallel_for(B, [&](size_t p) {
      host::take(st[p], p2, &comp[p * (size_t)p2.n * 48]);
      host::prove_after_phase2(st[p], ell, m_blinders + p * 4 * 32);
    });
  }

  // -- P3: D, B_d
  h_rvec_.ensure(B * 4 * n);
  h_rfin_.ensure(B * 3);   // c_final, d_final, x_final of every proof
  h_rgam_.ensure(B * 2);
  d_rvec_.ensure(B * 4 * n);
  d_rgam_.ensure(B * 2);
  d_rbeta_.ensure(B);
  d_rout_.ensure(B * (2 * n + 2));
  {
    const ReqList p3 = prove_phase3(ni, Li);
    run_tbl_phase(make_reqs(p3, scal), &comp);
    parallel_for(B, [&](size_t p) {   // the round vectors live on the device from here on: c | d | S_G | S_G'
      host::take(st[p], p3, &comp[p * (size_t)p3.n * 48]);
      host::prove_ipa_setup(st[p], ell, L, h_rvec_.p + p * 4 * n, h_rgam_.p + p);
    });
    CPX_HIP(hipMemcpyAsync(d_rvec_.p, h_rvec_.p, B * 4 * n * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(d_rbeta_.p, h_rgam_.p, B * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    wait_stream();   // h_rgam_ is reused for the round challenges
  }

  // -- P5: IPA rounds as MSMs over the original bases.  The Fr side of a round (cross-term scalars, inner products,
  //    folds of c and d, fold-coefficient updates) runs on the device (k_ipa_round_scalars / k_ipa_round_fold); the
  //    host hashes the four points of the round and returns gamma, gamma^-1.
  for (size_t j = 0; j < L; j++) {
    const size_t half = n >> (j + 1);
    const ReqList rd = prove_ipa_round(ni, Li, (int)j, false);
    launch_ipa_round_scalars(d_rvec_.p, (int)B, (int)n, (int)half, d_rbeta_.p, d_rout_.p, stream_);
    run_tbl_phase(make_reqs(rd, scal), &comp);
    parallel_for(B, [&](size_t p) {
      host::take(st[p], rd, &comp[p * (size_t)rd.n * 48]);
      host::prove_ipa_round(st[p], L, (int)j, h_rgam_.p + 2 * p);
    });
    CPX_HIP(hipMemcpyAsync(d_rgam_.p, h_rgam_.p, B * 2 * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    launch_ipa_round_fold(d_rvec_.p, (int)B, (int)n, (int)half, d_rgam_.p, stream_);
    if (j + 1 == L) {   // c_final, d_final (inner_product_argument.rs:188-195)
      CPX_HIP(hipMemcpy2DAsync(h_rfin_.p, 3 * sizeof(Fr), d_rvec_.p, 4 * n * sizeof(Fr), sizeof(Fr), B, hipMemcpyDeviceToHost, stream_));
      CPX_HIP(hipMemcpy2DAsync(h_rfin_.p + 1, 3 * sizeof(Fr), d_rvec_.p + n, 4 * n * sizeof(Fr), sizeof(Fr), B, hipMemcpyDeviceToHost, stream_));
      wait_stream();
    }
    // no sync otherwise: h_rgam_ is rewritten only after the next round's run_tbl_phase has synchronised the stream
  }

  // -- P6 (host only): SameScalar transcript, SameMSM step 1
  {
    wait_side();   // R, S and the four T_2 commitments from the side stream
    {
      HostSpan w(this, "host_wait_device");
      CPX_HIP(hipEventSynchronize(tab_.ev_done));   // the tables of T and U, B_t and B_u from the table stream
    }
    CPX_HIP(hipStreamWaitEvent(stream_, tab_.ev_done, 0));
    parallel_for(B, [&](size_t p) {   // c[0], d[0] after the last fold; the round vectors x | S_M for the device
      host::take(st[p], p1t, tab_.hcomp.p + p * (size_t)p1t.n * 48);   // B_t, B_u
      host::take(st[p], side_slots, 6, side_.hcomp.p + p * (size_t)CWN * 48, CW0);
      host::prove_smsm_setup(st[p], ell, L, h_rfin_.p[3 * p], h_rfin_.p[3 * p + 1], &inst_comp[p * 4 * ell * 48], crs_H_comp_, h_rvec_.p + p * 2 * n);
    });
    CPX_HIP(hipMemcpyAsync(d_rvec_.p, h_rvec_.p, B * 2 * n * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }

  // -- P7: SameMSM rounds; the Fr side (cross-term scalars, fold of x, fold-coefficient update) on the device
  for (size_t j = 0; j < L; j++) {
    const size_t half = n >> (j + 1);
    const ReqList rd = prove_smsm_round(ni, Li, (int)j);
    launch_smsm_round_scalars(d_rvec_.p, (int)B, (int)n, (int)half, d_rout_.p, stream_);
    run_tbl_phase(make_reqs(rd, scal), &comp);
    parallel_for(B, [&](size_t p) {
      host::take(st[p], rd, &comp[p * (size_t)rd.n * 48]);
      host::prove_smsm_round(st[p], L, (int)j, h_rgam_.p + 2 * p);
    });
    CPX_HIP(hipMemcpyAsync(d_rgam_.p, h_rgam_.p, B * 2 * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    launch_smsm_round_fold(d_rvec_.p, (int)B, (int)n, (int)half, d_rgam_.p, stream_);
    if (j + 1 == L) {   // x_final (same_multiscalar_argument.rs:138-141)
      CPX_HIP(hipMemcpy2DAsync(h_rfin_.p + 2, 3 * sizeof(Fr), d_rvec_.p, 2 * n * sizeof(Fr), sizeof(Fr), B, hipMemcpyDeviceToHost, stream_));
      wait_stream();
    }
  }

  // -- serialise (x[0] after the last fold: the device-resident vector)
  const size_t psz = ProofLayout(L).size();
  parallel_for(B, [&](size_t p) { host::prove_serialize(st[p], L, h_rfin_.p[3 * p + 2], proofs_out + p * psz); });
  if (opt_.trace)
    for (int i = 0; i < SC_COUNT; i++)
      if (kScNames[i]) trace_scalar(kScNames[i], st[0].sc[i].f);
  flush_timers();
}

// ---------------------------------------------------------------- verifier
void Engine::batch_verify(const uint8_t* proofs, const uint8_t* rand, int* verdict) { verify_core(proofs, rand, VF_COUNT, verdict, nullptr, nullptr); }
void Engine::batch_verify_fused(const uint8_t* proofs, const uint8_t* rand, uint8_t* partial_jac, int* n_invalid) {
  verify_core(proofs, rand, VF_FUSED_COUNT, nullptr, partial_jac, n_invalid);
}

void Engine::batch_verify_grouped(const uint8_t* proofs, const uint8_t* rand, int* verdict, size_t* n_rechecked) {
  size_t rechecked = 0;
  verify_core(proofs, rand, VF_FUSED_COUNT, verdict, nullptr, nullptr, &rechecked);
  if (n_rechecked) *n_rechecked = rechecked;
}

// One proof's scalars of the accumulated check (host_verify.hpp verify_scalars) into the staging copy of the layout of check_plan.hpp.  An
// undecodable proof contributes nothing to a sum it is part of; in every mode its verdict comes from its flag.
static void stage_check_scalars(const host::VerifyState& s, size_t p, const CheckPlan& cp, const CheckScalars<Fr>& at) {
  Fr* d = at.of_proof(p);
  Fr* c = at.crs_of(p);
  for (size_t i = 0; i < cp.NI; i++) d[i] = s.bad ? S::zero().f : s.scal[1][i].f;
  for (size_t j = 0; j < cp.NM; j++) d[cp.NI + j] = s.bad ? S::zero().f : s.scal[2][j].f;
  for (size_t i = 0; i < cp.n; i++) c[i] = s.bad ? S::zero().f : s.scal[0][i].f;
}
// CRS scalar i summed over the proofs [first, first + count) (the shared bases G | Hvec merge in Fr; msm_accumulator.rs:47-51)
static S crs_sum(const std::vector<host::VerifyState>& st, size_t i, size_t first, size_t count) {
  S t = S::zero();
  for (size_t p = first; p < first + count; p++)
    if (!st[p].bad) t += st[p].scal[0][i];
  return t;
}

// Shared body.  Per-proof mode (verdict != nullptr, 8 random factors per proof): curdleproofs.rs:197.  Fused mode
// (fused_partial != nullptr, 12 factors per proof): BASELINE config 5 — every check of every proof goes into ONE
// accumulated MSM (the reference's MsmAccumulator shared by all verify calls); the result is this
// engine's partial sum, which must add up to the identity over all engines / GPUs.
// Grouped mode (grouped != nullptr, verdict != nullptr, 12 factors per proof): the fused check stopped one level earlier — every group's sum is
// tested, and the proofs of the failing groups get their own check from the same scalars (locate_plan.hpp); *grouped = proofs rechecked.
void Engine::verify_core(const uint8_t* proofs, const uint8_t* rand, size_t rand_stride, int* verdict, uint8_t* fused_partial, int* fused_invalid, size_t* grouped) {
  HostSpan wall(this, "host_verify_wall");
  if (!B_) throw std::logic_error("batch_load first");
  CPX_HIP(hipSetDevice(device_));
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  const SlotMap sm(L);
  const ProofLayout pl(L);
  const size_t psz = pl.size();
  const int NPP = pl.n_points();
  // msm_accumulator.rs:44 draws every factor with Fr::rand; the ABI takes them from the caller, so they are validated:
  // a zero (or non-reduced) factor would silently drop the check it weights
  for (size_t i = 0; i < B * rand_stride; i++)
    if (!host::is_valid_factor(rand + 32 * i)) throw ArgError("verifier random factors must be non-zero reduced field elements");
  std::vector<uint8_t> canon;   // (read until the call ends)
  {   // infinity encodings as ark-bls12-381 ^0.4 reads them (option strict_infinity = 0): canonical before anything hashes or decodes them
    std::vector<size_t> offs((size_t)NPP);
    for (int q = 0; q < NPP; q++) offs[q] = pl.point_offset(q);
    proofs = canonical_infinities(proofs, B * psz, B, psz, offs, canon);
  }
  if (device_prefix(B)) {   // the whole verifier on the GPU (engine_device.cpp); a few proofs: host-driven Fiat-Shamir below
    verify_core_device(proofs, rand, rand_stride, verdict, fused_partial, fused_invalid, grouped);
    return;
  }

  TeamScope team(this, B);   // 2 ... device_min_batch - 1 (55) proofs: the host loops on spinning helper threads
  std::vector<host::VerifyState> st(B);

  // -- V0: compressed instance vectors and M -> affine first (the transcript starts with their bytes: the side stream copies them
  //    to the host), then the proof points are decompressed into their slots — the host hashes (V1a) while that kernel runs
  h_inst_comp_.ensure(B * 4 * ell * 48);
  h_mcomp_.ensure(B * 48);
  const uint8_t* inst_comp = h_inst_comp_.p;
  const uint8_t* mcomp = h_mcomp_.p;
  const size_t npts = (size_t)B * NPP;
  {
    h_pts_.ensure(npts * 48);
    h_u32_.ensure(npts + B);
    h_status_.ensure(npts);
    uint8_t* pts = h_pts_.p;
    uint32_t* dst = h_u32_.p;
    d_bytes_.ensure(B * 4 * ell * 48);
    tick("k_compress", 0, (double)(4 * ell * B));
    launch_compress(d_pp_.p, (int)(4 * ell), (int)pp_stride_, (int)B, d_bytes_.p, stream_);
    tock();
    d_dst_.ensure(B);
    d_comp_.ensure(B * 48);
    uint32_t* mdst = h_u32_.p + npts;
    for (size_t p = 0; p < B; p++) mdst[p] = slot_index(p, SL_M);
    d_mcomp_.ensure(B * 48);
    CPX_HIP(hipMemcpyAsync(d_dst_.p, mdst, B * 4, hipMemcpyHostToDevice, stream_));
    launch_finalize(d_Mjac_.p, (int)B, d_pp_.p, d_dst_.p, d_mcomp_.p, stream_);
    transcript_prefix_async(B);   // side stream: copies of the compressed bytes for the host's transcripts
    parallel_for(B, [&](size_t p) {
      for (int q = 0; q < NPP; q++) {
        memcpy(&pts[(p * NPP + q) * 48], proofs + p * psz + pl.point_offset(q), 48);
        dst[p * NPP + q] = slot_index(p, SL_A + q);
      }
    });
    d_vin_.ensure(npts * 48);
    d_vdst_.ensure(npts);
    d_status_.ensure(npts);
    CPX_HIP(hipMemcpyAsync(d_vin_.p, pts, npts * 48, hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(d_vdst_.p, dst, npts * 4, hipMemcpyHostToDevice, stream_));
    tick("k_decompress", 0, (double)npts);
    launch_decompress(opt_, d_vin_.p, (int)npts, d_pp_.p, d_vdst_.p, d_status_.p, 1, stream_);
    tock();
    CPX_HIP(hipMemcpyAsync(h_status_.p, d_status_.p, npts, hipMemcpyDeviceToHost, stream_));
    wait_side();
  }

  std::vector<uint8_t> comp;
  const ReqList vreqs = verify_requests((int)n, (int)L);   // D, A'

  // -- V1a: transcript up to the grand-product beta
  parallel_for(B, [&](size_t p) { host::verify_prefix(st[p], ell, L, proofs + p * psz, &inst_comp[p * 4 * ell * 48], &mcomp[p * 48]); });
  {   // the decompressed proof points (and their verdicts) are needed from here on
    wait_stream();
    const uint8_t* status = h_status_.p;
    for (size_t p = 0; p < B; p++)
      for (int q = 0; q < NPP; q++)
        if (status[p * NPP + q]) st[p].bad = true;
  }

  // -- V1b: D = B - beta^-1 sum(G) + alpha sum(H) (grand_product_argument.rs:223) and A' = A + cm_T.T_1 + cm_U.T_1
  //    (curdleproofs.rs:258) are hashed into the transcript, so they are needed as bytes: sums of decompressed proof
  //    points plus two fixed-base terms (G_sum, H_sum are columns of the CRS tables)
  {
    // (after verify_prefix scal[0] holds the coefficients of D's three terms, 1 for the addend B first)
    run_tbl_phase(make_reqs(vreqs, [&](size_t p, const ReqScal&) { return ScalAddr{st[p].scal[0].data() + 1, nullptr}; }), &comp);
  }

  // -- V1c: rest of the transcript and the scalars of the accumulated check; its "misc" part runs over the CRS singles, M and every
  //    proof point: the slots 0 .. NM (check_plan.hpp)
  auto comp_of = [&](size_t p, int slot) -> const uint8_t* {   // the bytes of the request whose output is `slot`
    for (int i = 0; i < vreqs.n; i++)
      if (vreqs.r[i].out == slot) return &comp[(p * (size_t)vreqs.n + i) * 48];
    throw std::logic_error("no verifier request writes this slot");
  };
  parallel_for(B, [&](size_t p) {
    host::verify_scalars(st[p], ell, L, &inst_comp[p * 4 * ell * 48], crs_H_comp_, comp_of(p, sm.D()), comp_of(p, sm.APRIME()), rand + p * rand_stride * 32,
                         fused_partial != nullptr || grouped != nullptr);
  });

  // -- V2: the accumulated check (check_plan.hpp) — the CRS part on the fixed-base table (k_msm_fix), the per-proof points (R | S | T | U
  //    and the slots) in bucket MSMs (k_msm_tblw<2, true>); the Horner tail adds the two.  Per proof: one task pair per proof.  Fused: ONE
  //    sum, the CRS scalars summed over the proofs, the points in up to 256 groups.  Grouped: stage 1 = one task pair per group, the CRS
  //    scalars summed per group; stage 2 = one task pair per suspect proof over the scalars already on the device (located_check).
  if (!fixtab()) throw std::logic_error("set_crs first");
  const bool fused = fused_partial != nullptr, global = fused || grouped;   // global: tasks over ranges of the batch's points (gather list)
  std::vector<uint32_t> flags(B);
  for (size_t p = 0; p < B; p++) flags[p] = (st[p].bad ? kLocateFlagDecode : 0u) | (st[p].reject ? kLocateFlagStruct : 0u);
  CheckPlan cp(B, ell, L, n);
  const size_t NPT = cp.NPT, N = cp.n_points();
  const LocatePlan lp = grouped ? locate_plan(B, opt_.locate_groups_max) : CheckPlan::fused_plan(B);   // (per proof: unused)
  const size_t NT = global ? lp.NT : B;                     // stage 1's bucket MSM tasks
  const size_t NF = fused ? 1 : NT;                         // ... and fixed-base tasks
  const size_t rows = grouped ? lp.NT : fused ? 1 : 0;      // rows of summed CRS scalars
  const size_t n2 = grouped ? B : 0;                        // room for stage 2's tasks behind stage 1's
  // device scalars: [ per-proof points' scalars (N) | per-proof CRS scalars (B n) | summed CRS scalars (rows n) ]
  const size_t o_crs = N, o_sum = N + B * n, total = o_sum + rows * n;
  const int fix_wpw = msm_fix_windows_per_wave(opt_, (int)NF, fix_bits_);
  const int fix_parts = msm_fix_parts(fix_bits_, fix_wpw);
  d_scal_.ensure(total);
  d_tasks_.ensure(NT + n2);
  d_ftasks_.ensure(NF + n2);
  if (global) d_big_idx_.ensure(N);
  const size_t b_scal = total * sizeof(Fr), b_mt = NT * sizeof(MsmTask), b_ft = NF * sizeof(FixTask), b_idx = global ? N * sizeof(uint32_t) : 0;
  h_stage_.ensure(b_scal + b_mt + b_ft + b_idx);
  Fr* hs = reinterpret_cast<Fr*>(h_stage_.p);
  MsmTask* hm = reinterpret_cast<MsmTask*>(h_stage_.p + b_scal);
  FixTask* hf = reinterpret_cast<FixTask*>(h_stage_.p + b_scal + b_mt);
  uint32_t* hi = reinterpret_cast<uint32_t*>(h_stage_.p + b_scal + b_mt + b_ft);
  std::vector<uint32_t> all_idx(global ? 0 : NPT);   // per proof: the row-relative gather list — the instance vectors, then the slots of the misc part
  for (size_t i = 0; i < all_idx.size(); i++) all_idx[i] = (uint32_t)i;
  cp.place(d_pp_.p, pp_stride_, global ? nullptr : idx_list(all_idx), d_big_idx_.p, d_scal_.p, d_scal_.p + o_crs, d_scal_.p + o_sum);
  const CheckScalars<Fr> at{hs, hs + o_crs, hs + o_sum, NPT, n};   // the staging copy
  parallel_for(B, [&](size_t p) {
    stage_check_scalars(st[p], p, cp, at);
    if (global) cp.gather_proof(p, hi);
  });
  if (rows)   // the CRS scalars summed over all proofs (fused) / per group
    parallel_for(n, [&](size_t i) {
      for (size_t r = 0; r < rows; r++) at.sum_row(r)[i] = crs_sum(st, i, grouped ? lp.group_first(r) : 0, grouped ? lp.group_count(r) : B).f;
    });
  if (grouped) cp.group_tasks(lp, (size_t)fix_parts, hm, hf);
  else if (fused) cp.fused_tasks(hm, hf);
  else cp.proof_tasks((size_t)fix_parts, hm, hf);
  CPX_HIP(hipMemcpyAsync(d_scal_.p, hs, b_scal, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_tasks_.p, hm, b_mt, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_ftasks_.p, hf, b_ft, hipMemcpyHostToDevice, stream_));
  if (global) CPX_HIP(hipMemcpyAsync(d_big_idx_.p, hi, b_idx, hipMemcpyHostToDevice, stream_));
  if (grouped) {
    *grouped = located_check(cp, lp, LocateTasks{d_tasks_.p, d_ftasks_.p, fix_wpw, fix_parts, d_tasks_.p + NT, d_ftasks_.p + NT}, flags.data(), false, verdict);
  } else if (fused) {
    launch_check_fused(d_tasks_.p, d_ftasks_.p, lp.NT, lp.G, NPT, N, fix_wpw, fix_parts);
    wait_stream();
    memcpy(fused_partial, h_comp_.p, sizeof(Jac));
    int invalid = 0;
    for (size_t p = 0; p < B; p++) invalid += flags[p] ? 1 : 0;
    if (fused_invalid) *fused_invalid = invalid;
  } else {
    launch_check(d_tasks_.p, d_ftasks_.p, B, NPT, fix_wpw, fix_parts, (size_t)msm_tblw_slices(opt_, (int)B, 2, (int)NPT));   // a lone proof: several waves per window
    wait_stream();
    for (size_t p = 0; p < B; p++) verdict[p] = check_verdict(flags[p], check_passed(p));
  }
  flush_timers();
}

}  // namespace cpx
