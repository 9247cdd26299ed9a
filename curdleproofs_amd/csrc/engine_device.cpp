// Device-resident batch prover / verifier of the engine — product code (see engine.hpp, protocol.h).
//
// For batches of >= 56 proofs (option device_min_batch) the whole protocol runs on the GPU: the MSM phases read their
// scalars from device memory through task descriptors that are built ONCE per loaded batch shape ("plans"), the
// finalisation kernels leave the compressed results in a per-proof slot registry, and one-wave-per-proof step kernels
// (protocol.hip) hash them into the transcripts and derive the next phase's scalars.  The host only enqueues: no
// synchronisation between cpx_batch_prove's input upload and the download of the proofs.  (Small batches keep the
// host-driven path of engine.cpp: a lone transcript is latency-bound on a GPU wave.)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "engine.hpp"
#include "recode.hpp"

namespace cpx {

// ---------------------------------------------------------------- plans
// Layout of a table-backed MSM phase — the requests of `list` (prove_reqs.hpp) for every proof — whose requests all read device-resident
// scalars (TblReq::dev), by the planner of tbl_plan.hpp; the launches (Engine::launch_tbl_phase) scatter the affine point (TblReq::dst)
// and write the compressed bytes to the request's slot of the registry.
void Engine::build_plan(TblPlan& pl, const ReqList& list, const ScalAt& scal_at) {
  if (!(fix_bits_ && fixtab())) throw std::logic_error("set_crs first");
  std::vector<uint32_t> comp_index;
  const std::vector<TblReq> reqs = make_reqs(list, scal_at, &comp_index);
  for (const TblReq& r : reqs)
    if (!r.dev && (r.seg0.n || r.seg1.n)) throw std::logic_error("device plan: request without device scalars");
  const CrsRange crs{ctab(), ctab() + (size_t)copies_ * nc()};
  tbl_count(reqs, crs, pl);
  pl.fix_wpw = pl.force_fix_wpw ? pl.force_fix_wpw : msm_fix_windows_per_wave(opt_, (int)pl.nft, fix_bits_);
  pl.tbl_wpw = pl.force_tbl_wpw ? pl.force_tbl_wpw : msm_tblw_windows_per_wave(opt_, (int)pl.ntt);
  std::vector<TblTask> ht(pl.ntt);
  std::vector<FixTask> hf(pl.nft);
  std::vector<uint32_t> meta(7 * pl.nt);
  // requests without a destination scatter their affine point to a write-only slot of proof 0 that NOTHING ever reads: TMP(7) for plans of the
  // main stream, TMP(5) for the plan that runs beside them on the table stream (phase 1t) — two streams never write the same slot
  const uint32_t dummy_dst = slot_index(0, SlotMap(L_).TMP(pl.table_stream ? 5 : 7));
  // two-segment per-proof tables: every segment of a table task must be one (the CRS segments all went to the fixed-base kernel)
  pl.tbl_segments = pcopies_ == copies_ ? 1 : 2;
  const uint32_t tbl_parts = (uint32_t)msm_tblw_parts(pl.tbl_wpw, pl.tbl_segments);
  tbl_plan(reqs, crs, (uint32_t)msm_fix_parts(fix_bits_, pl.fix_wpw), tbl_parts, dummy_dst, nullptr, comp_index.data(), pl, ht.data(), hf.data(), meta.data(), nullptr,
           tbw_parts_hi((uint32_t)pl.tbl_wpw, (uint32_t)pl.tbl_segments));   // (one slice: the class-1 partials of a task, which come first)
  if (pl.tbl_segments == 2)
    for (const TblTask& t : ht)
      for (const TblSeg& sg : t.seg)
        if (sg.n && !(sg.base >= d_ptab_.p && sg.base < d_ptab_.p + d_ptab_.cap)) throw std::logic_error("device plan: a table task outside the two-segment per-proof tables");
  // Long tasks first: a work-group's task is its index in these arrays, partial-sum slots travel with the task (out_first / pad).  With the
  // requests in protocol order a launch ended with the long waves of the last proofs and the GPU drained behind them (~0.8 ms of a
  // 7.6-ms k_msm_fix launch at 8192 proofs); now the one-point tasks fill the tail.
  if (!pl.keep_order) {
    std::stable_sort(hf.begin(), hf.end(), [](const FixTask& a, const FixTask& b) { return a.n > b.n; });
    std::stable_sort(ht.begin(), ht.end(), [](const TblTask& a, const TblTask& b) { return a.seg[0].n + a.seg[1].n > b.seg[0].n + b.seg[1].n; });
  }
  pl.ttasks.ensure(std::max<size_t>(pl.ntt, 1));
  pl.ftasks.ensure(std::max<size_t>(pl.nft, 1));
  pl.meta.ensure(std::max<size_t>(meta.size(), 1));
  if (pl.ntt) CPX_HIP(hipMemcpy(pl.ttasks.p, ht.data(), pl.ntt * sizeof(TblTask), hipMemcpyHostToDevice));
  if (pl.nft) CPX_HIP(hipMemcpy(pl.ftasks.p, hf.data(), pl.nft * sizeof(FixTask), hipMemcpyHostToDevice));
  if (pl.nt) CPX_HIP(hipMemcpy(pl.meta.p, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
}

void Engine::exec_plan(const TblPlan& pl, uint8_t* d_comp_registry, bool on_table_stream) {
  // (a plan on the table stream works in the table stream's own scratch, sized by prepare_device_prover: it runs beside the plans
  // of the main stream)
  if (on_table_stream && table_stream_on()) return launch_tbl_phase(pl, pl.ttasks.p, pl.ftasks.p, pl.meta.p, d_comp_registry, tab_.dstream, tab_.scr);
  main_.ensure(pl.fix_sets + pl.tbl_sets, pl.nparts);
  launch_tbl_phase(pl, pl.ttasks.p, pl.ftasks.p, pl.meta.p, d_comp_registry, stream_, main_);
}

// One late round: lane-per-output Straus MSMs over the materialised points, then the usual finalisation (affine, compressed bytes
// into the slot registry; nothing reads these points in affine form again)
void Engine::exec_late_round(const LateRound& r0, size_t comp_off, const char* what) {
  LateRound r = r0;
  const DevProver::Late& lt = dprove_.late;
  r.out = lt.part.p;
  const int nreq = r.total / r.slices, hm = r.m / 2, Bi = r.nproofs;
  const double pairs = (double)nreq * hm;
  tick(what, 128.0 * pairs, pairs);
  launch_late_msm(r, stream_);
  tock();
  const bool ipa = r.nout == 4;
  if (ipa) {   // beta <c_L, d_R> H and beta <c_R, d_L> H (inner_product_argument.rs:152,158) from the table of multiples: the extras of L_C, R_C
    launch_late_fix(d_rout_.p + hm, r.scal_proof_stride, lt.h_col, 1, 1, fixtab(), fix_bits_, (int)nc(), lt.extra.p, 4, Bi, stream_);
    launch_late_fix(d_rout_.p + 3 * hm + 1, r.scal_proof_stride, lt.h_col, 1, 1, fixtab(), fix_bits_, (int)nc(), lt.extra.p + 2, 4, Bi, stream_);
  }
  tick("k_msm_tail", 0, (double)nreq);
  launch_msm_tail(opt_, lt.part.p, main_.part.p, nullptr, nreq, r.slices, 128 / r.slices, stream_, ipa ? lt.extra.p : nullptr, ipa ? 1 : 0);
  tock();
  const uint32_t* meta = lt.meta.p;
  tick("k_finalize_ranges", 0, (double)nreq);
  launch_finalize_ranges(opt_, main_.part.p, meta, meta + 6 * B_, nreq, nullptr, nullptr, dprove_.slotcomp.p, stream_, nullptr, meta + comp_off);
  tock();
}

// ---------------------------------------------------------------- prover
// (Re)builds everything that depends only on the shape of the loaded batch: device buffers, the ProveDev view, the task
// descriptors of every phase and of the side stream.
void Engine::prepare_device_prover() {
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  const SlotMap sm(L);
  const RandIdx ri((int)n);
  const PtabRow row(n);
  const CtabCols cc(n);
  const size_t NS = sm.count(), NP = np(), nrand = ri.count();
  DevProver& dp = dprove_;
  // the layout of the per-proof tables this batch proves with (engine.hpp): part of the plans' signature
  pcopies_ = pcopies_for(B);
  // buffers (sizes only grow; a reallocation changes a pointer and invalidates the plans)
  d_ptab_.ensure(B * (size_t)pcopies_ * NP);   // (batch_load sized it under the options of its time)
  d_bytes_.ensure(B * 4 * ell * 48);
  d_mcomp_.ensure(B * 48);
  d_tstate_.ensure(B * 27);
  d_veca_.ensure(B * ell);
  d_rvec_.ensure(B * 4 * n);
  dp.rvec2.ensure(B * 2 * n);
  d_rgam_.ensure(B * 2);
  d_rbeta_.ensure(B);
  d_rout_.ensure(B * (2 * n + 2));
  dp.perm.ensure(B * ell);
  dp.k.ensure(B);
  dp.mbl.ensure(B * 4);
  dp.rnd.ensure(B * nrand);
  dp.vec.ensure(B * (size_t)V_COUNT * n);
  dp.sc.ensure(B * (size_t)SC_COUNT);
  dp.slotcomp.ensure(B * NS * 48);
  dp.proofs.ensure(B * proof_size());
  dp.mdst.ensure(B);
  side_.tasks.ensure(2 * B);
  side_.stasks.ensure(4 * B);
  side_.res.ensure(2 * B);
  side_.dst.ensure(2 * B);
  side_.ttasks.ensure(2 * B);
  dp.stasks_tbl.ensure(4 * B);
  if (!opt_.rs_from_tables) ensure_rs_scratch();   // (else on demand: a batch that falls back to the bucket MSMs)
  const std::vector<const void*> sig = {d_pp_.p,     d_ptab_.p,    d_psrc_.p,  d_bytes_.p,  d_mcomp_.p,   d_tstate_.p,   d_veca_.p,      d_rvec_.p,
                                        dp.rvec2.p,  d_rgam_.p,    d_rbeta_.p, d_rout_.p,   dp.perm.p,    dp.k.p,        dp.mbl.p,       dp.rnd.p,
                                        dp.vec.p,    dp.sc.p,      dp.slotcomp.p, dp.proofs.p, side_.tasks.p, side_.stasks.p, side_.dst.p, dp.stasks_tbl.p,
                                        ctab(),      fixtab(),     (const void*)(uintptr_t)B, (const void*)(uintptr_t)ell, (const void*)(uintptr_t)fix_bits_,
                                        (const void*)(uintptr_t)pcopies_};
  if (sig == dp.signature) return;
  dp.signature.clear();

  ProveDev& d = dp.dev;
  d.ell = (int)ell;
  d.n = (int)n;
  d.L = (int)L;
  d.NS = (int)NS;
  d.rs_tables = 0;   // (enqueue_prove_device sets it in its copy for the proves that take R and S from the tables)
  d.psz = proof_size();
  d.perm = dp.perm.p;
  d.k = dp.k.p;
  d.mbl = dp.mbl.p;
  d.rnd = dp.rnd.p;
  d.tstate = d_tstate_.p;
  d.veca = d_veca_.p;
  d.vec = dp.vec.p;
  d.sc = dp.sc.p;
  d.slotcomp = dp.slotcomp.p;
  d.inst_comp = d_bytes_.p;
  d.mcomp = d_mcomp_.p;
  d.rvec = d_rvec_.p;
  d.rvec2 = dp.rvec2.p;
  d.rgam = d_rgam_.p;
  d.rbeta = d_rbeta_.p;
  d.proofs = dp.proofs.p;
  memcpy(d.crs_h_comp, crs_H_comp_, 48);

  auto rnd = [&](size_t p, int i) { return dp.rnd.p + p * nrand + i; };
  // where the prover's kernels (protocol.hip) leave the scalars of a request
  const ScalAt scal = [&](size_t p, const ReqScal& sc) {
    const Fr* at = sc.kind == SCAL_RAND ? rnd(p, sc.at) : sc.kind == SCAL_VEC ? dp.vec.p + (p * V_COUNT + sc.at) * n : dp.sc.p + p * SC_COUNT + sc.at;
    return ScalAddr{nullptr, at};
  };
  auto cidx = [&](size_t p, int slot) { return (uint32_t)(p * NS + slot); };
  const int ni = (int)n, Li = (int)L;

  // mdst: where the affine M of proof p goes (table source slot 0)
  {
    std::vector<uint32_t> md(B);
    for (size_t p = 0; p < B; p++) md[p] = (uint32_t)(p * NP + row.M());
    CPX_HIP(hipMemcpy(dp.mdst.p, md.data(), B * 4, hipMemcpyHostToDevice));
  }
  // (decided before the plans are laid out: the phases of a small batch differ, too)
  // the last log2(m) rounds of a large batch work on m materialised folded bases per family instead (late.hip): m = 16 (four rounds) up to
  // n = 256; an all-MSM round of n = 512 / 1024 costs two / four times as much, while materialising costs the same whatever m (every base
  // is visited once) and a late round 32 x (4 + m) operations per cross term: m = 32 (five rounds) pays there — measured per pass of 2048
  // proofs of ell = 1020: m = 16 534.8 ms, m = 32 506.1 ms, m = 64 506.7 ms (six rounds, two k_late_uniform waves per proof: no further gain);
  // 4096 proofs of ell = 508: 500.9 / 475.8 / 495.2 ms; 8192 proofs of ell = 252: 507.4 / 511.2 ms
  DevProver::Late& lt = dp.late;
  const LateShape ls = late_shape(B);   // (engine.cpp: the layout of the per-proof tables depends on it, too)
  lt.m = ls.m;
  lt.nr = ls.nr;
  lt.on = ls.on;
  lt.j0 = lt.on ? L - (size_t)lt.nr : L;
  // fused log rounds (round.hip): every round of both arguments is ONE launch — for the batches in which a round is a chain of latency-bound
  // kernels (below the late rounds' threshold; the 16-bit table of multiples)
  const size_t fused_max = n <= 256 ? (size_t)opt_.fused_rounds_max : (size_t)opt_.fused_rounds_max * 256 / n;
  const size_t fused_smsm_max = n <= 256 ? (size_t)opt_.fused_smsm_max : (size_t)opt_.fused_smsm_max * 256 / n;
  const bool fused_ok = !lt.on && fix_bits_ == 16 && !opt_.serial_streams;
  dp.fused = fused_ok && opt_.fused_rounds_max > 0 && B <= fused_max;
  dp.fused_smsm = fused_ok && opt_.fused_smsm_max > 0 && B <= fused_smsm_max;
  if (dp.fused_smsm && pcopies_ != copies_) throw std::logic_error("fused SameMSM rounds read one-segment tables");   // (smsm_may_fuse() says the same)
  // wave shapes of the fused rounds: as many waves per proof as find a SIMD of their own (1024 SIMDs; proofs of n > 256 take n / 256 times the work)
  const size_t simd_share = 1024 * 256 / (B * std::max<size_t>(n, 256));   // SIMDs per proof
  const int f_fix_ipa = opt_.fused_fix_wpw ? (int)opt_.fused_fix_wpw : (simd_share >= 16 ? 4 : simd_share >= 8 ? 8 : 16);   // 16 / 8 / 4 waves per proof
  // SameMSM: separate fixed-base and table waves (12 per proof) while they find SIMDs of their own; then combined waves — a fixed-base block
  // and a table block per wave — 8 per proof (4 + 16 windows), and 4 per proof (8 + 32 windows) from 129 proofs on
  const bool f_combine = opt_.fused_combine >= 0 ? opt_.fused_combine != 0 : simd_share < 12;
  const bool f_combine4 = f_combine && opt_.fused_combine < 0 && simd_share < 8;
  const int f_fix_smsm = f_combine ? (f_combine4 ? 8 : 4) : std::max(8, opt_.fused_fix_wpw ? (int)opt_.fused_fix_wpw : 8);
  const int f_tbl_smsm = f_combine ? (f_combine4 ? 32 : 16) : (int)opt_.fused_tbl_wpw;
  dp.fused = dp.fused && round_fused_supported(f_fix_ipa, 0, true);
  dp.fused_smsm = dp.fused_smsm && round_fused_supported(f_fix_smsm, f_tbl_smsm, false);
  // -- phase 1: everything that depends only on vec_a and the prover's randomness (curdleproofs.rs:93,110-116,
  //    same_multiscalar_argument.rs:80 (B_a; B_t and B_u are phase 1t), inner_product_argument.rs:126, same_scalar_argument.rs:60-61).
  //    Without the option p1_split, A (phase 1b) leads the phase.
  build_plan(dp.p1, opt_.p1_split ? prove_phase1(ni, Li) : prove_phase1b(ni, Li).then(prove_phase1(ni, Li)), scal);
  // -- phase 1t: B_t = msm(T_b, r), B_u = msm(U_b, r) (same_multiscalar_argument.rs:81-82) — the two commitments of phase 1 over the
  //    per-proof tables.  Nothing reads them before the SameMSM transcript step: they follow the table build on the table stream, and
  //    the main stream goes on with the CRS-only commitments at once
  dp.p1t.table_stream = true;
  build_plan(dp.p1t, prove_phase1t(ni, Li), scal);
  // -- R and S from the tables (option rs_from_tables): k R = msm(T, a_sigma), k S = msm(U, a_sigma) — table requests like phase 1t, behind
  //    it on the same stream once V_APERM is there; then cm_T.T_2 = k R + r_t H, cm_U.T_2 = k S + r_u H as sums of kept points on the side stream
  dp.prs.table_stream = true;
  build_plan(dp.prs, prove_rs_tables(ni, Li), scal);
  build_plan(dp.prs_sum, prove_rs_sums(ni, Li), scal);
  tab_.scr.ensure(std::max(dp.p1t.fix_sets + dp.p1t.tbl_sets, dp.prs.fix_sets + dp.prs.tbl_sets), std::max(dp.p1t.nparts, dp.prs.nparts));
  // -- phase 1b (option p1_split): A = msm(G | Hvec, a_sigma | blinders) (curdleproofs.rs:93) alone — the one commitment of phase 1
  //    that needs vec_a; the rest of the phase then runs before the main stream waits for the transcript prefix
  build_plan(dp.p1b, opt_.p1_split ? prove_phase1b(ni, Li) : ReqList(), scal);
  // -- phase 2: B = A + alpha M + beta sum(G) (same_permutation_argument.rs:75-76), A' = A + cm_T.T_1 + cm_U.T_1
  //    (curdleproofs.rs:134), C = msm(G | Hvec, c) (grand_product_argument.rs:76).
  //    B.  Large batches: A + alpha M + beta sum(G) — two points and an addend.  Fused / small batches: the commitment the reference computes,
  //    msm(G | Hvec, a_sigma + alpha sigma + beta | a_blinders + alpha m_blinders) (same_permutation_argument.rs:75-76; the scalars are the
  //    grand-product factors k_ps_sameperm leaves in V_FACT) — a 256-point task of the fixed-base kernel like C beside it, instead of a
  //    one-point task of the bucket-list kernel whose 32 bucket sets per proof cost the phase 0.5 ms of reductions at 128 proofs
  build_plan(dp.p2, prove_phase2(ni, Li, dp.fused_smsm), scal);
  // -- phase 3: D = B - beta^-1 sum(G) + alpha sum(H) (grand_product_argument.rs:132), B_d = msm(G', r_d) = msm(G, r_d o u)
  build_plan(dp.p3, prove_phase3(ni, Li), scal);
  // -- IPA rounds as MSMs over the original bases; scalars from k_ipa_round_scalars
  dp.ipa.clear();
  dp.smsm.clear();
  for (size_t j = 0; j < L; j++) {
    if (j >= lt.j0) {   // placeholders: exec_late_round takes these rounds
      dp.ipa.emplace_back(nullptr);
      dp.smsm.emplace_back(nullptr);
      continue;
    }
    // (fused rounds: the H term of L_C / R_C rides in the same fixed-base task as the n/2 bases — one more column of the gather list, the
    // scalar beta <c, d> follows the n/2 cross-term scalars in memory anyway — instead of a one-point task of its own: 4 tasks per proof)
    dp.ipa.emplace_back(new TblPlan());
    if (dp.fused) {
      dp.ipa.back()->keep_order = true;
      dp.ipa.back()->force_fix_wpw = f_fix_ipa;
    }
    build_plan(*dp.ipa.back(), prove_ipa_round(ni, Li, (int)j, dp.fused), scal);
    dp.smsm.emplace_back(new TblPlan());
    if (dp.fused_smsm) {
      dp.smsm.back()->keep_order = true;
      dp.smsm.back()->combined = f_combine;
      dp.smsm.back()->force_fix_wpw = f_fix_smsm;
      dp.smsm.back()->force_tbl_wpw = f_tbl_smsm;
    }
    build_plan(*dp.smsm.back(), prove_smsm_round(ni, Li, (int)j), scal);
  }
  if (lt.on) {
    const int m = lt.m, hm = m / 2;
    const size_t BM = B * (size_t)m, ent = late_tab_entries();
    lt.jac.ensure((size_t)LATE_FAMILIES * BM);
    lt.tab.ensure((size_t)LATE_FAMILIES * BM * ent);
    std::vector<uint32_t> gb(n);
    cc.same_msm_basis(gb.data());
    lt.gb_cols = idx_list(gb);
    lt.h_col = idx_list({(uint32_t)cc.H()});
    lt.part.ensure(6 * B * (size_t)opt_.late_slices);
    lt.extra.ensure(4 * B);
    CPX_HIP(hipMemsetAsync(lt.extra.p, 0, 4 * B * sizeof(TJac), stream_));   // all-zero = the identity: the outputs without a CRS term keep it (ordered before the prove's launches on this stream)
    lt.ipa.clear();
    lt.smsm.clear();
    lt.ipa_comp.clear();
    lt.smsm_comp.clear();
    std::vector<uint32_t> meta(2 * 6 * B);
    for (size_t g = 0; g < 6 * B; g++) {
      meta[g] = (uint32_t)g;      // request g = partial sum g
      meta[6 * B + g] = 1;
    }
    for (int r = 0; r < lt.nr; r++) {
      const int j = (int)lt.j0 + r;
      LateRound a{};
      a.m = m;
      a.half = m >> (r + 1);
      a.nproofs = (int)B;
      a.slices = (int)opt_.late_slices;
      a.tab = lt.tab.p;
      a.scal = d_rout_.p;
      // inner_product_argument.rs:150-163: L_C = <c_L, G_R> + beta <c_L, d_R> H, L_D = <d_R, G'_L>, R_C = <c_R, G_L> + beta <c_R, d_L> H,
      // R_D = <d_L, G'_R>; scalar rows as k_ipa_round_scalars lays them out for m active elements
      a.nout = 4;
      a.total = (int)(4 * B) * a.slices;
      a.scal_proof_stride = (uint32_t)(4 * hm + 2);
      a.o[0] = LateOut{LATE_F_G, 1, 0u};                          // (+ the H terms at scalar offsets hm and 3 hm + 1: exec_late_round)
      a.o[1] = LateOut{LATE_F_GP, 0, (uint32_t)(hm + 1)};
      a.o[2] = LateOut{LATE_F_G, 0, (uint32_t)(2 * hm + 1)};
      a.o[3] = LateOut{LATE_F_GP, 1, (uint32_t)(3 * hm + 2)};
      lt.ipa.push_back(a);
      lt.ipa_comp.push_back(meta.size());
      for (size_t p = 0; p < B; p++)
        for (int s : {sm.LC(j), sm.LD(j), sm.RC(j), sm.RD(j)}) meta.push_back(cidx(p, s));
      // same_multiscalar_argument.rs:104-112: L_A, L_T, L_U = <x_L, {G_b, T_b, U_b}_R>, R_* = <x_R, {..}_L>
      a.nout = 6;
      a.total = (int)(6 * B) * a.slices;
      a.scal_proof_stride = (uint32_t)(2 * hm);
      const int fam[3] = {LATE_F_GB, LATE_F_T, LATE_F_U};
      for (int q = 0; q < 3; q++) {
        a.o[q] = LateOut{fam[q], 1, 0u};
        a.o[3 + q] = LateOut{fam[q], 0, (uint32_t)hm};
      }
      lt.smsm.push_back(a);
      lt.smsm_comp.push_back(meta.size());
      for (size_t p = 0; p < B; p++)
        for (int s : {sm.LA(j), sm.LT(j), sm.LU(j), sm.RA(j), sm.RT(j), sm.RU(j)}) meta.push_back(cidx(p, s));
    }
    lt.meta.ensure(meta.size());
    CPX_HIP(hipMemcpy(lt.meta.p, meta.data(), meta.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  // -- side stream: R = a x vec_R, S = a x vec_S (curdleproofs.rs:112-113) and the four T_2 = s * {R, S} + r * H
  //    scalar multiplications (curdleproofs.rs:115-116, same_scalar_argument.rs:60-61)
  {
    std::vector<MsmTask> mt(2 * B);
    std::vector<uint32_t> md(2 * B);
    std::vector<SmulTask> st(4 * B);
    for (size_t p = 0; p < B; p++) {
      mt[2 * p] = MsmTask{pp(p), nullptr, d_veca_.p + p * ell, (uint32_t)ell, 0, (uint32_t)(2 * p * ell)};
      mt[2 * p + 1] = MsmTask{pp(p) + ell, nullptr, d_veca_.p + p * ell, (uint32_t)ell, 0, (uint32_t)((2 * p + 1) * ell)};
      md[2 * p] = slot_index(p, SL_R);
      md[2 * p + 1] = slot_index(p, SL_S);
      const Fr* kk = dp.k.p + p;
      const Fr* rk = rnd(p, ri.RK());
      st[4 * p + 0] = SmulTask{slot(p, sm.TMP(0)), slot(p, SL_R), slot(p, SL_CMT2), kk, 0, 0};
      st[4 * p + 1] = SmulTask{slot(p, sm.TMP(1)), slot(p, SL_S), slot(p, SL_CMU2), kk, 0, 0};
      st[4 * p + 2] = SmulTask{slot(p, sm.TMP(2)), slot(p, SL_R), slot(p, sm.CMA2()), rk, 0, 0};
      st[4 * p + 3] = SmulTask{slot(p, sm.TMP(3)), slot(p, SL_S), slot(p, sm.CMB2()), rk, 0, 0};
    }
    CPX_HIP(hipMemcpy(side_.tasks.p, mt.data(), mt.size() * sizeof(MsmTask), hipMemcpyHostToDevice));
    CPX_HIP(hipMemcpy(side_.dst.p, md.data(), md.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    CPX_HIP(hipMemcpy(side_.stasks.p, st.data(), st.size() * sizeof(SmulTask), hipMemcpyHostToDevice));
    int side[6];
    side_stream_slots(Li, side);
    dp.side_cols = idx_list(std::vector<uint32_t>(side, side + 6));
    // ... and with R and S from the tables (prove_reqs.hpp): R = k^-1 Rk, S = k^-1 Sk, cm_A.T_2 = (r_k k^-1) Rk + r_a H, cm_B.T_2 likewise;
    // the scalars are k_ps_aperm's (cm_T.T_2 and cm_U.T_2 are the sums of dp.prs_sum, which compresses them as well)
    std::vector<SmulTask> sv(4 * B);
    for (size_t p = 0; p < B; p++) {
      const Fr* k_inv = dp.sc.p + p * SC_COUNT + SC_K_INV;
      const Fr* rk_k_inv = dp.sc.p + p * SC_COUNT + SC_RK_K_INV;
      Aff* const rk = slot(p, rs_tables_slot(Li, 0));
      Aff* const sk = slot(p, rs_tables_slot(Li, 1));
      sv[4 * p + 0] = SmulTask{nullptr, rk, slot(p, SL_R), k_inv, 0, 0};
      sv[4 * p + 1] = SmulTask{nullptr, sk, slot(p, SL_S), k_inv, 0, 0};
      sv[4 * p + 2] = SmulTask{slot(p, sm.TMP(2)), rk, slot(p, sm.CMA2()), rk_k_inv, 0, 0};
      sv[4 * p + 3] = SmulTask{slot(p, sm.TMP(3)), sk, slot(p, sm.CMB2()), rk_k_inv, 0, 0};
    }
    CPX_HIP(hipMemcpy(dp.stasks_tbl.p, sv.data(), sv.size() * sizeof(SmulTask), hipMemcpyHostToDevice));
    dp.side_cols_tbl = idx_list({(uint32_t)SL_R, (uint32_t)SL_S, (uint32_t)sm.CMA2(), (uint32_t)sm.CMB2()});
  }
  if (!tab_.dstream) CPX_HIP(hipStreamCreateWithFlags(&tab_.dstream, hipStreamNonBlocking));
  if (!dp.ev_t1) {
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_t1, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_t2, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_a2, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_ap, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_rs, hipEventDisableTiming));
  }
  if (!dp.ev_a) {
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_a, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_b, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_c, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dp.ev_d, hipEventDisableTiming));
  }
  // the shared scratch of exec_plan sized for the largest phase now: nothing is allocated (no implicit device synchronisation)
  // between the first and the last launch of a prove
  {
    size_t max_parts = 1, max_sets = 1;
    auto upd = [&](const TblPlan& pl) {
      max_parts = std::max(max_parts, pl.nparts);
      max_sets = std::max(max_sets, pl.fix_sets + pl.tbl_sets);
    };
    upd(dp.p1);
    upd(dp.p1b);
    upd(dp.p1t);   // (in line on the main stream when the table stream is off: large batches, serial_streams)
    upd(dp.prs);   // (likewise)
    upd(dp.p2);
    upd(dp.p3);
    for (auto& pl : dp.ipa)
      if (pl) upd(*pl);
    for (auto& pl : dp.smsm)
      if (pl) upd(*pl);
    if (lt.on) max_parts = std::max(max_parts, 6 * B);
    if (dp.fused || dp.fused_smsm) {
      dp.rpart.ensure(max_parts);
      dp.rcount.ensure(B);
    }
    main_.ensure(max_sets, max_parts);
    d_tbltmp_.ensure(std::max(table_chunk_rows(B) * NP * (size_t)(pcopies_ / 2 - 1),   // one chunk of the table build ...
                              (3 * B * (size_t)lt.m + 63) / 64 * 64 * late_tmp_per_lane()));               // ... or the multiples of the late rounds' materialised points
  }
  dp.signature = sig;
}

// The side scratch of the one-off bucket MSMs R = msm(vec_R, a), S = msm(vec_S, a) (launch_rs) for the loaded batch: with R and S from the
// tables only the batches that fall back need it
void Engine::ensure_rs_scratch() {
  side_.conv.ensure(4 * B_ * ell_);
  side_.digits.ensure(9 * 2 * B_ * ell_);
  side_.scr.ensure(2 * B_ * 32, 2 * B_ * 32);
}

// Whether the loaded batch runs its table build and phase 1t on the table stream (option table_stream_max, stated for n <= 256)
bool Engine::table_stream_on() const { return !opt_.serial_streams && (long)(B_ * std::max<size_t>(n_, 256)) <= opt_.table_stream_max * 256L; }

// The high-priority stream of a small batch's transcript prefix (created on first use; a plain stream where priorities are not offered)
hipStream_t Engine::prefix_stream() {
  if (!side_.hi_stream) {
    int lo = 0, hi = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) {
      (void)hipGetLastError();
      lo = hi = 0;
    }
    if (hipStreamCreateWithPriority(&side_.hi_stream, hipStreamNonBlocking, hi) != hipSuccess) {
      (void)hipGetLastError();
      CPX_HIP(hipStreamCreateWithFlags(&side_.hi_stream, hipStreamNonBlocking));
    }
  }
  return side_.hi_stream;
}

// The kernel launches of one device-resident prove (everything between the upload of the witnesses and the download of the proofs),
// on the main stream and — forked and joined through events — the side stream.  No host synchronisation, no allocation.
void Engine::enqueue_prove_device() {
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  const SlotMap sm(L);
  const size_t NP = np(), NS = sm.count();
  DevProver& dp = dprove_;
  const ProveDev& d = dp.dev;
  const int Bi = (int)B;
  // (measurement aid, option serial_streams: the side stream's work in line on the main stream, so that every kernel's duration is its
  // own and a pass is the plain sum of its kernels)
  hipStream_t const side = opt_.serial_streams ? stream_ : side_.stream;
  // -- P0: compressed instance vectors, M -> affine (table source slot 0); side stream: transcript prefix (instance + M
  //    absorbed, vec_a drawn), then R and S; main stream: the per-proof tables
  tick("k_compress", 0, (double)(4 * ell * B));
  launch_compress(d_pp_.p, (int)(4 * ell), (int)pp_stride_, Bi, d_bytes_.p, stream_);
  tock();
  launch_finalize(d_Mjac_.p, Bi, d_psrc_.p, dp.mdst.p, d_mcomp_.p, stream_);
  CPX_HIP(hipEventRecord(dp.ev_a, stream_));
  CPX_HIP(hipStreamWaitEvent(side, dp.ev_a, 0));
  // (a small batch: the prefix's waves claim whole SIMDs and go through a high-priority queue, so that they are placed before the
  // waves of the table build that becomes ready at the same moment — otherwise they wait for SIMDs to drain)
  const bool excl = (long)B <= opt_.transcript_excl_max && !opt_.serial_streams;
  hipStream_t const pre = excl ? prefix_stream() : side;
  if (pre != side) {
    // head start: the main and the table stream continue behind an event the prefix stream records just before it launches — one
    // more hop between queues (~80 us) than the prefix kernel needs to place its waves on empty SIMDs
    CPX_HIP(hipStreamWaitEvent(pre, dp.ev_a, 0));
    CPX_HIP(hipEventRecord(dp.ev_a2, pre));
  }
  tick("k_transcript_step1", 0, (double)B);
  launch_transcript_step1(d_bytes_.p, d_mcomp_.p, Bi, (int)ell, d_tstate_.p, d_veca_.p, pre, (long)B * 256 >= opt_.transcript_lane_min_batch * (long)std::max<size_t>(n, 256), excl);
  tock();
  CPX_HIP(hipEventRecord(dp.ev_b, pre));
  if (pre != side) CPX_HIP(hipStreamWaitEvent(side, dp.ev_b, 0));
  // R and S: from the per-proof tables further down (dp.rs_tables), or here as one-off bucket MSMs over vec_R and vec_S
  const bool rs_tbl = dp.rs_tables;
  if (!rs_tbl) launch_rs(2 * B, 2 * B, 1, opt_.rs_pairs != 0, side, true);
  ProveDev d_aperm = d;
  d_aperm.rs_tables = rs_tbl ? 1 : 0;
  // table stream: the per-proof tables, then B_t and B_u (phase 1t) — nothing on the main stream needs a table before phase 2 (M's row)
  // nor B_t, B_u before the SameMSM transcript step
  hipStream_t const tabs = table_stream_on() ? tab_.dstream : stream_;
  if (tabs != stream_) CPX_HIP(hipStreamWaitEvent(tabs, pre != side ? dp.ev_a2 : dp.ev_a, 0));
  if (pre != side) CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_a2, 0));
  // (in equal chunks of table_chunk_rows(B) proofs, one after the other on this stream, through ONE chunk's worth of scratch: 6.7 instead of
  // 13.5 GB per context at 8192 proofs of ell = 252; a chunk of 4096 proofs is 2 M threads — the GPU is as full as with all rows at once)
  for (size_t r0 = 0, ch = table_chunk_rows(B); r0 < B; r0 += ch) {
    const size_t rows = std::min(ch, B - r0);
    tick("k_table_build", 0, (double)(rows * NP));
    launch_table_build(opt_, d_psrc_.p + r0 * NP, NP, d_ptab_.p + r0 * (size_t)pcopies_ * NP, (int)rows, (size_t)pcopies_ * NP, (int)NP, (int)NP, pcopies_, true, d_tbltmp_.p, tabs,
                       8);   // copy c = 2^(8c) P whatever the copy count
    tock();
  }
  CPX_HIP(hipEventRecord(dp.ev_t1, tabs));
  exec_plan(dp.p1t, dp.slotcomp.p, true);
  CPX_HIP(hipEventRecord(dp.ev_t2, tabs));
  if (opt_.p1_split) {   // the randomness-only commitments beside the prefix, A behind it
    exec_plan(dp.p1, dp.slotcomp.p);
    CPX_HIP(hipEventRecord(dp.ev_c, stream_));
    CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_b, 0));
    launch_ps_aperm(d_aperm, Bi, stream_);
    if (rs_tbl && tabs != stream_) CPX_HIP(hipEventRecord(dp.ev_ap, stream_));
    exec_plan(dp.p1b, dp.slotcomp.p);
  } else {
    CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_b, 0));   // vec_a and the transcript states
    // -- P1
    launch_ps_aperm(d_aperm, Bi, stream_);
    if (rs_tbl && tabs != stream_) CPX_HIP(hipEventRecord(dp.ev_ap, stream_));
    exec_plan(dp.p1, dp.slotcomp.p);
    CPX_HIP(hipEventRecord(dp.ev_c, stream_));           // the r * H points of the T_2 commitments are in TMP0..3
  }
  if (rs_tbl) {   // k R = msm(T, a_sigma), k S = msm(U, a_sigma): behind the tables, B_t, B_u (same stream) and V_APERM
    if (tabs != stream_) CPX_HIP(hipStreamWaitEvent(tabs, dp.ev_ap, 0));
    exec_plan(dp.prs, dp.slotcomp.p, true);
    CPX_HIP(hipEventRecord(dp.ev_rs, tabs));
    CPX_HIP(hipStreamWaitEvent(side, dp.ev_rs, 0));
  }
  CPX_HIP(hipStreamWaitEvent(side, dp.ev_c, 0));
  tick("k_smul", 0, (double)(4 * B));
  count_smul_quad(launch_smul(rs_tbl ? dp.stasks_tbl.p : side_.stasks.p, 4 * Bi, 1, side, /*exclusive_simd=*/side != stream_, opt_.serial_streams ? 0 : opt_.smul_quad_max));   // (a small batch: at most 16 waves, each on a SIMD of its own)
  tock();
  if (rs_tbl) {   // cm_T.T_2 = k R + r_t H, cm_U.T_2 = k S + r_u H: sums, compressed into their slots (no MSM task: the scratch is not touched)
    launch_tbl_phase(dp.prs_sum, dp.prs_sum.ttasks.p, dp.prs_sum.ftasks.p, dp.prs_sum.meta.p, dp.slotcomp.p, side, main_);
    launch_compress_cols(d_pp_.p + 4 * ell, dp.side_cols_tbl, 4, (int)pp_stride_, Bi, dp.slotcomp.p, (int)NS, side);
  } else {
    launch_compress_cols(d_pp_.p + 4 * ell, dp.side_cols, 6, (int)pp_stride_, Bi, dp.slotcomp.p, (int)NS, side);
  }
  CPX_HIP(hipEventRecord(dp.ev_d, side));
  launch_ps_sameperm(d, Bi, stream_);
  // -- P2, P3
  if (tabs != stream_) CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_t1, 0));   // M's table row
  exec_plan(dp.p2, dp.slotcomp.p);
  launch_ps_gprod(d, Bi, stream_);
  exec_plan(dp.p3, dp.slotcomp.p);
  launch_ps_ipa_setup(d, Bi, stream_);
  // -- IPA rounds (inner_product_argument.rs:150-186 in all-MSM form; the last log2(m) of a large batch on materialised folded
  //    bases: late.hip)
  const DevProver::Late& lt = dp.late;
  const size_t BM = B * (size_t)lt.m;
  // fused rounds (round.hip): the descriptor of a round's launch from its plan (the scratch pointers are read at enqueue time: a later
  // batch of another shape may have regrown them)
  if (dp.fused || dp.fused_smsm) CPX_HIP(hipMemsetAsync(dp.rcount.p, 0, B * sizeof(uint32_t), stream_));
  auto round_dev = [&](const TblPlan& pl, int nreq, bool last) {
    RoundDev rd{};
    rd.ftasks = pl.ftasks.p;
    rd.ttasks = pl.ttasks.p;
    rd.nf = (int)(pl.nft / B);
    rd.nt = (int)(pl.ntt / B);
    rd.fix_wpw = pl.fix_wpw;
    rd.tbl_wpw = rd.nt ? pl.tbl_wpw : 0;
    rd.combine = (rd.nt && pl.combined && rd.nf * (16 / pl.fix_wpw) == rd.nt * (32 / pl.tbl_wpw)) ? 1 : 0;
    rd.wpp = rd.combine ? (uint32_t)(rd.nt * (32 / pl.tbl_wpw)) : (uint32_t)(rd.nf * (16 / pl.fix_wpw) + (rd.nt ? rd.nt * (32 / pl.tbl_wpw) : 0));
    rd.nreq = nreq;
    rd.nproofs = Bi;
    rd.max_count = (uint32_t)std::max(16 / pl.fix_wpw, rd.nt ? 64 / pl.tbl_wpw : 0);
    rd.next_scalars = last ? 0 : 1;
    rd.fixtab = fixtab();
    rd.nc = (int)nc();
    rd.fraw = main_.raw.p;
    rd.fraw_slot = main_.rawslot.p;
    rd.traw = main_.raw.p + pl.fix_sets * raw_set_words();
    rd.traw_slot = main_.rawslot.p + pl.fix_sets;
    rd.part = dp.rpart.p;
    rd.meta = pl.meta.p;
    rd.comp_index = pl.meta.p + 3 * pl.nt;
    rd.counter = dp.rcount.p;
    rd.scal_out = d_rout_.p;
    return rd;
  };
  if (dp.fused) {
    launch_ipa_round_scalars(d_rvec_.p, Bi, (int)n, (int)(n >> 1), d_rbeta_.p, d_rout_.p, stream_);   // round 0's scalars; every later round's come from the tail before it
    for (size_t j = 0; j < L; j++) {
      const TblPlan& pl = *dp.ipa[j];
      tick("k_round_fused<ipa>", 128.0 * pl.pts_fix, pl.pts_fix);
      launch_round_fused(round_dev(pl, 4, j + 1 == L), d, (int)j, true, stream_);
      tock();
    }
  }
  for (size_t j = 0; j < L && !dp.fused; j++) {
    const int half = (int)(n >> (j + 1));
    if (lt.on && j == lt.j0) {   // G^(j0) and G'^(j0) from the table of multiples (fold coefficients S_G, S_G' = u o S^-1), their small multiples
      tick("k_late_fix", 128.0 * 2 * n * B, (double)(2 * n * B));
      launch_late_fix(d_rvec_.p + 2 * n, 4 * n, nullptr, (int)n, lt.m, fixtab(), fix_bits_, (int)nc(), lt.jac.p + LATE_F_G * BM, (size_t)lt.m, Bi, stream_);
      tock();
      launch_late_fix(d_rvec_.p + 3 * n, 4 * n, nullptr, (int)n, lt.m, fixtab(), fix_bits_, (int)nc(), lt.jac.p + LATE_F_GP * BM, (size_t)lt.m, Bi, stream_);
      tick("k_late_tables", 0, (double)(2 * BM));
      launch_late_tables(lt.jac.p + LATE_F_G * BM, lt.tab.p + LATE_F_G * BM * late_tab_entries(), d_tbltmp_.p, (int)(2 * BM), stream_);
      tock();
      launch_late_restart(d_rvec_.p, (int)n, lt.m, Bi, stream_);
    }
    if (lt.on && j >= lt.j0) {
      launch_ipa_round_scalars(d_rvec_.p, Bi, (int)n, half, d_rbeta_.p, d_rout_.p, stream_, lt.m);
      exec_late_round(lt.ipa[j - lt.j0], lt.ipa_comp[j - lt.j0], "k_late_msm");
      launch_ps_ipa_round(d, Bi, (int)j, stream_);
      launch_ipa_round_fold(d_rvec_.p, Bi, (int)n, half, d_rgam_.p, stream_, lt.m);
      continue;
    }
    launch_ipa_round_scalars(d_rvec_.p, Bi, (int)n, half, d_rbeta_.p, d_rout_.p, stream_);
    exec_plan(*dp.ipa[j], dp.slotcomp.p);
    launch_ps_ipa_round(d, Bi, (int)j, stream_);
    launch_ipa_round_fold(d_rvec_.p, Bi, (int)n, half, d_rgam_.p, stream_);
  }
  // -- SameScalar, SameMSM step 1 (needs R, S and the T_2 commitments of the side stream)
  CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_d, 0));
  if (tabs != stream_) CPX_HIP(hipStreamWaitEvent(stream_, dp.ev_t2, 0));   // B_t, B_u in the slot registry
  launch_ps_smsm_setup(d, Bi, stream_);
  if (dp.fused_smsm) {
    launch_smsm_round_scalars(dp.rvec2.p, Bi, (int)n, (int)(n >> 1), d_rout_.p, stream_);
    for (size_t j = 0; j < L; j++) {
      const TblPlan& pl = *dp.smsm[j];
      tick("k_round_fused<smsm>", 128.0 * (pl.pts_fix + pl.pts_tbl), pl.pts_fix + pl.pts_tbl);
      launch_round_fused(round_dev(pl, 6, j + 1 == L), d, (int)j, false, stream_);
      tock();
    }
  }
  for (size_t j = 0; j < L && !dp.fused_smsm; j++) {
    const int half = (int)(n >> (j + 1));
    if (lt.on && j == lt.j0) {   // T_b^(j0), U_b^(j0), G_b^(j0): one shared digit sequence per proof (fold coefficients S_M)
      // (T_b, U_b with two lanes per output fill a wave at m = 16, with one lane per output at m = 32; m = 64: two waves per proof; G_b comes
      // from the table of multiples like G and G')
      tick("k_late_uniform", 128.0 * 2 * n * B, (double)(2 * n * B));
      launch_late_uniform(dp.rvec2.p + n, 2 * n, d_ptab_.p, (size_t)pcopies_ * NP, (int)NP, ctab(), (int)nc(), lt.gb_cols, (int)n, lt.m, 2, 4 * lt.m <= 64 ? 2 : 1,
                          lt.jac.p + LATE_F_T * BM, BM, Bi, stream_, copies_ / pcopies_);
      tock();
      launch_late_fix(dp.rvec2.p + n, 2 * n, lt.gb_cols, (int)n, lt.m, fixtab(), fix_bits_, (int)nc(), lt.jac.p + LATE_F_GB * BM, (size_t)lt.m, Bi, stream_);
      tick("k_late_tables", 0, (double)(3 * BM));
      launch_late_tables(lt.jac.p + LATE_F_T * BM, lt.tab.p + LATE_F_T * BM * late_tab_entries(), d_tbltmp_.p, (int)(3 * BM), stream_);
      tock();
    }
    if (lt.on && j >= lt.j0) {
      launch_smsm_round_scalars(dp.rvec2.p, Bi, (int)n, half, d_rout_.p, stream_, lt.m);
      exec_late_round(lt.smsm[j - lt.j0], lt.smsm_comp[j - lt.j0], "k_late_msm");
      launch_ps_smsm_round(d, Bi, (int)j, stream_);
      launch_smsm_round_fold(dp.rvec2.p, Bi, (int)n, half, d_rgam_.p, stream_, lt.m);
      continue;
    }
    launch_smsm_round_scalars(dp.rvec2.p, Bi, (int)n, half, d_rout_.p, stream_);
    exec_plan(*dp.smsm[j], dp.slotcomp.p);
    launch_ps_smsm_round(d, Bi, (int)j, stream_);
    launch_smsm_round_fold(dp.rvec2.p, Bi, (int)n, half, d_rgam_.p, stream_);
  }
  launch_ps_serialize(d, Bi, stream_);
}

void Engine::batch_prove_device(const ProveDraws& dr, uint8_t* proofs_out) {
  HostSpan wall(this, "host_prove_wall");
  CPX_HIP(hipSetDevice(device_));
  const size_t B = B_, ell = ell_, n = n_, nrand = 3 * n + 9;
  prepare_device_prover();
  DevProver& dp = dprove_;
  // R and S from the per-proof tables (option rs_from_tables) need k^-1: a batch in which some k is zero — the reference proves such a
  // witness, T and U all identity — takes the one-off bucket MSMs as a whole, and so does one whose k is already on the device (no look
  // without a synchronisation).  (Fr::zero() is all-zero bytes in Montgomery form, too.)
  dp.rs_tables = opt_.rs_from_tables != 0 && dr.kind == hipMemcpyHostToDevice;
  for (size_t p = 0; p < B && dp.rs_tables; p++) {
    static const uint8_t zero[sizeof(Fr)] = {};
    if (!memcmp(dr.k + p * sizeof(Fr), zero, sizeof(Fr))) dp.rs_tables = false;
  }
  if (!dp.rs_tables) ensure_rs_scratch();   // (allocates on the first such batch only)

  // witnesses and the prover's random draws: the only host -> device traffic of a prove (with states: 40 bytes of randomness per proof)
  CPX_HIP(hipMemcpyAsync(dp.perm.p, dr.perm, B * ell * sizeof(uint32_t), dr.kind, stream_));
  CPX_HIP(hipMemcpyAsync(dp.k.p, dr.k, B * sizeof(Fr), dr.kind, stream_));
  CPX_HIP(hipMemcpyAsync(dp.mbl.p, dr.mbl, B * 4 * sizeof(Fr), dr.kind, stream_));
  if (dr.rand) {
    CPX_HIP(hipMemcpyAsync(dp.rnd.p, dr.rand, B * nrand * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  } else {
    if (dr.states_in) {
      rng_.states.ensure(B * RNG_STATE_BYTES);
      CPX_HIP(hipMemcpyAsync(rng_.states.p, dr.states_in, B * RNG_STATE_BYTES, hipMemcpyHostToDevice, stream_));
    }
    tick("k_rng_draw", (double)(B * nrand * sizeof(Fr)), (double)(B * nrand));
    launch_rng_draw(rng_draw_args(rng_.states.p, nullptr, B, 0, nullptr, {{nrand, dp.rnd.p}}), stream_);
    tock();
  }

  enqueue_prove_device();
  CPX_HIP(hipMemcpyAsync(proofs_out, dp.proofs.p, B * proof_size(), hipMemcpyDeviceToHost, stream_));
  wait_stream_blocking();
  flush_timers();
  // the advanced states: read once the prove has ended, so that a prove that throws leaves the caller's states alone
  if (!dr.rand && dr.states_out) CPX_HIP(hipMemcpy(dr.states_out, rng_.states.p, B * RNG_STATE_BYTES, hipMemcpyDeviceToHost));
  if (opt_.trace) {   // debugging aid: the challenges and responses of proof 0, same format as the host-driven prover prints
    std::vector<Fr> sc(SC_COUNT);
    CPX_HIP(hipMemcpy(sc.data(), dp.sc.p, SC_COUNT * sizeof(Fr), hipMemcpyDeviceToHost));
    for (int i = 0; i < SC_COUNT; i++)
      if (kScNames[i]) trace_scalar(kScNames[i], sc[i]);
  }
}

// ---------------------------------------------------------------- verifier
void Engine::prepare_device_verifier(size_t rand_stride) {
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  const SlotMap sm(L);
  const ProofLayout pl(L);
  CheckPlan cp(B, ell, L, n);
  const size_t NS = sm.count(), NPP = pl.n_points(), NM = cp.NM, NPT = cp.NPT, psz = pl.size();
  DevVerifier& dv = dverify_;
  d_bytes_.ensure(B * 4 * ell * 48);
  d_mcomp_.ensure(B * 48);
  d_tstate_.ensure(B * 27);
  d_veca_.ensure(B * ell);
  dv.proofs.ensure(B * psz);
  dv.rnd.ensure(B * VF_FUSED_COUNT);
  dv.vsc.ensure(B * (size_t)VSC_COUNT);
  dv.slotcomp.ensure(B * NS * 48);
  dv.status.ensure(B * NPP);
  dv.scal.ensure(B * NPT + n);   // + the summed CRS scalars of a fused batch
  dv.scal_crs.ensure(B * n);
  dv.flags.ensure(B);
  dv.src_off.ensure(B * NPP);
  dv.dst.ensure(B * NPP);
  dv.mdst.ensure(B);
  dv.mtasks.ensure(B);
  dv.ftasks.ensure(B + 1);
  dv.gidx.ensure(B * NPT);
  d_conv_.ensure(2 * B * NPT);
  d_digits_.ensure(9 * B * NPT);
  d_ttasks_.ensure(B);
  d_part_.ensure(B * 32);
  d_res_.ensure(B);
  d_comp_.ensure(B * 48);
  // grouped verifier: the plan for option locate_groups_max and the buffers its task lists point into
  const LocatePlan lp = locate_plan(B, opt_.locate_groups_max);
  dv.lsum.ensure(lp.s1_crs_scalars(n));
  dv.ltasks.ensure(lp.NT);
  dv.lftasks.ensure(lp.NT);
  dv.l2tasks.ensure(B);
  dv.l2ftasks.ensure(B);
  const std::vector<const void*> sig = {d_pp_.p,       d_bytes_.p,  d_mcomp_.p,     d_tstate_.p, d_veca_.p,  dv.proofs.p, dv.rnd.p,    dv.vsc.p, dv.slotcomp.p,
                                        dv.status.p,   dv.scal.p,   dv.scal_crs.p,  dv.flags.p,  dv.mtasks.p, dv.ftasks.p, dv.gidx.p,  ctab(),   fixtab(),
                                        (const void*)(uintptr_t)B, (const void*)(uintptr_t)ell, (const void*)(uintptr_t)fix_bits_,
                                        dv.lsum.p,     dv.ltasks.p, dv.lftasks.p,   (const void*)(uintptr_t)lp.G, (const void*)(uintptr_t)lp.NT};
  dv.dev.rand_stride = (int)rand_stride;
  if (sig == dv.signature) return;
  dv.signature.clear();
  VerifyDev& d = dv.dev;
  d.ell = (int)ell;
  d.n = (int)n;
  d.L = (int)L;
  d.NS = (int)NS;
  d.NM = (int)NM;
  d.psz = psz;
  d.proofs = dv.proofs.p;
  d.rnd = dv.rnd.p;
  d.tstate = d_tstate_.p;
  d.veca = d_veca_.p;
  d.vsc = dv.vsc.p;
  d.slotcomp = dv.slotcomp.p;
  d.inst_comp = d_bytes_.p;
  d.mcomp = d_mcomp_.p;
  d.status = dv.status.p;
  d.scal = dv.scal.p;
  d.scal_crs = dv.scal_crs.p;
  d.flags = dv.flags.p;
  memcpy(d.crs_h_comp, crs_H_comp_, 48);

  std::vector<uint32_t> so(B * NPP), ds(B * NPP), md(B);
  for (size_t p = 0; p < B; p++) {
    for (size_t q = 0; q < NPP; q++) {
      so[p * NPP + q] = (uint32_t)(p * psz + pl.point_offset((int)q));   // where the proof points sit inside the serialized proofs
      ds[p * NPP + q] = slot_index(p, SL_A + (int)q);
    }
    md[p] = slot_index(p, SL_M);
  }
  CPX_HIP(hipMemcpy(dv.src_off.p, so.data(), so.size() * 4, hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.dst.p, ds.data(), ds.size() * 4, hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.mdst.p, md.data(), md.size() * 4, hipMemcpyHostToDevice));
  // D = B - beta^-1 sum(G) + alpha sum(H) (grand_product_argument.rs:223) and A' = A + cm_T.T_1 + cm_U.T_1 (curdleproofs.rs:258)
  // are hashed into the transcript, so they are needed as bytes
  build_plan(dv.pd, verify_requests((int)n, (int)L), [&](size_t p, const ReqScal& sc) { return ScalAddr{nullptr, dv.vsc.p + p * VSC_COUNT + sc.at}; });
  // the accumulated check: per proof one fixed-base task over G | Hvec and one bucket MSM over R | S | T | U and the misc slots
  //   (check_plan.hpp: k_vs_scalars fills scal | scal_crs, k_vs_crs_sum_groups the summed rows)
  std::vector<uint32_t> all_idx(NPT);   // row-relative gather list: misc index j == slot j (SL_H .. SL_M, then the proof points)
  for (size_t i = 0; i < NPT; i++) all_idx[i] = (uint32_t)i;
  cp.place(d_pp_.p, pp_stride_, idx_list(all_idx), dv.gidx.p, dv.scal.p, dv.scal_crs.p, dv.lsum.p);
  dv.cplan = cp;
  dv.fix_wpw = msm_fix_windows_per_wave(opt_, (int)B, fix_bits_);
  dv.fix_parts = msm_fix_parts(fix_bits_, dv.fix_wpw);
  dv.fix_wpw1 = msm_fix_windows_per_wave(opt_, 1, fix_bits_);
  dv.fix_parts1 = msm_fix_parts(fix_bits_, dv.fix_wpw1);
  std::vector<MsmTask> mt(B);
  std::vector<FixTask> ft(B + 1);
  std::vector<uint32_t> gi(cp.n_points());
  cp.proof_tasks((size_t)dv.fix_parts, mt.data(), ft.data());
  cp.gather(gi.data());
  // fused batch: the proofs in up to 256 groups, every group one task of the endomorphism bucket-list kernel; the CRS scalars summed
  // over the proofs sit behind the point scalars
  dv.fplan = CheckPlan::fused_plan(B);
  dv.gtasks.ensure(dv.fplan.NT);
  std::vector<MsmTask> gt(dv.fplan.NT);
  CheckPlan fcp = cp;
  fcp.at.sums = dv.scal.p + cp.n_points();
  fcp.fused_tasks(gt.data(), &ft[B]);
  // grouped verifier, stage 1: the same layout for ITS group size, and per group a fixed-base task over the group's summed CRS scalars
  dv.lplan = lp;
  dv.lfix_wpw = msm_fix_windows_per_wave(opt_, (int)lp.NT, fix_bits_);
  dv.lfix_parts = msm_fix_parts(fix_bits_, dv.lfix_wpw);
  std::vector<MsmTask> lt(lp.NT);
  std::vector<FixTask> lf(lp.NT);
  cp.group_tasks(lp, (size_t)dv.lfix_parts, lt.data(), lf.data());
  CPX_HIP(hipMemcpy(dv.mtasks.p, mt.data(), B * sizeof(MsmTask), hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.ftasks.p, ft.data(), (B + 1) * sizeof(FixTask), hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.gidx.p, gi.data(), gi.size() * 4, hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.gtasks.p, gt.data(), gt.size() * sizeof(MsmTask), hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.ltasks.p, lt.data(), lp.NT * sizeof(MsmTask), hipMemcpyHostToDevice));
  CPX_HIP(hipMemcpy(dv.lftasks.p, lf.data(), lp.NT * sizeof(FixTask), hipMemcpyHostToDevice));
  if (!dv.ev_a) {
    CPX_HIP(hipEventCreateWithFlags(&dv.ev_a, hipEventDisableTiming));
    CPX_HIP(hipEventCreateWithFlags(&dv.ev_b, hipEventDisableTiming));
  }
  dv.signature = sig;
}

// curdleproofs.rs:197 for every loaded instance (verdict != nullptr) or BASELINE config 5 (fused_partial != nullptr), all on the
// device: the host uploads proofs and random factors, enqueues, and reads back 48 bytes + a flag word per proof (or one point).
void Engine::verify_core_device(const uint8_t* proofs, const uint8_t* rand, size_t rand_stride, int* verdict, uint8_t* fused_partial, int* fused_invalid,
                                size_t* grouped) {
  CPX_HIP(hipSetDevice(device_));
  const size_t B = B_, ell = ell_, n = n_, L = L_;
  const ProofLayout pl(L);
  const size_t NPP = pl.n_points(), psz = pl.size();
  prepare_device_verifier(rand_stride);
  DevVerifier& dv = dverify_;
  const VerifyDev& d = dv.dev;
  const size_t NPT = dv.cplan.NPT;
  const int Bi = (int)B;
  CPX_HIP(hipMemcpyAsync(dv.proofs.p, proofs, B * psz, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dv.rnd.p, rand, B * rand_stride * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  // -- V0: compressed instance vectors, M -> affine; side stream: transcript prefix; main: proof points -> slots
  tick("k_compress", 0, (double)(4 * ell * B));
  launch_compress(d_pp_.p, (int)(4 * ell), (int)pp_stride_, Bi, d_bytes_.p, stream_);
  tock();
  launch_finalize(d_Mjac_.p, Bi, d_pp_.p, dv.mdst.p, d_mcomp_.p, stream_);
  CPX_HIP(hipEventRecord(dv.ev_a, stream_));
  hipStream_t const side = opt_.serial_streams ? stream_ : side_.stream;
  CPX_HIP(hipStreamWaitEvent(side, dv.ev_a, 0));
  tick("k_transcript_step1", 0, (double)B);
  launch_transcript_step1(d_bytes_.p, d_mcomp_.p, Bi, (int)ell, d_tstate_.p, d_veca_.p, side, (long)B * 256 >= opt_.transcript_lane_min_batch * (long)std::max<size_t>(n, 256), (long)B <= opt_.transcript_excl_max && !opt_.serial_streams);
  tock();
  CPX_HIP(hipEventRecord(dv.ev_b, side));
  tick("k_decompress", 0, (double)(B * NPP));
  launch_decompress(opt_, dv.proofs.p, (int)(B * NPP), d_pp_.p, dv.dst.p, dv.status.p, 1, stream_, dv.src_off.p);
  tock();
  CPX_HIP(hipStreamWaitEvent(stream_, dv.ev_b, 0));
  // -- V1: transcript up to the grand-product beta; D and A' as bytes; the rest of the transcript and the scalars
  launch_vs_prefix(d, Bi, stream_);
  exec_plan(dv.pd, dv.slotcomp.p);
  launch_vs_scalars(d, Bi, stream_);
  // -- V2: the accumulated check(s)
  //    (check_plan.hpp); the flag words arrive behind the same wait as the first sums — copied behind the check's launches where the mode
  //    allows it (a copy between the kernels of a pass cost the four-context fused bench 1 - 2 %)
  h_u32_.ensure(B);
  const uint32_t* flags = h_u32_.p;
  auto fetch_flags = [&] { CPX_HIP(hipMemcpyAsync(h_u32_.p, dv.flags.p, B * 4, hipMemcpyDeviceToHost, stream_)); };
  if (fused_partial) {   // the CRS scalars summed over all proofs: one group of B
    launch_vs_crs_sum_groups(dv.scal_crs.p, Bi, (int)n, Bi, 1, dv.scal.p + B * NPT, stream_);
    launch_check_fused(dv.gtasks.p, dv.ftasks.p + B, dv.fplan.NT, dv.fplan.G, NPT, B * NPT, dv.fix_wpw1, dv.fix_parts1);
    fetch_flags();
    wait_stream_blocking();
    memcpy(fused_partial, h_comp_.p, sizeof(Jac));
    int invalid = 0;
    for (size_t p = 0; p < B; p++) invalid += flags[p] ? 1 : 0;
    if (fused_invalid) *fused_invalid = invalid;
  } else if (grouped) {   // the grouped check (locate_plan.hpp): every group's CRS scalars added up in Fr, then the two stages
    const LocatePlan& lp = dv.lplan;
    tick("k_vs_crs_sum_groups", 32.0 * B * n, (double)(B * n));
    launch_vs_crs_sum_groups(dv.scal_crs.p, Bi, (int)n, (int)lp.G, (int)lp.NT, dv.lsum.p, stream_);
    tock();
    fetch_flags();   // (located_check reads them behind stage 1's wait)
    *grouped = located_check(dv.cplan, lp, LocateTasks{dv.ltasks.p, dv.lftasks.p, dv.lfix_wpw, dv.lfix_parts, dv.l2tasks.p, dv.l2ftasks.p}, flags, true, verdict);
  } else {
    launch_check(dv.mtasks.p, dv.ftasks.p, B, NPT, dv.fix_wpw, dv.fix_parts, 1);
    fetch_flags();
    wait_stream_blocking();
    for (size_t p = 0; p < B; p++) verdict[p] = check_verdict(flags[p], check_passed(p));
  }
  flush_timers();
}

void trace_scalar(const char* name, const Fr& x) {
  fprintf(stderr, "[cpx trace] %-12s ", name);
  for (int i = 7; i >= 0; i--) fprintf(stderr, "%08x", x.v[i]);
  fprintf(stderr, "\n");
}

}  // namespace cpx
