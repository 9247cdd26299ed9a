// The sub-argument stack of the host engine — see engine.hpp: the log-round loops as one call each, and on top of them the stand-alone
// provers and verifiers of the inner-product, same-multiscalar, grand-product and same-permutation arguments on the caller's bases, many
// items per call.  Product code: every point operation below is a kernel launch.  The stack has three layers, each laid out by a plan
// header placed behind the one it wraps (loop_plan.hpp -> subarg_prove_plan.hpp / subarg_check_plan.hpp -> gprod_plan.hpp ->
// same_perm_plan.hpp) and each a set of functions here: core_* (inner product or same multiscalar), gprod_*, same_perm_*.  The two
// drivers, Engine::subarg_prove and Engine::subarg_verify, are lists of phases; what belongs to no single layer is called subarg_*.
// The MSM chain, CallScope and the tier-0 calls they share with msm_many are in engine.cpp.
#include "engine.hpp"
#include <algorithm>

namespace cpx {

// The log-round loops as one call each (include/cpx.h cpx_ipa_rounds, cpx_same_msm_rounds): inner_product_argument.rs:150-186 /
// same_multiscalar_argument.rs:99-136 for `count` independent items in the all-MSM form, laid out by loop_plan.hpp.  Per round the chain
// above over the round's 4 / 6 count cross terms (gathered from the uploaded bases: nothing is folded), k_finalize for their encodings,
// and one k_loop_step (loop.hip) for the transcript step, the folds and the next round's scalars: launches whose number does not
// depend on count, nothing returning to the host between the one upload and the one download.  fam: G | G' | H resp. G | T | U;
// vec: c | d resp. x.  The outputs are written when the call has succeeded, never before.
void Engine::ipa_rounds(size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* H, const uint8_t* vec_c, const uint8_t* vec_d,
                        uint8_t* transcripts, uint8_t* rounds_comp, uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas) {
  const uint8_t *fam[3] = {G, G_prime, H}, *vec[2] = {vec_c, vec_d};
  loop_rounds(true, count, n, fam, vec, transcripts, rounds_comp, rounds_aff, finals, gammas);
}
void Engine::same_msm_rounds(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* vec_x, uint8_t* transcripts,
                             uint8_t* rounds_comp, uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas) {
  const uint8_t *fam[3] = {G, T, U}, *vec[2] = {vec_x, nullptr};
  loop_rounds(false, count, n, fam, vec, transcripts, rounds_comp, rounds_aff, finals, gammas);
}
void Engine::loop_rounds(bool ipa, size_t count, size_t n, const uint8_t* const fam[3], const uint8_t* const vec[2], uint8_t* transcripts, uint8_t* rounds_comp,
                         uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas) {
  if (!count) return;
  LoopPlan lp;
  switch (loop_plan(ipa, count, n, lp)) {
    case LOOP_NOT_POW2: throw std::invalid_argument("the log-round loops take n = 2^L elements per item, L >= 0");
    case LOOP_TOO_LARGE: throw ArgError(ipa ? "cpx_ipa_rounds: at most 16384 items and count (2 n + 2) <= 2^24 points per round"
                                            : "cpx_same_msm_rounds: at most 10922 items and 3 count n <= 2^24 points per round");
    default: break;
  }
  const size_t nvec = ipa ? 2 : 1, L = lp.L, NT = lp.tasks(), terms = (size_t)lp.terms();
  for (size_t v = 0; v < nvec; v++)
    for (size_t i = 0; i < count * n; i++)
      if (!fr_wire_reduced(vec[v] + i * sizeof(Fr))) throw ArgError("a scalar of a log-round loop is not reduced");
  for (size_t i = 0; i < count; i++)
    if (!transcript_state_valid(transcripts + i * kTranscriptBytes)) throw ArgError("a transcript state with pos > 165 or pos_begin > 166");
  if (n == 1) {   // no round: the finals are the inputs, the states stay
    for (size_t i = 0; i < count; i++)
      for (size_t v = 0; v < nvec; v++) memcpy(finals + (i * nvec + v) * sizeof(Fr), vec[v] + i * sizeof(Fr), sizeof(Fr));
    return;
  }
  // host memory the enqueued copies read or write: above the scope
  std::vector<MsmTask> tasks;
  std::vector<uint32_t> idx, lens;
  std::vector<Fr> hvec;
  std::vector<uint8_t> h_comp, h_aff, h_states, h_fr;
  Tier0MsmPlan pl;
  if (!lp.round_msm(pl, lens)) throw ArgError("a round of the loop exceeds the limits of cpx_g1_msm_many");
  CallScope call(this);
  pl.slices = msm_tblw_slices(opt_, (int)NT, 2, (int)pl.max_n);   // (every round has the same lengths)
  DevBuf<Aff>&db = t0_.a0, &daff = t0_.a1;
  DevBuf<Fr>& dfr = t0_.fr;
  DevBuf<Jac>& res = t0_.res;
  DevBuf<uint8_t>& dcomp = t0_.bytes;
  db.ensure(count * lp.base_stride());
  dfr.ensure(lp.fr_total());
  res.ensure(lp.results());
  daff.ensure(lp.results());
  dcomp.ensure(lp.results() * 48);
  t0_.lidx.ensure(lp.idx_total());
  t0_.lstate.ensure(count * kTranscriptWords);
  msm_chain_reserve(pl);
  t0_.mtask.ensure(L * NT);
  // ---- the one upload: bases item by item, vectors with unit fold coefficients, index lists, every round's tasks, states
  const size_t pitch = lp.base_stride() * sizeof(Aff);
  for (int f = 0; f < 3; f++) {
    const size_t each = ipa && f == 2 ? 1 : n, off = ipa && f == 2 ? lp.h_index() : lp.family_off(f);
    CPX_HIP(hipMemcpy2DAsync(db.p + off, pitch, fam[f], each * sizeof(Aff), each * sizeof(Aff), count, hipMemcpyHostToDevice, stream_));
  }
  hvec.assign(count * lp.vec_words() + (ipa ? count : 0), Fr::one());
  for (size_t i = 0; i < count; i++)
    for (size_t v = 0; v < nvec; v++) memcpy(&hvec[i * lp.vec_words() + v * n], vec[v] + i * n * sizeof(Fr), n * sizeof(Fr));
  Fr* const d_vec = dfr.p + lp.fr_vec();
  Fr* const d_ones = dfr.p + lp.fr_ones();
  CPX_HIP(hipMemcpyAsync(d_vec, hvec.data(), count * lp.vec_words() * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (ipa) CPX_HIP(hipMemcpyAsync(d_ones, hvec.data() + count * lp.vec_words(), count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  loop_rounds_lists(lp, pl, idx, tasks);
  CPX_HIP(hipMemcpyAsync(t0_.lstate.p, transcripts, count * kTranscriptBytes, hipMemcpyHostToDevice, stream_));
  loop_rounds_resident(lp, pl);
  // ---- the one download, into host memory of the call: the caller's buffers are written once everything has arrived
  h_states.resize(count * kTranscriptBytes);
  h_fr.resize((count * L + count * lp.finals_each()) * sizeof(Fr));   // gammas | finals, as they sit in the Fr memory
  CPX_HIP(hipMemcpyAsync(h_states.data(), t0_.lstate.p, h_states.size(), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(h_fr.data(), dfr.p + lp.fr_gammas(), h_fr.size(), hipMemcpyDeviceToHost, stream_));
  if (rounds_comp) {
    h_comp.resize(lp.results() * 48);
    CPX_HIP(hipMemcpyAsync(h_comp.data(), dcomp.p, h_comp.size(), hipMemcpyDeviceToHost, stream_));
  }
  if (rounds_aff) {
    h_aff.resize(lp.results() * sizeof(Aff));
    CPX_HIP(hipMemcpyAsync(h_aff.data(), daff.p, h_aff.size(), hipMemcpyDeviceToHost, stream_));
  }
  call.finish();
  memcpy(transcripts, h_states.data(), h_states.size());
  memcpy(finals, h_fr.data() + count * L * sizeof(Fr), count * lp.finals_each() * sizeof(Fr));
  if (gammas) memcpy(gammas, h_fr.data(), count * L * sizeof(Fr));
  // device order [L][count][terms] -> the caller's [count][L][terms]
  for (size_t i = 0; i < count; i++)
    for (size_t j = 0; j < L; j++) {
      const size_t src = lp.result_index(j, i, 0), dst = (i * L + j) * terms;
      if (rounds_comp) memcpy(rounds_comp + dst * 48, h_comp.data() + src * 48, terms * 48);
      if (rounds_aff) memcpy(rounds_aff + dst * sizeof(Aff), h_aff.data() + src * sizeof(Aff), terms * sizeof(Aff));
    }
}
// The two halves of the loop that cpx_ipa_rounds / cpx_same_msm_rounds share with cpx_ipa_prove / cpx_same_msm_prove, inside the caller's
// scope and after its last ensure(), on the tier-0 buffers at the offsets of loop_plan.hpp: bases in t0_.a0, Fr memory in t0_.fr, sums in
// t0_.res, their affine forms in t0_.a1 and encodings in t0_.bytes, states in t0_.lstate.
// ... what of the upload depends on (count, n) alone: the index lists of every round and every round's tasks.  idx, tasks: the caller's,
// declared above its scope (enqueued copies read them)
void Engine::loop_rounds_lists(const LoopPlan& lp, const Tier0MsmPlan& pl, std::vector<uint32_t>& idx, std::vector<MsmTask>& tasks) {
  const size_t count = lp.count, L = lp.L, NT = lp.tasks(), terms = (size_t)lp.terms();
  Fr* const d_rows = t0_.fr.p + lp.fr_rows();
  lp.fill_idx(idx);
  CPX_HIP(hipMemcpyAsync(t0_.lidx.p, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  tasks.resize(L * NT);
  for (size_t j = 0; j < L; j++)
    for (size_t i = 0; i < count; i++)
      for (int q = 0; q < (int)terms; q++) {
        const size_t k = i * terms + (size_t)q;
        tasks[j * NT + k] = MsmTask{t0_.a0.p + i * lp.base_stride() + lp.family_off(lp.term_family(q)), t0_.lidx.p + lp.idx_off(j, lp.term_hi(q)),
                                    d_rows + i * lp.row_words() + lp.scal_off(q), lp.term_len(q), 0, pl.conv_off[k]};
      }
  CPX_HIP(hipMemcpyAsync(t0_.mtask.p, tasks.data(), tasks.size() * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
}
// ... and the rounds themselves, on vectors, unit coefficients, bases, lists, tasks and states that are on the device
void Engine::loop_rounds_resident(const LoopPlan& lp, const Tier0MsmPlan& pl) {
  const bool ipa = lp.ipa;
  const size_t count = lp.count, n = lp.n, L = lp.L, NT = lp.tasks();
  Fr* const d_vec = t0_.fr.p + lp.fr_vec();
  Fr* const d_rows = t0_.fr.p + lp.fr_rows();
  Jac* const res = t0_.res.p;
  Aff* const daff = t0_.a1.p;
  uint8_t* const dcomp = t0_.bytes.p;
  const LoopDev ld{d_vec, d_rows, t0_.fr.p + lp.fr_gammas(), t0_.fr.p + lp.fr_finals(), t0_.lstate.p, dcomp, (int)count, (int)n, (int)L};
  if (ipa) launch_ipa_round_scalars(d_vec, (int)count, (int)n, (int)(n / 2), t0_.fr.p + lp.fr_ones(), d_rows, stream_);
  else launch_smsm_round_scalars(d_vec, (int)count, (int)n, (int)(n / 2), d_rows, stream_);
  for (size_t j = 0; j < L; j++) {
    msm_chain_run(pl, t0_.mtask.p + j * NT, res + j * NT);
    tick("k_finalize", 0, (double)NT);
    launch_finalize(res + j * NT, (int)NT, daff + j * NT, nullptr, dcomp + j * NT * 48, stream_);
    tock();
    tick("k_loop_step", 0, (double)count, true);
    launch_loop_step(ipa, ld, (int)j, stream_);
    tock();
  }
}
// ------------------------------------------------------------------ the provers
// How deep a call goes: the core alone, the grand-product layer ahead of the inner-product core, the same-permutation layer ahead of both
enum class SubargDepth { Ipa, SameMsm, Gprod, SamePerm };

// What an entry point hands to the driver: the depth and the inputs of the layers that exist at that depth
struct SubargProveArgs {
  SubargDepth depth;
  size_t count, n;   // n = ell + nb above the core
  // every depth: exactly one of rand and rng_states is given
  const uint8_t* rand;
  uint8_t *rng_states, *transcripts, *proofs, *challenges;
  int* status;
  // the core alone.  fam: G | G' resp. G | T | U; stmt: crs_H | C | D resp. A | Z_t | Z_u; vec: c | d resp. x
  const uint8_t *fam[3] = {}, *stmt[3] = {}, *z = nullptr, *vec[2] = {};
  // grand product and same permutation
  size_t ell = 0, nb = 0;
  const uint8_t *G = nullptr, *H = nullptr, *crs_U = nullptr;
  // grand product alone (the same-permutation layer makes them on the device)
  const uint8_t *B = nullptr, *result = nullptr, *vec_b = nullptr, *vec_b_blinders = nullptr;
  // same permutation
  const uint8_t *A = nullptr, *M = nullptr, *vec_a = nullptr;
  const uint32_t* perm = nullptr;
  const uint8_t *vec_a_blinders = nullptr, *vec_m_blinders = nullptr;
};

// One prover call: plans and totals, the MSM plans, every host vector an enqueued copy reads or writes, the device pointers.  Declared
// above the call's CallScope (engine.hpp), so all of it outlives the scope's wait.
struct SubargProveCall {
  const SubargProveArgs& a;
  const bool ipa, gp, sm;   // the core is the inner-product prover; the grand-product layer is there; the same-permutation layer is there
  const size_t count, n, ell, nb;
  SamePermProvePlan spl;   // (sm: the regions of the same-permutation layer behind those of the grand-product layer, gp: those behind the inner-product prover's)
  GprodProvePlan& gpl = spl.gp;
  SubargProvePlan& sp = gpl.sp;
  LoopPlan& lp = sp.lp;
  SubargTotals tot{};                 // of the outermost plan in use
  size_t gp_byte = 0, gp_chal = 0;    // where the grand-product layer's bytes and challenges start in an item's outputs: behind the same-permutation layer's
  size_t L = 0, NT = 0, NF = 0, DE = 0, DT = 0;   // DT: the caller's draws per item, the grand product's nb ahead of the core's DE
  Tier0MsmPlan pl, plb, plg, plm;     // a round | the B points | the C and D tasks | the same-permutation B tasks
  std::vector<MsmTask> tasks, btasks, gtasks, mtasks;
  std::vector<SmulTask> stasks;
  std::vector<uint32_t> idx, lens, blens, glens, addend, mlens, m_gather, m_addend;
  std::vector<Fr> hwit, h_fr, h_ab, h_gp, h_sm;
  std::vector<uint8_t> h_comp, h_states, h_flags, h_rng, h_smB;
  // the tier-0 buffers of the call, once subarg_prove_reserve has sized them
  Aff *db = nullptr, *daff = nullptr;   // the loop's item rows | affine forms
  Fr* dfr = nullptr;
  Jac *res = nullptr, *din = nullptr, *d_stmt = nullptr;
  uint8_t *dby = nullptr, *dflag = nullptr, *d_rng = nullptr;
  uint32_t* dix = nullptr;
  MsmTask *dtask = nullptr, *d_btasks = nullptr;
  uint64_t* dstate = nullptr;
  size_t pitch = 0;   // of an item's row, in bytes
  SubargProveDev sd{};
  GprodDev gd{};

  explicit SubargProveCall(const SubargProveArgs& args);
  void check() const;
  void msm_plans();
};

// the plans, by whose status a call is refused first
SubargProveCall::SubargProveCall(const SubargProveArgs& args)
    : a(args), ipa(args.depth != SubargDepth::SameMsm), gp(args.depth == SubargDepth::Gprod || args.depth == SubargDepth::SamePerm), sm(args.depth == SubargDepth::SamePerm),
      count(args.count), n(args.n), ell(args.ell), nb(args.nb) {
  if (gp) {
    switch (gprod_prove_plan(count, ell, nb, gpl)) {
      case GPROD_NO_FACTOR: throw ArgError("cpx_gprod_prove: ell = 0 has no first prefix product (the reference's ell - 1 underflows)");
      case GPROD_NOT_POW2: throw std::invalid_argument("the grand-product prover takes ell + n_blinders = 2^L elements per item");
      case GPROD_TOO_LARGE: throw ArgError("cpx_gprod_prove: at most 16384 items and count (2 n + 2) <= 2^24 points per round");
      case GPROD_NO_BLINDERS: throw ArgError("cpx_gprod_prove: n = 1 has no blinders (the reference's n - 2 underflows)");
      default: break;
    }
  } else {
    switch (subarg_prove_plan(ipa, count, n, sp)) {
      case LOOP_NOT_POW2: throw std::invalid_argument("the sub-argument provers take n = 2^L elements per item, L >= 0");
      case LOOP_TOO_LARGE: throw ArgError(ipa ? "cpx_ipa_prove: at most 16384 items and count (2 n + 2) <= 2^24 points per round"
                                              : "cpx_same_msm_prove: at most 10922 items and 3 count n <= 2^24 points per round");
      default: break;
    }
    if (ipa && n == 1) throw ArgError("cpx_ipa_prove: n = 1 has no blinders (the reference's n - 2 underflows)");
  }
  tot = sm ? spl.totals() : gp ? gpl.totals() : sp.totals();
  if (gp) {
    const SubargTotals g = gpl.totals();
    gp_byte = tot.lead_bytes - g.lead_bytes;
    gp_chal = tot.lead_challenges - g.lead_challenges;
  }
  L = lp.L, NT = lp.tasks(), NF = sp.first(), DE = sp.draws_each(), DT = DE + nb;
}

static void same_perm_prove_check(const SubargProveCall& c) {
  const uint8_t* const sc[3] = {c.a.vec_a, c.a.vec_a_blinders, c.a.vec_m_blinders};
  const size_t each[3] = {c.ell, c.nb, c.nb};
  for (int v = 0; v < 3; v++)
    for (size_t i = 0; i < c.count * each[v]; i++)
      if (!fr_wire_reduced(sc[v] + i * sizeof(Fr))) throw ArgError("a scalar of cpx_same_perm_prove is not reduced");
  for (size_t i = 0; i < c.count * c.ell; i++)   // the reference indexes vec_a out of bounds (util.rs:78)
    if (c.a.perm[i] >= c.ell) throw ArgError("cpx_same_perm_prove: a permutation entry >= ell");
}
static void gprod_prove_check(const SubargProveCall& c) {
  const uint8_t* const sc[3] = {c.a.result, c.a.vec_b, c.a.vec_b_blinders};
  const size_t each[3] = {1, c.ell, c.nb};
  for (int v = 0; v < 3; v++)
    for (size_t i = 0; i < c.count * each[v]; i++)
      if (!fr_wire_reduced(sc[v] + i * sizeof(Fr))) throw ArgError("a scalar of cpx_gprod_prove is not reduced");
}
static void core_prove_check(const SubargProveCall& c) {
  for (size_t v = 0; v < c.sp.nvec(); v++)
    for (size_t i = 0; i < c.count * c.n; i++)
      if (!fr_wire_reduced(c.a.vec[v] + i * sizeof(Fr))) throw ArgError("a witness scalar of a sub-argument prover is not reduced");
  if (c.ipa)
    for (size_t i = 0; i < c.count; i++)
      if (!fr_wire_reduced(c.a.z + i * sizeof(Fr))) throw ArgError("a scalar z of cpx_ipa_prove is not reduced");
}
// the draws or rng positions, the scalars of the outermost layer (the layers below it get theirs from the device), the transcript states
void SubargProveCall::check() const {
  if (a.rng_states) {   // (the limits of one k_rng_draw launch, as cpx_rng_fr has them)
    if (DT > ((size_t)1 << 20) || count * DT > ((size_t)1 << 26)) throw ArgError("rng draws: at most 2^20 draws per stream and 2^26 per call");
    for (size_t i = 0; i < count; i++) {
      uint64_t pos;
      memcpy(&pos, a.rng_states + i * RNG_STATE_BYTES + 32, 8);
      if (!rng_pos_valid(pos)) throw ArgError("rng state: word_pos within 2^32 words of 2^64");
    }
  } else {
    for (size_t i = 0; i < count * DT; i++)
      if (!fr_wire_reduced(a.rand + i * sizeof(Fr))) throw ArgError("a draw of a sub-argument prover is not reduced");
  }
  if (sm) same_perm_prove_check(*this);
  else if (gp) gprod_prove_check(*this);
  else core_prove_check(*this);
  for (size_t i = 0; i < count; i++)
    if (!transcript_state_valid(a.transcripts + i * kTranscriptBytes)) throw ArgError("a transcript state with pos > 165 or pos_begin > 166");
}
// the MSM plans, from the core outwards (a layer's tasks stay below a round's: the plan headers)
void SubargProveCall::msm_plans() {
  if (L && !lp.round_msm(pl, lens)) throw ArgError("a round of the loop exceeds the limits of cpx_g1_msm_many");
  if (!sp.first_msm(plb, blens)) throw ArgError("the B points exceed the limits of cpx_g1_msm_many");
  if (gp && !gpl.item_msm(plg, glens)) throw ArgError("the C and D tasks exceed the limits of cpx_g1_msm_many");
  if (sm && !spl.item_msm(plm, mlens)) throw ArgError("the B tasks exceed the limits of cpx_g1_msm_many");
}

// The stand-alone sub-argument provers (include/cpx.h cpx_ipa_prove, cpx_same_msm_prove and their _rng forms): InnerProductProof::new
// (inner_product_argument.rs:98-199) / SameMultiscalarProof::new (same_multiscalar_argument.rs:69-150) for `count` independent items, laid
// out by subarg_prove_plan.hpp on top of loop_plan.hpp.  One upload (the bases straight into the loop's item rows); the draws uploaded or
// made by k_rng_draw; IPA: k_subarg_blinders; the MSM chain over the 2 / 3 count B points; k_finalize over them and the 3 count statement
// points; SameMSM: k_compress over T | U; k_subarg_prove_setup (subarg_prove.hip); IPA: k_smul for H = beta crs_H into the items' rows;
// then the rounds of loop_rounds_resident; one download; one synchronisation.  The launches do not depend on count.  The outputs are
// written when the call has succeeded, never before.
void Engine::ipa_prove(size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D, const uint8_t* z,
                       const uint8_t* vec_c, const uint8_t* vec_d, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs,
                       uint8_t* challenges, int* status) {
  SubargProveArgs a{SubargDepth::Ipa, count, n, rand, rng_states, transcripts, proofs, challenges, status};
  a.fam[0] = G, a.fam[1] = G_prime, a.stmt[0] = crs_H, a.stmt[1] = C, a.stmt[2] = D, a.z = z, a.vec[0] = vec_c, a.vec[1] = vec_d;
  subarg_prove(a);
}
void Engine::same_msm_prove(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t, const uint8_t* Z_u,
                            const uint8_t* vec_x, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  SubargProveArgs a{SubargDepth::SameMsm, count, n, rand, rng_states, transcripts, proofs, challenges, status};
  a.fam[0] = G, a.fam[1] = T, a.fam[2] = U, a.stmt[0] = A, a.stmt[1] = Z_t, a.stmt[2] = Z_u, a.vec[0] = vec_x;
  subarg_prove(a);
}
// The grand-product prover (include/cpx.h cpx_gprod_prove and its _rng form): GrandProductProof::new (grand_product_argument.rs:43-166) for
// `count` independent items, laid out by gprod_plan.hpp on top of subarg_prove_plan.hpp.  It is the inner-product prover with the
// grand-product layer ahead of its steps: G | H uploaded into both families of the loop's item rows (G' is never formed), k_finalize
// over B, k_gprod_products, the MSM chain over the C tasks, k_finalize over C, k_gprod_setup (gprod.hip), the MSM chain over the D tasks
// — B is added to their sums by the k_finalize that normalises the statement points —, then the inner-product prover with k_gprod_rdu
// behind k_subarg_blinders (B_d's scalars are r_d o u) and u as the fold coefficients of G'.
void Engine::gprod_prove(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B, const uint8_t* gprod_result,
                         const uint8_t* vec_b, const uint8_t* vec_b_blinders, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs,
                         uint8_t* challenges, int* status) {
  SubargProveArgs a{SubargDepth::Gprod, count, ell + n_blinders, rand, rng_states, transcripts, proofs, challenges, status};
  a.ell = ell, a.nb = n_blinders, a.G = G, a.H = H, a.crs_U = crs_U, a.B = B, a.result = gprod_result, a.vec_b = vec_b, a.vec_b_blinders = vec_b_blinders;
  subarg_prove(a);
}
// The same-permutation prover (include/cpx.h cpx_same_perm_prove and its _rng form): SamePermutationProof::new
// (same_permutation_argument.rs:40-99) for `count` independent items, laid out by same_perm_plan.hpp on top of gprod_plan.hpp.  It is
// gprod_prove above with the same-permutation layer ahead: k_finalize over A | M, k_same_perm_step (same_perm.hip) and the MSM chain over
// the B tasks, whose sums land where the grand-product layer reads B; its k_finalize adds A.  Nothing returns to the host in between.
void Engine::same_perm_prove(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A, const uint8_t* M,
                             const uint8_t* vec_a, const uint32_t* permutation, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders, const uint8_t* rand,
                             uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  SubargProveArgs a{SubargDepth::SamePerm, count, ell + n_blinders, rand, rng_states, transcripts, proofs, challenges, status};
  a.ell = ell, a.nb = n_blinders, a.G = G, a.H = H, a.crs_U = crs_U;
  a.A = A, a.M = M, a.vec_a = vec_a, a.perm = permutation, a.vec_a_blinders = vec_a_blinders, a.vec_m_blinders = vec_m_blinders;
  subarg_prove(a);
}

// every buffer of the call from the totals of the outermost plan, before the first launch (ensure() may free a buffer); then the pointers
void Engine::subarg_prove_reserve(SubargProveCall& c) {
  const SubargTotals& t = c.tot;
  if (c.L) c.pl.slices = msm_tblw_slices(opt_, (int)c.NT, 2, (int)c.pl.max_n);
  c.plb.slices = msm_tblw_slices(opt_, (int)c.plb.count, 2, (int)c.plb.max_n);
  if (c.gp) c.plg.slices = msm_tblw_slices(opt_, (int)c.plg.count, 2, (int)c.plg.max_n);
  if (c.sm) c.plm.slices = msm_tblw_slices(opt_, (int)c.plm.count, 2, (int)c.plm.max_n);
  t0_.a0.ensure(c.count * c.lp.base_stride());
  t0_.fr.ensure(t.fr);
  t0_.res.ensure(std::max<size_t>(t.res, 1));
  t0_.jin.ensure(t.jac);
  t0_.a1.ensure(t.aff);
  t0_.bytes.ensure(t.bytes);
  t0_.status.ensure(t.flags);
  t0_.lidx.ensure(std::max<size_t>(t.ix, 1));
  t0_.lstate.ensure(c.count * kTranscriptWords);
  if (c.L) msm_chain_reserve(c.pl);
  msm_chain_reserve(c.plb);
  if (c.gp) msm_chain_reserve(c.plg);
  if (c.sm) msm_chain_reserve(c.plm);
  t0_.mtask.ensure(t.tasks);
  if (c.ipa) t0_.stask.ensure(c.count);
  c.db = t0_.a0.p, c.daff = t0_.a1.p, c.dfr = t0_.fr.p, c.res = t0_.res.p, c.din = t0_.jin.p, c.dby = t0_.bytes.p, c.dflag = t0_.status.p;
  c.dix = t0_.lidx.p, c.dtask = t0_.mtask.p, c.dstate = t0_.lstate.p;
  c.pitch = c.lp.base_stride() * sizeof(Aff);
  c.d_stmt = c.din + c.sp.pt_statement(0, 0);
  c.d_rng = c.dby + c.sp.by_rng();
  c.d_btasks = c.dtask + c.sp.task_first();
  c.sd = SubargProveDev{c.sp, c.dfr, c.dfr + c.lp.fr_vec(), c.dfr + c.lp.fr_ones(), c.dfr + c.lp.fr_finals(), c.dby, c.dflag, c.dstate, c.gp ? c.dfr + c.gpl.fr_u() : nullptr};
  c.gd = GprodDev{c.gpl, c.dfr, c.dby, c.dflag, c.dstate};
}

// ---- the upload: bases into the loop's item rows, statement points, witness, z, draws or rng states, lists, tasks, states
// G | H is family 0 and family 1; crs_U into the IPA's crs_H slot; C and D are made below
void Engine::gprod_prove_upload_bases(SubargProveCall& c) {
  const size_t K = SubargProvePlan::kStatement;
  for (int f = 0; f < 2; f++) {
    CPX_HIP(hipMemcpy2DAsync(c.db + c.lp.family_off(f), c.pitch, c.a.G, c.ell * sizeof(Aff), c.ell * sizeof(Aff), c.count, hipMemcpyHostToDevice, stream_));
    if (c.nb) CPX_HIP(hipMemcpy2DAsync(c.db + c.lp.family_off(f) + c.ell, c.pitch, c.a.H, c.nb * sizeof(Aff), c.nb * sizeof(Aff), c.count, hipMemcpyHostToDevice, stream_));
  }
  CPX_HIP(hipMemcpy2DAsync(c.d_stmt, K * sizeof(Jac), c.a.crs_U, sizeof(Jac), sizeof(Jac), c.count, hipMemcpyHostToDevice, stream_));
}
// A, M, vec_a, the permutation and the two blinder vectors instead of B, gprod_result, vec_b and vec_b_blinders; the B tasks and their lists
void Engine::same_perm_prove_upload(SubargProveCall& c) {
  const SamePermProvePlan& spl = c.spl;
  const size_t count = c.count, ell = c.ell, nb = c.nb;
  CPX_HIP(hipMemcpyAsync(c.din + spl.jac_A(), c.a.A, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.din + spl.jac_M(), c.a.M, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dfr + spl.fr_a(), c.a.vec_a, count * ell * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dix + spl.ix_perm(), c.a.perm, count * ell * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  if (nb) {
    CPX_HIP(hipMemcpyAsync(c.dfr + spl.fr_ra(), c.a.vec_a_blinders, count * nb * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(c.dfr + spl.fr_rm(), c.a.vec_m_blinders, count * nb * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  spl.fill_lists(c.m_gather, c.m_addend);
  CPX_HIP(hipMemcpyAsync(c.dix + spl.ix_gather(), c.m_gather.data(), c.m_gather.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dix + spl.ix_addend(), c.m_addend.data(), c.m_addend.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  c.mtasks.resize(count);
  for (size_t i = 0; i < count; i++)   // B - A = beta sum G + alpha M
    c.mtasks[i] = MsmTask{c.db + i * c.lp.base_stride(), c.dix + spl.ix_gather(), c.dfr + spl.fr_bsc() + i * (ell + 1), (uint32_t)(ell + 1), 0, c.plm.conv_off[i]};
  CPX_HIP(hipMemcpyAsync(c.dtask + spl.task_B(), c.mtasks.data(), c.mtasks.size() * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
}
// B, gprod_result, vec_b and vec_b_blinders unless the same-permutation layer makes them; vec_c_blinders and the IPA's draws; the addend
// list; the C and D tasks
void Engine::gprod_prove_upload(SubargProveCall& c) {
  const GprodProvePlan& gpl = c.gpl;
  const size_t count = c.count, n = c.n, ell = c.ell, nb = c.nb;
  if (!c.sm) {
    CPX_HIP(hipMemcpyAsync(c.din + gpl.pt_B(0), c.a.B, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(c.dfr + gpl.fr_result(), c.a.result, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(c.dfr + gpl.fr_b(), c.a.vec_b, count * ell * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    if (nb) CPX_HIP(hipMemcpyAsync(c.dfr + gpl.fr_rb(), c.a.vec_b_blinders, count * nb * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  if (!c.a.rng_states) {   // per item vec_c_blinders | the IPA's draws
    if (nb) CPX_HIP(hipMemcpy2DAsync(c.dfr + gpl.fr_cbl(), nb * sizeof(Fr), c.a.rand, c.DT * sizeof(Fr), nb * sizeof(Fr), count, hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpy2DAsync(c.dfr + c.sp.fr_draws(), c.DE * sizeof(Fr), c.a.rand + nb * sizeof(Fr), c.DT * sizeof(Fr), c.DE * sizeof(Fr), count, hipMemcpyHostToDevice, stream_));
  }
  gpl.fill_addend(c.addend);
  CPX_HIP(hipMemcpyAsync(c.dix + gpl.ix_addend(), c.addend.data(), c.addend.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  c.gtasks.resize(2 * count);
  for (size_t i = 0; i < count; i++) {   // C = <c, G | H>; D - B = <D's scalars, G | H>
    c.gtasks[i] = MsmTask{c.db + i * c.lp.base_stride() + c.lp.family_off(0), nullptr, c.dfr + c.sp.fr_wit() + i * 2 * n, (uint32_t)n, 0, c.plg.conv_off[i]};
    c.gtasks[count + i] = MsmTask{c.db + i * c.lp.base_stride() + c.lp.family_off(0), nullptr, c.dfr + gpl.fr_dsc() + i * n, (uint32_t)n, 0, c.plg.conv_off[i]};
  }
  CPX_HIP(hipMemcpyAsync(c.dtask + gpl.task_C(), c.gtasks.data(), c.gtasks.size() * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
}
// the core alone: the caller's bases, statement points, witness, z and draws
void Engine::core_prove_upload(SubargProveCall& c) {
  const size_t count = c.count, n = c.n, nvec = c.sp.nvec(), K = SubargProvePlan::kStatement;
  for (int f = 0; f < (c.ipa ? 2 : 3); f++)
    CPX_HIP(hipMemcpy2DAsync(c.db + c.lp.family_off(f), c.pitch, c.a.fam[f], n * sizeof(Aff), n * sizeof(Aff), count, hipMemcpyHostToDevice, stream_));
  for (size_t k = 0; k < K; k++)
    CPX_HIP(hipMemcpy2DAsync(c.d_stmt + k, K * sizeof(Jac), c.a.stmt[k], sizeof(Jac), sizeof(Jac), count, hipMemcpyHostToDevice, stream_));
  c.hwit.resize(count * nvec * n);
  for (size_t i = 0; i < count; i++)
    for (size_t v = 0; v < nvec; v++) memcpy(&c.hwit[(i * nvec + v) * n], c.a.vec[v] + i * n * sizeof(Fr), n * sizeof(Fr));
  CPX_HIP(hipMemcpyAsync(c.dfr + c.sp.fr_wit(), c.hwit.data(), c.hwit.size() * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (c.ipa) CPX_HIP(hipMemcpyAsync(c.dfr + c.sp.fr_z(), c.a.z, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (!c.a.rng_states) CPX_HIP(hipMemcpyAsync(c.dfr + c.sp.fr_draws(), c.a.rand, count * c.DE * sizeof(Fr), hipMemcpyHostToDevice, stream_));
}
// what the core uploads at every depth: the loop's lists and tasks, the B tasks, the states
void Engine::subarg_prove_upload_tasks(SubargProveCall& c) {
  const size_t count = c.count, n = c.n, NF = c.NF;
  if (c.L) loop_rounds_lists(c.lp, c.pl, c.idx, c.tasks);
  const Fr* const d_rd = c.dfr + (c.gp ? c.gpl.fr_rdu() : c.sp.fr_rd());   // the hand-off slot of B_d's scalars: r_d, or the grand-product layer's r_d o u
  c.btasks.resize(count * NF);
  for (size_t i = 0; i < count; i++)
    for (size_t b = 0; b < NF; b++) {   // IPA: G r_c, G' r_d (grand product: G (r_d o u)); SameMSM: G r, T r, U r
      const Fr* sc = c.ipa && b == 1 ? d_rd + i * n : c.dfr + c.sp.fr_draws() + i * c.DE;
      c.btasks[i * NF + b] = MsmTask{c.db + i * c.lp.base_stride() + c.lp.family_off(c.sp.first_family(b)), nullptr, sc, (uint32_t)n, 0, c.plb.conv_off[i * NF + b]};
    }
  CPX_HIP(hipMemcpyAsync(c.d_btasks, c.btasks.data(), c.btasks.size() * sizeof(MsmTask), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dstate, c.a.transcripts, count * kTranscriptBytes, hipMemcpyHostToDevice, stream_));
}

// ---- the steps before the loop
// the _rng forms: every item's stream draws the grand product's vec_c_blinders, then the core's draws
void Engine::subarg_prove_draw(SubargProveCall& c) {
  tick("k_rng_draw", (double)(c.count * c.DT * sizeof(Fr)), (double)(c.count * c.DT));
  if (c.nb) launch_rng_draw(rng_draw_args(c.d_rng, nullptr, c.count, 0, nullptr, {{c.nb, c.dfr + c.gpl.fr_cbl()}, {c.DE, c.dfr + c.sp.fr_draws()}}), stream_);
  else launch_rng_draw(rng_draw_args(c.d_rng, nullptr, c.count, 0, nullptr, {{c.DE, c.dfr + c.sp.fr_draws()}}), stream_);
  tock();
}
// the same-permutation layer: the encodings of A and M, step 1 with the factors, their product and vec_b_blinders, B - A.  Hands to the
// grand-product layer: vec_b, gprod_result, vec_b_blinders in its Fr regions, the B sums in its B slots, A's slots in the addend list
void Engine::same_perm_prove_steps(SubargProveCall& c) {
  const SamePermProvePlan& spl = c.spl;
  const size_t count = c.count;
  tick("k_finalize", 0, 2.0 * count);
  launch_finalize(c.din + spl.jac_A(), (int)(2 * count), c.daff + spl.aff_A(), nullptr, c.dby + spl.by_A(), stream_);
  tock();
  CPX_HIP(hipMemcpy2DAsync(c.db + c.lp.h_index(), c.pitch, c.daff + spl.aff_M(), sizeof(Aff), sizeof(Aff), count, hipMemcpyDeviceToDevice, stream_));
  tick("k_same_perm_step", 0, (double)count, true);
  launch_same_perm_step(SamePermDev{spl, c.dfr, c.dby, c.dix + spl.ix_perm(), c.dstate}, stream_);
  tock();
  msm_chain_run(c.plm, c.dtask + spl.task_B(), c.din + c.gpl.pt_B(0));
}
// the grand-product layer: B's encoding (same-permutation: A is added first), vec_c, C, steps 1 and 2 with vec_d and inner_prod, D - B.
// Hands to the core: its witness c | d and z in its Fr regions, C and D in its statement slots, B's slots in the addend list
void Engine::gprod_prove_steps(SubargProveCall& c) {
  const GprodProvePlan& gpl = c.gpl;
  const size_t count = c.count, K = SubargProvePlan::kStatement;
  tick("k_finalize", 0, (double)count);
  launch_finalize(c.din + gpl.pt_B(0), (int)count, c.daff + c.sp.aff_points() + gpl.pt_B(0), nullptr, c.dby + gpl.by_B(), stream_,
                  c.sm ? c.dix + c.spl.ix_addend() : nullptr);
  tock();
  tick("k_gprod_products", 0, (double)count, true);
  launch_gprod_products(c.gd, stream_);
  tock();
  msm_chain_run(c.plg, c.dtask + gpl.task_C(), c.res + gpl.res_C(0));
  tick("k_finalize", 0, (double)count);
  launch_finalize(c.res + gpl.res_C(0), (int)count, nullptr, nullptr, c.dby + gpl.by_C(), stream_);
  tock();
  tick("k_gprod_setup", 0, (double)count, true);
  launch_gprod_setup(c.gd, stream_);
  tock();
  msm_chain_run(c.plg, c.dtask + gpl.task_D(), c.res + gpl.res_D(0));
  CPX_HIP(hipMemcpy2DAsync(c.d_stmt + 1, K * sizeof(Jac), c.res + gpl.res_C(0), sizeof(Jac), sizeof(Jac), count, hipMemcpyDeviceToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(c.d_stmt + 2, K * sizeof(Jac), c.res + gpl.res_D(0), sizeof(Jac), sizeof(Jac), count, hipMemcpyDeviceToDevice, stream_));
}
// IPA: r_d and the flags of generate_ipa_blinders; SameMSM draws no such vector, its flags are clear
void Engine::core_prove_blinders(SubargProveCall& c) {
  if (c.ipa) {
    tick("k_subarg_blinders", 0, (double)c.count, true);
    launch_subarg_blinders(c.sd, stream_);
    tock();
  } else {
    CPX_HIP(hipMemsetAsync(c.dflag, 0, c.count, stream_));
  }
}
// B_d's scalars r_d o u, once the core has made r_d
void Engine::gprod_prove_rdu(SubargProveCall& c) {
  tick("k_gprod_rdu", 0, (double)c.count, true);
  launch_gprod_rdu(c.gd, stream_);
  tock();
}
// the B points, the normalised forms and encodings of them and of the statement points (grand product: B is added to the D sums), step 1
// with the rewrite of the vectors, IPA: H
void Engine::core_prove_steps(SubargProveCall& c) {
  const SubargProvePlan& sp = c.sp;
  const size_t count = c.count, n = c.n;
  msm_chain_run(c.plb, c.d_btasks, c.din);
  tick("k_finalize", 0, (double)sp.points());
  launch_finalize(c.din, (int)sp.points(), c.daff + sp.aff_points(), nullptr, c.dby + sp.by_points(), stream_, c.gp ? c.dix + c.gpl.ix_addend() : nullptr);
  tock();
  if (!c.ipa) {
    tick("k_compress", 0, 2.0 * count * n, true);
    launch_compress(c.db + c.lp.family_off(1), (int)(2 * n), (int)c.lp.base_stride(), (int)count, c.dby + sp.by_tu(), stream_);
    tock();
  }
  tick("k_subarg_prove_setup", 0, (double)count, true);
  launch_subarg_prove_setup(c.sd, stream_);
  tock();
  if (c.ipa) {   // H = beta crs_H (inner_product_argument.rs:140) into slot h_index() of the item's row
    c.stasks.resize(count);
    for (size_t i = 0; i < count; i++)
      c.stasks[i] = SmulTask{nullptr, c.daff + sp.aff_points() + sp.pt_statement(i, 0), c.db + i * c.lp.base_stride() + c.lp.h_index(), c.dfr + sp.fr_ab() + 2 * i + 1, 0, smul_flag()};
    CPX_HIP(hipMemcpyAsync(t0_.stask.p, c.stasks.data(), count * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
    smul_tasks(t0_.stask.p, count, 1, (double)count);
  }
}

// ---- the one download, into host memory of the call: the caller's buffers are written once everything has arrived.  The copies keep the
// order they have always had: the core's, the grand-product layer's, the same-permutation layer's, the rng states
void Engine::subarg_prove_download(SubargProveCall& c) {
  const size_t count = c.count;
  c.h_states.resize(count * kTranscriptBytes);
  c.h_fr.resize(count * c.L + count * c.lp.finals_each());   // gammas | finals, as they sit in the Fr memory
  c.h_ab.resize(count * c.sp.ab_each());
  c.h_comp.resize(c.sp.by_tu());                             // the round encodings | the B and statement encodings
  c.h_flags.resize(c.tot.flags);                             // grand product: behind the blinders' flags those of beta = 0
  CPX_HIP(hipMemcpyAsync(c.h_states.data(), c.dstate, c.h_states.size(), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_fr.data(), c.dfr + c.lp.fr_gammas(), c.h_fr.size() * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_ab.data(), c.dfr + c.sp.fr_ab(), c.h_ab.size() * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_comp.data(), c.dby, c.h_comp.size(), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_flags.data(), c.dflag, c.h_flags.size(), hipMemcpyDeviceToHost, stream_));
  if (c.gp) {
    c.h_gp.resize(3 * count);   // r_p | alpha, beta, as they sit in the Fr memory
    CPX_HIP(hipMemcpyAsync(c.h_gp.data(), c.dfr + c.gpl.fr_rp(), c.h_gp.size() * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  }
  if (c.sm) {
    c.h_sm.resize(2 * count);     // alpha, beta per item
    c.h_smB.resize(count * 48);   // B's encodings
    CPX_HIP(hipMemcpyAsync(c.h_sm.data(), c.dfr + c.spl.fr_chal(), c.h_sm.size() * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(c.h_smB.data(), c.dby + c.gpl.by_B(), c.h_smB.size(), hipMemcpyDeviceToHost, stream_));
  }
  if (c.a.rng_states) {
    c.h_rng.resize(count * RNG_STATE_BYTES);
    CPX_HIP(hipMemcpyAsync(c.h_rng.data(), c.d_rng, c.h_rng.size(), hipMemcpyDeviceToHost, stream_));
  }
}

// ---- the write-out of item i.  o: the item's proof bytes, ch: its challenges or null; every layer writes its own piece
// same_permutation_argument.rs:173-177: B, then the GrandProductProof
static void same_perm_write_proof(const SubargProveCall& c, size_t i, uint8_t* o, uint8_t* ch) {
  memcpy(o + c.spl.byte_B(), c.h_smB.data() + i * 48, 48);
  if (ch) memcpy(ch, c.h_sm.data() + 2 * i, 2 * sizeof(Fr));
}
// grand_product_argument.rs:248-253: C, r_p, then the InnerProductProof
static void gprod_write_proof(const SubargProveCall& c, size_t i, uint8_t* o, uint8_t* ch) {
  o += c.gp_byte;
  memcpy(o + c.gpl.byte_C(), c.h_comp.data() + c.sp.by_points() + c.sp.pt_statement(i, 1) * 48, 48);
  host::S(c.h_gp[i]).to_le_bytes(o + c.gpl.byte_rp());
  if (ch) memcpy(ch + c.gp_chal * sizeof(Fr), c.h_gp.data() + c.count + 2 * i, 2 * sizeof(Fr));
}
// inner_product_argument.rs:328-338, same_multiscalar_argument.rs:263-275: the B points, the blocks of round points, the finals; the state
static void core_write_proof(const SubargProveCall& c, size_t i, uint8_t* o, uint8_t* ch) {
  const SubargProvePlan& sp = c.sp;
  const LoopPlan& lp = c.lp;
  const size_t L = c.L, nlead = c.tot.lead_challenges;
  const Fr *const h_gam = c.h_fr.data(), *const h_fin = c.h_fr.data() + c.count * L;
  o += c.tot.lead_bytes;
  for (size_t b = 0; b < c.NF; b++) memcpy(o + sp.point_byte(b), c.h_comp.data() + sp.by_points() + sp.pt_first(i, b) * 48, 48);
  for (size_t b = 0; b < sp.blocks(); b++)
    for (size_t j = 0; j < L; j++) memcpy(o + sp.point_byte(sp.round_slot(j, b)), c.h_comp.data() + lp.result_index(j, i, sp.block_term(b)) * 48, 48);
  for (size_t v = 0; v < lp.finals_each(); v++) host::S(h_fin[i * lp.finals_each() + v]).to_le_bytes(o + sp.scalar_byte(v));
  memcpy(c.a.transcripts + i * kTranscriptBytes, c.h_states.data() + i * kTranscriptBytes, kTranscriptBytes);
  if (ch) {
    memcpy(ch + nlead * sizeof(Fr), c.h_ab.data() + i * sp.ab_each(), sp.ab_each() * sizeof(Fr));
    memcpy(ch + (nlead + sp.ab_each()) * sizeof(Fr), h_gam + i * L, L * sizeof(Fr));
  }
}
static void subarg_prove_write(const SubargProveCall& c) {
  const SubargProveArgs& a = c.a;
  if (a.rng_states) memcpy(a.rng_states, c.h_rng.data(), c.h_rng.size());   // (a refused item's stream has drawn too)
  const size_t PBT = c.tot.lead_bytes + c.sp.proof_bytes(), NCT = c.tot.lead_challenges + c.sp.challenges();
  for (size_t i = 0; i < c.count; i++) {
    uint8_t* const o = a.proofs + i * PBT;
    uint8_t* const ch = a.challenges ? a.challenges + i * NCT * sizeof(Fr) : nullptr;
    if (c.h_flags[i] || (c.gp && c.h_flags[c.gpl.flag_beta() + i])) {   // the reference panics (generate_ipa_blinders; beta = 0): zero bytes, zero challenges, the state as it came
      memset(o, 0, PBT);
      if (ch) memset(ch, 0, NCT * sizeof(Fr));
      a.status[i] = CPX_ERR_ARG;
      continue;
    }
    if (c.sm) same_perm_write_proof(c, i, o, ch);
    if (c.gp) gprod_write_proof(c, i, o, ch);
    core_write_proof(c, i, o, ch);
    a.status[i] = CPX_OK;
  }
}

// The one driver of the four provers.  The phases are fixed; in each the same-permutation layer goes first, then the grand-product
// layer, then the core — except where the stream has always had another order, which is kept: the MSM plans and the downloads go from
// the core outwards, the grand product's bases go up ahead of the same-permutation layer's inputs.
void Engine::subarg_prove(const SubargProveArgs& a) {
  if (!a.count) return;
  SubargProveCall c(a);   // the plans and their totals; above the scope with everything an enqueued copy reads or writes
  c.check();
  c.msm_plans();
  CallScope call(this);
  subarg_prove_reserve(c);
  if (a.rng_states) CPX_HIP(hipMemcpyAsync(c.d_rng, a.rng_states, c.count * RNG_STATE_BYTES, hipMemcpyHostToDevice, stream_));
  if (c.gp) gprod_prove_upload_bases(c);
  if (c.sm) same_perm_prove_upload(c);
  if (c.gp) gprod_prove_upload(c);
  else core_prove_upload(c);
  subarg_prove_upload_tasks(c);
  if (a.rng_states) subarg_prove_draw(c);
  if (c.sm) same_perm_prove_steps(c);
  if (c.gp) gprod_prove_steps(c);
  core_prove_blinders(c);
  if (c.gp) gprod_prove_rdu(c);
  core_prove_steps(c);
  if (c.L) loop_rounds_resident(c.lp, c.pl);
  subarg_prove_download(c);
  call.finish();
  subarg_prove_write(c);
}

// ------------------------------------------------------------------ the verifiers
struct SubargVerifyArgs {
  SubargDepth depth;
  size_t count, n;   // n = ell + nb above the core
  // every depth.  rand: the caller's factors per item, the same-permutation check's ahead of the core's
  const uint8_t *proofs, *rand;
  uint8_t *transcripts, *challenges;
  int* verdicts;
  // the core alone.  fam: G resp. G | T | U; stmt: crs_H | C | D resp. A | Z_t | Z_u; z, vec_u: IPA
  const uint8_t *fam[3] = {}, *stmt[3] = {}, *z = nullptr, *vec_u = nullptr;
  // grand product and same permutation
  size_t ell = 0, nb = 0;
  const uint8_t *G = nullptr, *H = nullptr, *crs_U = nullptr, *g_sum = nullptr, *h_sum = nullptr;
  // grand product alone (same permutation: B is the proof's first point, the result is made on the device)
  const uint8_t *B = nullptr, *result = nullptr;
  // same permutation
  const uint8_t *A = nullptr, *M = nullptr, *vec_a = nullptr;
};

// One verifier call, as SubargProveCall is one prover call
struct SubargVerifyCall {
  const SubargVerifyArgs& a;
  const bool ipa, gp, sm;
  const size_t count, n, ell, nb;
  SamePermCheckPlan spl;            // (sm: the regions of the same-permutation steps behind those of the grand-product steps and the three further points of every row)
  GprodCheckPlan& gpl = spl.gp;     // (gp: the regions of the grand-product steps behind those of the inner-product check)
  SubargCheckPlan& sp = gpl.sp;
  SubargTotals tot{};               // of the outermost plan in use
  size_t gp_byte = 0, gp_chal = 0;  // where the grand-product proof and its challenges start in an item's: behind the same-permutation layer's B resp. challenges
  size_t NP = 0, PP = 0, PB = 0, PBT = 0, NC = 0, NR = 0;   // PBT: the whole proof's bytes; NR: the caller's factors per item
  const uint8_t* proofs = nullptr;  // the caller's, or their canonical copy in canon
  Tier0MsmPlan pl;
  std::vector<MsmTask> tasks;
  std::vector<uint32_t> ix, lens, gix, six;
  std::vector<uint8_t> canon, h_states, h_bad, h_gbad, h_sbad;
  std::vector<size_t> point_bytes;
  std::vector<Fr> h_chal, h_gchal, h_schal;
  std::vector<Jac> h_res;
  std::vector<SmulTask> stasks;
  // the tier-0 buffers of the call, once subarg_verify_reserve has sized them
  Aff *rows = nullptr, *g_aff = nullptr;   // the items' rows | the grand-product layer's dense points
  Fr* dfr = nullptr;
  uint8_t *db = nullptr, *dst = nullptr, *d_bad = nullptr;   // dst: the decoder's verdicts [count][PP] | the items' flags [count] | the layers'
  Jac *din = nullptr, *res = nullptr;
  uint32_t* dix = nullptr;
  uint64_t* dstate = nullptr;

  explicit SubargVerifyCall(const SubargVerifyArgs& args);
  void check() const;
  void point_offsets();
};

SubargVerifyCall::SubargVerifyCall(const SubargVerifyArgs& args)
    : a(args), ipa(args.depth != SubargDepth::SameMsm), gp(args.depth == SubargDepth::Gprod || args.depth == SubargDepth::SamePerm), sm(args.depth == SubargDepth::SamePerm),
      count(args.count), n(args.n), ell(args.ell), nb(args.nb) {
  switch (sm   ? same_perm_check_plan(count, ell, nb, spl)
          : gp ? gprod_check_plan(count, ell, nb, gpl)
               : subarg_check_plan(ipa, count, n, sp)) {
    case SUBARG_NOT_POW2: throw std::invalid_argument("the sub-argument verifiers take n = 2^L elements per item, L >= 0");
    case SUBARG_TOO_LARGE: throw ArgError(ipa ? "cpx_ipa_verify: at most 65536 items and count (n + 4 L + 5) <= 2^24 points"
                                              : "cpx_same_msm_verify: at most 65536 items and count (3 n + 6 L + 6) <= 2^24 points");
    default: break;
  }
  tot = sm ? spl.totals() : gp ? gpl.totals() : sp.totals();
  if (gp) {
    const SubargTotals g = gpl.totals();
    gp_byte = tot.lead_bytes - g.lead_bytes;
    gp_chal = tot.lead_challenges - g.lead_challenges;
  }
  NP = sp.points(), PP = sp.proof_points(), PB = sp.proof_bytes(), PBT = tot.lead_bytes + PB, NC = sp.challenges();
  NR = sm ? (size_t)spl.checks() : (size_t)sp.checks();
}
// the random factors, the scalars of the outermost layer, the transcript states
void SubargVerifyCall::check() const {
  for (size_t i = 0; i < count * NR; i++)
    if (!host::is_valid_factor(a.rand + 32 * i)) throw ArgError("the random factors of a sub-argument check must be non-zero reduced field elements");
  if (sm) {
    for (size_t i = 0; i < count * ell; i++)
      if (!fr_wire_reduced(a.vec_a + i * sizeof(Fr))) throw ArgError("a scalar of vec_a of cpx_same_perm_verify is not reduced");
  } else if (gp) {
    for (size_t i = 0; i < count; i++)
      if (!fr_wire_reduced(a.result + i * sizeof(Fr))) throw ArgError("a scalar gprod_result of cpx_gprod_verify is not reduced");
  } else if (ipa) {
    for (size_t i = 0; i < count; i++)
      if (!fr_wire_reduced(a.z + i * sizeof(Fr))) throw ArgError("a scalar z of cpx_ipa_verify is not reduced");
    for (size_t i = 0; i < count * n; i++)
      if (!fr_wire_reduced(a.vec_u + i * sizeof(Fr))) throw ArgError("a scalar of vec_u is not reduced");
  }
  for (size_t i = 0; i < count; i++)
    if (!transcript_state_valid(a.transcripts + i * kTranscriptBytes)) throw ArgError("a transcript state with pos > 165 or pos_begin > 166");
}
// where a proof's points are, for canonical_infinities: the inner proof's shifted by the lead, then C, then B.
// The grand product's proof is C, r_p, then the InnerProductProof's bytes (grand_product_argument.rs:248-253)
// ... and the same-permutation proof is B, then the grand product's (same_permutation_argument.rs:173-177)
void SubargVerifyCall::point_offsets() {
  point_bytes.resize(PP);
  for (size_t s = 0; s < PP; s++) point_bytes[s] = tot.lead_bytes + sp.point_byte(s);
  if (gp) point_bytes.push_back(gp_byte);
  if (sm) point_bytes.push_back(0);
}

// The stand-alone sub-argument verifiers (include/cpx.h cpx_ipa_verify, cpx_same_msm_verify): InnerProductProof::verify
// (inner_product_argument.rs:202-326) / SameMultiscalarProof::verify (same_multiscalar_argument.rs:153-261) for `count` independent items,
// each against an MsmAccumulator of its own, flattened by subarg_check_plan.hpp into one MSM per item.  One upload; k_decompress with
// status over every proof point of the call, k_finalize over the statement points (their affine forms into the items' rows, their encodings
// for the transcript), for SameMSM k_compress over T | U, k_subarg_scalars (subarg.hip), the MSM chain with one task per item; one
// download of the sums, flags, states and challenges; one synchronisation.  The launches do not depend on count.  The outputs are written
// when the call has succeeded, never before.
void Engine::ipa_verify(size_t count, size_t n, const uint8_t* G, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D, const uint8_t* z, const uint8_t* vec_u,
                        const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  SubargVerifyArgs a{SubargDepth::Ipa, count, n, proofs, rand, transcripts, challenges, verdicts};
  a.fam[0] = G, a.stmt[0] = crs_H, a.stmt[1] = C, a.stmt[2] = D, a.z = z, a.vec_u = vec_u;
  subarg_verify(a);
}
void Engine::same_msm_verify(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t, const uint8_t* Z_u,
                             const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  SubargVerifyArgs a{SubargDepth::SameMsm, count, n, proofs, rand, transcripts, challenges, verdicts};
  a.fam[0] = G, a.fam[1] = T, a.fam[2] = U, a.stmt[0] = A, a.stmt[1] = Z_t, a.stmt[2] = Z_u;
  subarg_verify(a);
}
// The grand-product verifier (include/cpx.h cpx_gprod_verify): GrandProductProof::verify (grand_product_argument.rs:180-246) for `count`
// independent items.  It is the inner-product check on G | H, crs_U, the proof's C and D = B - beta^-1 crs_G_sum + alpha crs_H_sum, with the
// steps that make z, vec_u and D on the device ahead of it: k_decompress over C into the items' rows, k_finalize over crs_U (into the rows)
// and B (its encoding for step 1), k_gprod_verify_steps (gprod.hip), two k_smul launches for D and k_compress for its encoding, which
// ipa_step1 hashes — so D is formed, and once it is, it takes the IPA's own weight in the row.  A wrong crs_G_sum or crs_H_sum gives
// another D and CPX_ERR_VERIFY.
void Engine::gprod_verify(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                          const uint8_t* crs_H_sum, const uint8_t* B, const uint8_t* gprod_result, const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts,
                          uint8_t* challenges, int* verdicts) {
  if (!count) return;
  if (!ell) throw ArgError("cpx_gprod_verify: ell = 0 (the reference's prover cannot make such a proof: its ell - 1 underflows)");
  if (ell + n_blinders < ell) throw ArgError("cpx_gprod_verify: ell + n_blinders overflows");
  SubargVerifyArgs a{SubargDepth::Gprod, count, ell + n_blinders, proofs, rand, transcripts, challenges, verdicts};
  a.ell = ell, a.nb = n_blinders, a.G = G, a.H = H, a.crs_U = crs_U, a.g_sum = crs_G_sum, a.h_sum = crs_H_sum, a.B = B, a.result = gprod_result;
  subarg_verify(a);
}
// The same-permutation verifier (include/cpx.h cpx_same_perm_verify): SamePermutationProof::verify (same_permutation_argument.rs:112-171) for
// `count` independent items.  It is gprod_verify above with B taken from the proof (k_decompress, with a verdict), k_finalize over A | M into
// three further slots of every row, k_same_perm_verify_step ahead of k_gprod_verify_steps and k_same_perm_weights behind k_subarg_scalars
// (same_perm.hip): the relation of :149 joins the item's one MSM with the first of the item's three factors.
void Engine::same_perm_verify(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                              const uint8_t* crs_H_sum, const uint8_t* A, const uint8_t* M, const uint8_t* vec_a, const uint8_t* proofs, const uint8_t* rand,
                              uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  if (!count) return;
  if (!ell) throw ArgError("cpx_same_perm_verify: ell = 0 (the reference's prover cannot make such a proof: its ell - 1 underflows)");
  if (ell + n_blinders < ell) throw ArgError("cpx_same_perm_verify: ell + n_blinders overflows");
  SubargVerifyArgs a{SubargDepth::SamePerm, count, ell + n_blinders, proofs, rand, transcripts, challenges, verdicts};
  a.ell = ell, a.nb = n_blinders, a.G = G, a.H = H, a.crs_U = crs_U, a.g_sum = crs_G_sum, a.h_sum = crs_H_sum, a.A = A, a.M = M, a.vec_a = vec_a;
  subarg_verify(a);
}

// every buffer of the call from the totals of the outermost plan; then the pointers
void Engine::subarg_verify_reserve(SubargVerifyCall& c) {
  const SubargTotals& t = c.tot;
  c.pl.slices = msm_tblw_slices(opt_, (int)c.count, 2, (int)c.pl.max_n);
  t0_.a0.ensure(c.count * c.NP);
  t0_.fr.ensure(t.fr);
  t0_.bytes.ensure(t.bytes);
  t0_.status.ensure(t.flags);
  t0_.jin.ensure(t.jac);
  t0_.res.ensure(t.res);
  t0_.lidx.ensure(t.ix);
  t0_.lstate.ensure(c.count * kTranscriptWords);
  if (c.gp) {   // the dense points and the two tasks that form D
    t0_.a1.ensure(t.aff);
    t0_.stask.ensure(2);
  }
  msm_chain_reserve(c.pl);
  c.rows = t0_.a0.p, c.g_aff = t0_.a1.p, c.dfr = t0_.fr.p, c.db = t0_.bytes.p, c.dst = t0_.status.p, c.din = t0_.jin.p, c.res = t0_.res.p;
  c.dix = t0_.lidx.p, c.dstate = t0_.lstate.p;
  c.d_bad = c.dst + c.sp.st_bad();
}

// ---- the upload: bases and statement points into their places, proofs, scalars, index words, states
// G | H into the items' rows; crs_U (din: crs_U [count] | B [count])
void Engine::gprod_verify_upload_bases(SubargVerifyCall& c) {
  const size_t count = c.count, ell = c.ell, nb = c.nb, NP = c.NP;
  CPX_HIP(hipMemcpy2DAsync(c.rows, NP * sizeof(Aff), c.a.G, ell * sizeof(Aff), ell * sizeof(Aff), count, hipMemcpyHostToDevice, stream_));
  if (nb) CPX_HIP(hipMemcpy2DAsync(c.rows + ell, NP * sizeof(Aff), c.a.H, nb * sizeof(Aff), nb * sizeof(Aff), count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.din, c.a.crs_U, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
}
// B is the proof's first point (into the grand-product layer's by_B), gprod_result is made on the device; A | M, vec_a, the first factor of
// every item, the row slots of A and M
void Engine::same_perm_verify_upload(SubargVerifyCall& c) {
  const SamePermCheckPlan& spl = c.spl;
  const size_t count = c.count;
  CPX_HIP(hipMemcpy2DAsync(c.db + c.gpl.by_B(), 48, c.proofs, c.PBT, 48, count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.din + spl.jac_A(), c.a.A, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.din + spl.jac_A() + count, c.a.M, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dfr + spl.fr_a(), c.a.vec_a, count * c.ell * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(c.dfr + spl.fr_a0(), sizeof(Fr), c.a.rand, c.NR * sizeof(Fr), sizeof(Fr), count, hipMemcpyHostToDevice, stream_));
  spl.fill_idx(c.six);
  CPX_HIP(hipMemcpyAsync(c.dix + spl.ix_AM_dst(), c.six.data(), c.six.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
}
// B and gprod_result unless the same-permutation layer has them; the sums; the proofs in two parts: the inner-product proofs where the
// core reads them, the heads C | r_p; the layer's index words
void Engine::gprod_verify_upload(SubargVerifyCall& c) {
  const GprodCheckPlan& gpl = c.gpl;
  const size_t count = c.count, glead = GprodCheckPlan::kHead;
  if (!c.sm) {
    CPX_HIP(hipMemcpyAsync(c.din + count, c.a.B, count * sizeof(Jac), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(c.dfr + gpl.fr_result(), c.a.result, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  CPX_HIP(hipMemcpyAsync(c.g_aff + gpl.aff_g_sum(), c.a.g_sum, count * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.g_aff + gpl.aff_h_sum(), c.a.h_sum, count * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(c.db + c.sp.by_proofs(), c.PB, c.proofs + c.tot.lead_bytes, c.PBT, c.PB, count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(c.db + gpl.by_heads(), glead, c.proofs + c.gp_byte, c.PBT, glead, count, hipMemcpyHostToDevice, stream_));
  gpl.fill_idx(c.gix);
  CPX_HIP(hipMemcpyAsync(c.dix + gpl.ix_C_src(), c.gix.data(), c.gix.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
}
// the core alone: the caller's bases, statement points and proofs; IPA: z and vec_u
void Engine::core_verify_upload(SubargVerifyCall& c) {
  const SubargCheckPlan& sp = c.sp;
  const size_t count = c.count, n = c.n, K = SubargCheckPlan::kStatement;
  for (int f = 0; f < sp.families(); f++)
    CPX_HIP(hipMemcpy2DAsync(c.rows + sp.base_off(f), c.NP * sizeof(Aff), c.a.fam[f], n * sizeof(Aff), n * sizeof(Aff), count, hipMemcpyHostToDevice, stream_));
  for (size_t k = 0; k < K; k++)
    CPX_HIP(hipMemcpy2DAsync(c.din + k, K * sizeof(Jac), c.a.stmt[k], sizeof(Jac), sizeof(Jac), count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.db + sp.by_proofs(), c.proofs, count * c.PB, hipMemcpyHostToDevice, stream_));
  if (c.ipa) {
    CPX_HIP(hipMemcpyAsync(c.dfr + sp.fr_z(), c.a.z, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(c.dfr + sp.fr_u(), c.a.vec_u, count * n * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
}
// what the core uploads at every depth: its factors (behind the same-permutation check's first), its index words, the states
void Engine::subarg_verify_upload_lists(SubargVerifyCall& c) {
  const SubargCheckPlan& sp = c.sp;
  const size_t count = c.count, checks = (size_t)sp.checks();
  if (c.sm) CPX_HIP(hipMemcpy2DAsync(c.dfr + sp.fr_rand(), checks * sizeof(Fr), c.a.rand + sizeof(Fr), c.NR * sizeof(Fr), checks * sizeof(Fr), count, hipMemcpyHostToDevice, stream_));
  else CPX_HIP(hipMemcpyAsync(c.dfr + sp.fr_rand(), c.a.rand, count * checks * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  sp.fill_idx(c.ix);
  CPX_HIP(hipMemcpyAsync(c.dix, c.ix.data(), c.ix.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(c.dstate, c.a.transcripts, count * kTranscriptBytes, hipMemcpyHostToDevice, stream_));
}

// ---- the device work
// every point of the inner proofs into the rows, with a verdict
void Engine::core_verify_decode(SubargVerifyCall& c) {
  tick("k_decompress", 0, (double)(c.count * c.PP));
  launch_decompress(opt_, c.db, (int)(c.count * c.PP), c.rows, c.dix + c.sp.ix_dst(), c.dst, 1, stream_, c.dix + c.sp.ix_src());
  tock();
}
// the core alone: the caller's statement points into the rows, their encodings for the transcript
void Engine::core_verify_statement(SubargVerifyCall& c) {
  const size_t K = SubargCheckPlan::kStatement;
  tick("k_finalize", 0, (double)(c.count * K));
  launch_finalize(c.din, (int)(c.count * K), c.rows, c.dix + c.sp.ix_statement(), c.db + c.sp.by_statement(), stream_);
  tock();
}
// same_permutation_argument.rs:149 joins the item's one MSM, once the core has written the row of weights
void Engine::same_perm_verify_weights(SubargVerifyCall& c) {
  tick("k_same_perm_weights", 0, (double)c.count, true);
  launch_same_perm_weights(SamePermVerifyDev{c.spl, c.dfr, c.db, c.dstate}, stream_);
  tock();
}
// C into the rows' C slots, crs_U into the rows, B's affine form and encoding unless the same-permutation layer decodes it
void Engine::gprod_verify_decode(SubargVerifyCall& c) {
  const GprodCheckPlan& gpl = c.gpl;
  const size_t count = c.count;
  tick("k_decompress", 0, (double)count);
  launch_decompress(opt_, c.db + gpl.by_heads(), (int)count, c.rows, c.dix + gpl.ix_C_dst(), c.dst + gpl.st_C(), 1, stream_, c.dix + gpl.ix_C_src());   // C into the rows' C slots
  tock();
  tick("k_finalize", 0, 2.0 * count);
  launch_finalize(c.din, (int)count, c.rows, c.dix + gpl.ix_U_dst(), nullptr, stream_);                               // crs_U into the rows
  if (!c.sm) launch_finalize(c.din + count, (int)count, c.g_aff + gpl.aff_B(), nullptr, c.db + gpl.by_B(), stream_);   // B: affine and encoding
  tock();
}
// B from its encoding, with a verdict; A | M into the rows behind the statement slots, their encodings for step 1; the step.  Hands to the
// grand-product layer: B's affine form in its aff_B, gprod_result in its Fr region
void Engine::same_perm_verify_steps(SubargVerifyCall& c) {
  const SamePermCheckPlan& spl = c.spl;
  const size_t count = c.count;
  tick("k_decompress", 0, (double)count);
  launch_decompress(opt_, c.db + c.gpl.by_B(), (int)count, c.g_aff + c.gpl.aff_B(), nullptr, c.dst + spl.st_B(), 1, stream_);
  tock();
  tick("k_finalize", 0, 2.0 * count);
  launch_finalize(c.din + spl.jac_A(), (int)(2 * count), c.rows, c.dix + spl.ix_AM_dst(), c.db + spl.by_A(), stream_);
  tock();
  CPX_HIP(hipMemcpy2DAsync(c.rows + spl.row_B(), c.NP * sizeof(Aff), c.g_aff + c.gpl.aff_B(), sizeof(Aff), sizeof(Aff), count, hipMemcpyDeviceToDevice, stream_));
  tick("k_same_perm_verify_step", 0, (double)count, true);
  launch_same_perm_verify_step(SamePermVerifyDev{spl, c.dfr, c.db, c.dstate}, stream_);
  tock();
}
// steps 1 and 2 with z and vec_u; D, its encoding and its place in the rows.  Hands to the core: z and vec_u in its Fr regions, the
// encodings of C and D among its statement encodings, C, D and crs_U in its rows
void Engine::gprod_verify_steps(SubargVerifyCall& c) {
  const GprodCheckPlan& gpl = c.gpl;
  const SubargCheckPlan& sp = c.sp;
  const size_t count = c.count, glead = GprodCheckPlan::kHead, K = SubargCheckPlan::kStatement;
  Aff* const g_aff = c.g_aff;
  uint8_t *const g_heads = c.db + gpl.by_heads(), *const g_denc = c.db + gpl.by_D();
  tick("k_gprod_verify_steps", 0, (double)count, true);
  launch_gprod_verify_steps(GprodVerifyDev{gpl, c.dfr, c.db, c.dst, c.dstate}, stream_);
  tock();
  // D = (B - beta^-1 crs_G_sum) + alpha crs_H_sum (:223), one element per item in each launch; then its encoding and its place in the rows
  c.stasks = {SmulTask{g_aff + gpl.aff_B(), g_aff + gpl.aff_g_sum(), g_aff + gpl.aff_partial(), c.dfr + gpl.fr_neg_beta_inv(), 1, smul_flag()},
              SmulTask{g_aff + gpl.aff_partial(), g_aff + gpl.aff_h_sum(), g_aff + gpl.aff_D(), c.dfr + gpl.fr_alpha(), 1, smul_flag()}};
  CPX_HIP(hipMemcpyAsync(t0_.stask.p, c.stasks.data(), 2 * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
  smul_tasks(t0_.stask.p, 1, count, (double)count);
  smul_tasks(t0_.stask.p + 1, 1, count, (double)count);
  tick("k_compress", 0, (double)count, true);
  launch_compress(g_aff + gpl.aff_D(), (int)count, (int)count, 1, g_denc, stream_);
  tock();
  uint8_t* const d_stmt_enc = c.db + sp.by_statement();   // [count][3][48]: (crs_U: not hashed) | C | D
  CPX_HIP(hipMemcpy2DAsync(d_stmt_enc + 48, K * 48, g_heads, glead, 48, count, hipMemcpyDeviceToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(d_stmt_enc + 96, K * 48, g_denc, 48, 48, count, hipMemcpyDeviceToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(c.rows + sp.statement_off() + 2, c.NP * sizeof(Aff), g_aff + gpl.aff_D(), sizeof(Aff), sizeof(Aff), count, hipMemcpyDeviceToDevice, stream_));
}
// SameMSM: the encodings of T | U; the transcript and scalar step: flags, states, challenges, the rows of weights
void Engine::core_verify_scalars(SubargVerifyCall& c) {
  const SubargCheckPlan& sp = c.sp;
  const size_t count = c.count, n = c.n, NP = c.NP;
  if (!c.ipa) {
    tick("k_compress", 0, 2.0 * count * n, true);
    for (size_t i = 0; i < count; i += 65535) {   // (a row per item in the grid's second dimension: 65535 at most; 2^16 items take two launches)
      const size_t rows_now = std::min<size_t>(count - i, 65535);
      launch_compress(c.rows + i * NP + sp.base_off(1), (int)(2 * n), (int)NP, (int)rows_now, c.db + sp.by_tu() + i * 2 * n * 48, stream_);
    }
    tock();
  }
  tick("k_subarg_scalars", 0, (double)count, true);
  launch_subarg_scalars(SubargDev{sp, c.dfr, c.db, c.dst, c.d_bad, c.dstate}, stream_);
  tock();
}

// ---- the one download, into host memory of the call: the core's, the grand-product layer's, the same-permutation layer's
void Engine::subarg_verify_download(SubargVerifyCall& c) {
  const size_t count = c.count, NC = c.NC;
  c.h_res.resize(count);
  c.h_bad.resize(count);
  c.h_states.resize(count * kTranscriptBytes);
  c.h_chal.resize(count * NC);
  CPX_HIP(hipMemcpyAsync(c.h_res.data(), c.res, count * sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_bad.data(), c.d_bad, count, hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_states.data(), c.dstate, c.h_states.size(), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(c.h_chal.data(), c.dfr + c.sp.fr_challenges(), count * NC * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  if (c.gp) {
    c.h_gbad.resize(count);
    c.h_gchal.resize(2 * count);
    CPX_HIP(hipMemcpyAsync(c.h_gbad.data(), c.dst + c.gpl.st_bad(), count, hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(c.h_gchal.data(), c.dfr + c.gpl.fr_chal(), 2 * count * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  }
  if (c.sm) {
    c.h_sbad.resize(count);
    c.h_schal.resize(2 * count);
    CPX_HIP(hipMemcpyAsync(c.h_sbad.data(), c.dst + c.spl.st_B(), count, hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(c.h_schal.data(), c.dfr + c.spl.fr_chal(), 2 * count * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  }
}

// ---- the write-out.  The core alone: states and challenges whole.  With the layers: item by item, and an item that does not deserialise
// keeps the state it came with (the device had advanced it by steps 1 and 2) and gets zero challenges
static void subarg_verify_write(const SubargVerifyCall& c) {
  const SubargVerifyArgs& a = c.a;
  const size_t count = c.count, NC = c.NC, NCT = c.tot.lead_challenges + NC;
  if (!c.gp) {
    memcpy(a.transcripts, c.h_states.data(), c.h_states.size());
    if (a.challenges) memcpy(a.challenges, c.h_chal.data(), count * NC * sizeof(Fr));
    for (size_t i = 0; i < count; i++) a.verdicts[i] = c.h_bad[i] ? CPX_ERR_DESERIALIZE : c.h_res[i].is_identity() ? CPX_OK : CPX_ERR_VERIFY;
    return;
  }
  for (size_t i = 0; i < count; i++) {
    const bool bad = c.h_bad[i] || c.h_gbad[i] || (c.sm && c.h_sbad[i]);
    uint8_t* const ch = a.challenges ? a.challenges + i * NCT * sizeof(Fr) : nullptr;
    if (!bad) memcpy(a.transcripts + i * kTranscriptBytes, c.h_states.data() + i * kTranscriptBytes, kTranscriptBytes);
    if (ch && bad) memset(ch, 0, NCT * sizeof(Fr));
    if (ch && !bad) {   // the same-permutation challenges ahead of the grand product's ahead of the core's
      if (c.sm) memcpy(ch, c.h_schal.data() + 2 * i, 2 * sizeof(Fr));
      memcpy(ch + c.gp_chal * sizeof(Fr), c.h_gchal.data() + 2 * i, 2 * sizeof(Fr));
      memcpy(ch + c.tot.lead_challenges * sizeof(Fr), c.h_chal.data() + i * NC, NC * sizeof(Fr));
    }
    a.verdicts[i] = bad ? CPX_ERR_DESERIALIZE : c.h_res[i].is_identity() ? CPX_OK : CPX_ERR_VERIFY;
  }
}

// The one driver of the four verifiers: the phases of subarg_prove with the device work in place of the steps and the rounds, and the
// same exception to the order of the layers — the grand product's bases go up ahead of the same-permutation layer's inputs.
void Engine::subarg_verify(const SubargVerifyArgs& a) {
  if (!a.count) return;
  SubargVerifyCall c(a);   // the plans and their totals; above the scope with everything an enqueued copy reads or writes
  c.check();
  if (!c.sp.msm(c.pl, c.lens)) throw ArgError("the items exceed the limits of cpx_g1_msm_many");
  c.point_offsets();
  c.proofs = canonical_infinities(a.proofs, c.count * c.PBT, c.count, c.PBT, c.point_bytes, c.canon);
  CallScope call(this);
  subarg_verify_reserve(c);
  if (c.gp) gprod_verify_upload_bases(c);
  if (c.sm) same_perm_verify_upload(c);
  if (c.gp) gprod_verify_upload(c);
  else core_verify_upload(c);
  subarg_verify_upload_lists(c);
  core_verify_decode(c);
  if (c.gp) gprod_verify_decode(c);
  if (c.sm) same_perm_verify_steps(c);
  if (c.gp) gprod_verify_steps(c);
  else core_verify_statement(c);
  core_verify_scalars(c);
  if (c.sm) same_perm_verify_weights(c);
  msm_chain(c.pl, c.lens.data(), c.rows, c.dfr + c.sp.fr_weights(), c.res, c.tasks);   // one task per item: its row against its weights
  subarg_verify_download(c);
  call.finish();
  subarg_verify_write(c);
}

}  // namespace cpx
