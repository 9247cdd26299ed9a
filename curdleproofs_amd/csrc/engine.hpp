// Host engine of the MI355X Curdleproofs core — product code.
//
// One `Engine` = one HIP device + one stream + the device-resident CRS and batch buffers.  A batch of
// B independent shuffle instances (same ell) advances in lock-step: every protocol phase is ONE set of
// kernel launches covering all B proofs (the batch is a grid dimension), bracketed by the host-side
// Fiat-Shamir step.  Mirrors /root/reference/src/curdleproofs.rs:59-298 and the sub-arguments it calls.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <chrono>
#include <map>
#include <mutex>
#include <thread>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/cpx.h"   // public error codes
#include "host_math.hpp"
#include "host_threads.hpp"
#include "kernels.h"
#include "check_plan.hpp"
#include "locate_plan.hpp"
#include "tracker_check_plan.hpp"
#include "protocol.h"
#include "prove_reqs.hpp"
#include "rng.hpp"
#include "rng_g1_plan.hpp"
#include "shuffle_plan.hpp"
#include "tbl_plan.hpp"
#include "tier0_plan.hpp"
#include "loop_plan.hpp"
#include "subarg_check_plan.hpp"
#include "transcript_state.hpp"

namespace cpx {

struct HipError : std::runtime_error {
  hipError_t code;
  HipError(hipError_t c, const char* what) : std::runtime_error(what), code(c) {}
};
struct SubargProveArgs;   // (engine_subarg.cpp)
struct SubargProveCall;
struct SubargVerifyArgs;
struct SubargVerifyCall;
// a caller-supplied value is out of range (-> CPX_ERR_ARG)
struct ArgError : std::runtime_error {
  explicit ArgError(const char* what) : std::runtime_error(what) {}
};
#define CPX_HIP(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) throw ::cpx::HipError(_e, (std::string(#expr) + ": " + hipGetErrorString(_e)).c_str()); \
  } while (0)

// Page-locked host memory comes from the (uninstrumented) HIP runtime, which hands a freed range out again: ThreadSanitizer cannot see the
// runtime's lock between one owner's hipHostFree and the next owner's hipHostMalloc of the same addresses — one context's staging buffer
// released, another context's status buffer allocated there — and reports the two owners' accesses as a race (tests/test_sanitizers.py, the
// engine under TSan on the GPU box).  The free / allocate pair is therefore announced to the tool as a release / acquire on one
// process-wide object; a no-op in every other build.
#if defined(__has_feature)
#if __has_feature(thread_sanitizer)
#define CPX_TSAN 1
#endif
#endif
#if defined(CPX_TSAN)
extern "C" void AnnotateHappensBefore(const char* file, int line, const volatile void* addr);
extern "C" void AnnotateHappensAfter(const char* file, int line, const volatile void* addr);
inline char g_pinned_memory_sync = 0;
#define CPX_HOST_MEMORY_RELEASE() AnnotateHappensBefore(__FILE__, __LINE__, &::cpx::g_pinned_memory_sync)
#define CPX_HOST_MEMORY_ACQUIRE() AnnotateHappensAfter(__FILE__, __LINE__, &::cpx::g_pinned_memory_sync)
#else
#define CPX_HOST_MEMORY_RELEASE() ((void)0)
#define CPX_HOST_MEMORY_ACQUIRE() ((void)0)
#endif

template <class T> struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  size_t bytes() const { return cap * sizeof(T); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) CPX_HIP(hipFree(p));
    p = nullptr;
    CPX_HIP(hipMalloc(&p, n * sizeof(T)));
    cap = n;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};
template <class F, class... B> void each_buf(F&& f, B&... b) {   // f on every buffer of a list, whatever their element types
  (f(b), ...);
}
template <class T> struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    CPX_HOST_MEMORY_RELEASE();
    if (p) CPX_HIP(hipHostFree(p));
    p = nullptr;
    CPX_HIP(hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault));
    CPX_HOST_MEMORY_ACQUIRE();
    cap = n;
  }
  ~PinBuf() {
    CPX_HOST_MEMORY_RELEASE();
    if (p) (void)hipHostFree(p);
  }
};

struct KernelStat {
  uint64_t launches = 0;
  double ms = 0;
  double alg_bytes = 0;   // algorithmic bytes moved (SURVEY §8d accounting)
  double units = 0;       // MSM points / scalar-mul elements / points processed
};


// kernel names as rocprofv3 reports the template instantiations (statistics keys)
inline const char* fix_kernel_name(int bits, int wpw) {
  if (bits == 19) return "k_msm_fix<19, 7>";
  if (bits == 16) return wpw == 16 ? "k_msm_fix<16, 16>" : wpw == 8 ? "k_msm_fix<16, 8>" : wpw == 4 ? "k_msm_fix<16, 4>" : "k_msm_fix<16, 2>";
  return wpw == 16 ? "k_msm_fix<8, 16>" : "k_msm_fix<8, 8>";
}
inline const char* tblw_kernel_name(int wpw) {
  switch (wpw) {
    case 32: return "k_msm_tblw<32, false>";
    case 16: return "k_msm_tblw<16, false>";
    case 8: return "k_msm_tblw<8, false>";
    case 4: return "k_msm_tblw<4, false>";
    default: return "k_msm_tblw<2, false>";
  }
}


void trace_scalar(const char* name, const Fr& x);   // CPX_TRACE=1 debugging aid (engine_device.cpp)

// Scratch of one stream's MSM launches: the raw lane accumulators of k_msm_tblw / k_msm_fix and the partial-sum slot of every set
// (kernels.h), the group sums between the two reduction launches, and the partial sums the reduction leaves.  Together with its stream
// it says where a phase runs.
struct MsmScratch {
  DevBuf<uint32_t> raw, rawslot;
  DevBuf<TJac> mid, part;
  void ensure(size_t nsets, size_t nparts) {
    nsets = std::max<size_t>(nsets, 1);
    raw.ensure(nsets * raw_set_words());
    rawslot.ensure(nsets);
    mid.ensure(nsets * reduce_mid_per_set());
    part.ensure(std::max<size_t>(nparts, 1));
  }
};

class Engine {
 public:
  explicit Engine(int device);
  ~Engine();

  // crs.rs:37-58 CurdleproofsCrs::from_points: ell + 7 affine points (G[ell] | H[4] | H | G_t | G_u)
  void set_crs(size_t ell, const uint8_t* points);
  size_t ell() const { return ell_; }
  size_t n() const { return n_; }
  size_t log2n() const { return L_; }
  size_t proof_size() const { return ProofLayout(L_).size(); }
  void crs_sums(uint8_t* g_sum, uint8_t* h_sum) const;

  // ---- tier 0: the reference's util::msm & friends on caller buffers ----
  void msm(const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out_jac);                  // util.rs:19-22
  void msm_jac(const uint8_t* bases_jac, const uint8_t* scalars, size_t n, uint8_t* out_jac);          // util.rs:25-29
  void fold(uint8_t* PL, const uint8_t* PR, const uint8_t* gamma, size_t half);                        // IPA / SameMSM folds
  void scale(const uint8_t* P, const uint8_t* scalars, size_t scalar_stride, size_t n, uint8_t* out);  // G' rescale / k*R
  // the calls of one log round, many per call (tier0_plan.hpp): ONE upload, kernel chain, download and stream synchronisation each
  void msm_many(size_t count, const uint32_t* lens, const uint8_t* bases, const uint8_t* scalars, uint8_t* out_jac, uint8_t* out_comp);   // the cross terms: inner_product_argument.rs:158-161, same_multiscalar_argument.rs:107-112
  void fold_many(size_t families, size_t half, uint8_t* PL, const uint8_t* PR, const uint8_t* gammas);                                      // the basis folds: inner_product_argument.rs:177-178, same_multiscalar_argument.rs:128-130
  // the log-round loops themselves, `count` independent items per call (loop_plan.hpp, loop.hip; include/cpx.h cpx_ipa_rounds /
  // cpx_same_msm_rounds): states in/out, every round's cross terms, the finals and the challenges; no CRS, the batch is left alone
  void ipa_rounds(size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* H, const uint8_t* vec_c, const uint8_t* vec_d, uint8_t* transcripts,
                  uint8_t* rounds_comp, uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas);                                              // inner_product_argument.rs:150-186
  void same_msm_rounds(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* vec_x, uint8_t* transcripts, uint8_t* rounds_comp,
                       uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas);                                                               // same_multiscalar_argument.rs:99-136
  // the verifiers of the two sub-arguments on the caller's bases, `count` independent items per call, each against an accumulator of its own
  // (subarg_check_plan.hpp, subarg.hip; include/cpx.h cpx_ipa_verify / cpx_same_msm_verify): states in/out, per-item verdicts; no CRS, the
  // batch is left alone
  void ipa_verify(size_t count, size_t n, const uint8_t* G, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D, const uint8_t* z, const uint8_t* vec_u,
                  const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts);                     // inner_product_argument.rs:202-326
  void same_msm_verify(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t, const uint8_t* Z_u,
                       const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts);                // same_multiscalar_argument.rs:153-261
  // the provers of the two sub-arguments on the caller's bases, `count` independent items per call (subarg_prove_plan.hpp, subarg_prove.hip;
  // include/cpx.h cpx_ipa_prove / cpx_same_msm_prove and their _rng forms): the reference's `serialize` bytes, states in/out, per-item status.
  // Exactly one of rand (the draws) and rng_states (count x 40 bytes, in/out: the draws are made on the device) is non-null; no CRS, the
  // batch is left alone
  void ipa_prove(size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D, const uint8_t* z,
                 const uint8_t* vec_c, const uint8_t* vec_d, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges,
                 int* status);                                                                                                               // inner_product_argument.rs:98-199
  void same_msm_prove(size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t, const uint8_t* Z_u,
                      const uint8_t* vec_x, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges,
                      int* status);                                                                                                          // same_multiscalar_argument.rs:69-150
  // the grand-product prover on the caller's bases likewise (gprod_plan.hpp, gprod.hip; include/cpx.h cpx_gprod_prove and its _rng form):
  // ell factors and n_blinders blinders per item, rand = vec_c_blinders then the inner-product prover's draws
  void gprod_prove(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B, const uint8_t* gprod_result,
                   const uint8_t* vec_b, const uint8_t* vec_b_blinders, const uint8_t* rand, uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs,
                   uint8_t* challenges, int* status);                                                                                        // grand_product_argument.rs:43-166
  void gprod_verify(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                    const uint8_t* crs_H_sum, const uint8_t* B, const uint8_t* gprod_result, const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts,
                    uint8_t* challenges, int* verdicts);                                                                                     // grand_product_argument.rs:180-246
  // the same-permutation prover and verifier on the caller's bases likewise (same_perm_plan.hpp, same_perm.hip; include/cpx.h
  // cpx_same_perm_prove, its _rng form and cpx_same_perm_verify): the layer above the grand-product one, which draws nothing
  void same_perm_prove(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A, const uint8_t* M,
                       const uint8_t* vec_a, const uint32_t* permutation, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders, const uint8_t* rand,
                       uint8_t* rng_states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status);                        // same_permutation_argument.rs:40-99
  void same_perm_verify(size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                        const uint8_t* crs_H_sum, const uint8_t* A, const uint8_t* M, const uint8_t* vec_a, const uint8_t* proofs, const uint8_t* rand,
                        uint8_t* transcripts, uint8_t* challenges, int* verdicts);                                                           // same_permutation_argument.rs:112-171
  void normalize(const uint8_t* jac, size_t n, uint8_t* out_aff, uint8_t* out_comp);                   // normalize_batch (+compress)
  int decompress(const uint8_t* comp, size_t n, uint8_t* out_aff, int check_subgroup, uint8_t* status_out = nullptr);   // whisk.rs:318-320

  // ---- tier 2: batches of whole proofs, instance data resident in HBM ----
  void batch_load(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M);
  // the next batch's instance uploaded beside the running batch (include/cpx.h cpx_batch_load_begin / _end)
  void batch_load_begin(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M);
  void batch_load_end();
  // witnesses + the 3n+9 Fr draws per proof (SURVEY §8b RNG contract); writes batch * proof_size() bytes
  void batch_prove(const uint32_t* permutation, const uint8_t* k, const uint8_t* m_blinders, const uint8_t* rand, uint8_t* proofs_out);
  // proofs: batch * proof_size() bytes; rand: batch * 8 Fr; verdict[i] = CPX_OK / CPX_ERR_VERIFY / CPX_ERR_DESERIALIZE
  bool sum_jac(const uint8_t* points_jac, size_t n, uint8_t* out_jac);   // true iff the sum is the identity
  void batch_verify(const uint8_t* proofs, const uint8_t* rand, int* verdict);
  // BASELINE config 5: all proofs of the batch in one accumulated MSM; 12 random factors per proof; output = this
  // engine's partial sum (Jacobian, standard form) and the number of structurally invalid proofs
  void batch_verify_fused(const uint8_t* proofs, const uint8_t* rand, uint8_t* partial_jac, int* n_invalid);
  // The grouped form of the accumulated check (locate_plan.hpp; include/cpx.h cpx_batch_verify_grouped): 12 factors per proof as for the fused
  // call, one verdict per proof; n_rechecked (nullable) = the proofs that went through the second stage.  All three modes lay out their scalars,
  // gather list and tasks by check_plan.hpp on both paths: verify_core stages them from the host, prepare_device_verifier builds them once per shape
  void batch_verify_grouped(const uint8_t* proofs, const uint8_t* rand, int* verdict, size_t* n_rechecked);
  size_t batch() const { return B_; }

  // ---- Whisk byte-level API (whisk.rs; whisk.cpp) ----
  int whisk_generate_shuffle_proof(const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders, const uint8_t* rand,
                                   uint8_t* post_trackers_out, uint8_t* proof_out);
  int whisk_is_valid_shuffle_proof(const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proof, const uint8_t* rand, int* valid);
  int whisk_generate_tracker_proof(const uint8_t tracker[96], const uint8_t k[32], const uint8_t blinder[32], uint8_t proof_out[128]);
  int whisk_is_valid_tracker_proof(const uint8_t tracker[96], const uint8_t k_commitment[48], const uint8_t proof[128], int* valid);
  // the two tracker-proof functions for `count` independent items per call: a constant number of launches and one stream synchronisation
  // (tracker.hip); status / verdict per item, the loaded batch and the CRS are not touched
  void whisk_generate_tracker_proofs(size_t count, const uint8_t* trackers, const uint8_t* k, const uint8_t* blinders, uint8_t* proofs_out, int* status);
  void whisk_verify_tracker_proofs(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, int* verdict);
  // the same two relations weighted by two caller-drawn factors per item and summed per group: ONE bucket MSM of 1 + 5 G points per group
  // (tracker_check_plan.hpp).  grouped: one verdict per item, the items of a failing group rechecked by the per-item relations; fused: the
  // sum over all items as a 144-byte partial and the number of undecodable items
  void whisk_verify_tracker_proofs_grouped(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                                           size_t* n_rechecked);
  void whisk_verify_tracker_proofs_fused(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand,
                                         uint8_t* partial_jac, int* n_invalid);
  // what those calls consume, `count` per call, as multiples of the generator on its fixed-base table (genmul.hip): out[i] = scalars[i] G, and
  // WhiskTracker::from_k_r / get_k_commitment (whisk.rs:45-55, :370) for (k, r) pairs; either output may be null
  void generator_mul(size_t count, const uint8_t* scalars, uint8_t* out_affine, uint8_t* out_compressed);
  // which key opens which tracker, k_j * r_G_i == k_r_G_i for every pair (find.hip, find_plan.hpp): owner[i] = the smallest such j or CPX_NO_OWNER
  void whisk_find_trackers(size_t n_trackers, const uint8_t* trackers, size_t n_keys, const uint8_t* k, uint32_t* owner, int* status);
  void whisk_trackers_from_k_r(size_t count, const uint8_t* k, const uint8_t* r, uint8_t* trackers_out, uint8_t* k_commitments_out);
  // the shuffle step and the two shuffle-proof functions for `count` independent shuffles per call (shuffle.hip): compressed bytes in, compressed
  // bytes out, nothing returns to the host between the uploads and the batch prover / verifier; the count instances become the loaded batch
  void shuffle_batch(size_t count, const uint8_t* vec_R, const uint8_t* vec_S, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                     uint8_t* vec_T_out, uint8_t* vec_U_out, uint8_t* M_out);
  void whisk_generate_shuffle_proofs(size_t count, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                                     const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status);
  void whisk_verify_shuffle_proofs(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand, int* verdict);
  // ---- the reference's `rng: &mut T` as ChaCha12 states (rng.hpp), the draws made on the device by k_rng_draw (rng.hip; whisk.cpp) ----
  // states: count x 40 bytes, in/out; a call that throws leaves them as they were
  void rng_fr(size_t count, uint8_t* states, size_t n_each, uint8_t* out);
  // G1Projective::rand(rng).into_affine() n_each times per stream (rng_g1.hip); either output may be null.  Needs no CRS, leaves the batch alone
  void rng_g1(size_t count, uint8_t* states, size_t n_each, uint8_t* out_affine, uint8_t* out_compressed);
  // README.md:85-95 per stream at the loaded ell: shuffle of 0..ell, k, vec_R, vec_S; any output may be null, the states advance by the whole set
  void rng_instance_draws(size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* vec_R_out, uint8_t* vec_S_out);
  // crs.rs:61-69 generate_crs(ell) from the caller's stream: ell + 7 draws, then set_crs; points_out (nullable) receives them
  void crs_generate(size_t ell, uint8_t* state, uint8_t* points_out);
  // mul_by_cofactor for n points of E(Fp) (k_clear_cofactor), independent of option scale_any_point
  void clear_cofactor(const uint8_t* points, size_t n, uint8_t* out_affine);
  // the draws of one generate_whisk_shuffle_proof per stream (shuffle, k, 4 blinders, 3n + 9), downloaded; any output may be null.
  // states_after_k (nullable): every stream's state as it stands after the shuffle and k (whisk.rs:150-157 returns Err there)
  void rng_shuffle_draws(size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* blinders_out, uint8_t* rand_out,
                         uint8_t* states_after_k = nullptr);
  void whisk_generate_shuffle_proofs_rng(size_t count, const uint8_t* pre_trackers, uint8_t* states, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status);
  // batch_prove with the 3n + 9 draws of every loaded instance taken from its stream
  void batch_prove_rng(const uint32_t* permutation, const uint8_t* k, const uint8_t* m_blinders, uint8_t* states, uint8_t* proofs_out);
  // ... with 12 factors per item and the grouped check behind it
  void whisk_verify_shuffle_proofs_grouped(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                                           size_t* n_rechecked);
  // ---- the resident candidate tracker list and a run of shuffles against it (run.hip, run_plan.hpp; whisk.cpp) ----
  // decodes the 2n points once (subgroup-checked) and keeps points, status and bytes until the next load or the end of the engine;
  // status (nullable): per candidate the decoder's code of r_G if non-zero, else of k_r_G
  void whisk_candidates_load(size_t n, const uint8_t* trackers, uint8_t* status);
  size_t whisk_candidates_size() const { return cand_.n; }
  void whisk_candidates_read(size_t first, size_t count, uint8_t* trackers_out) const;
  // whisk.rs:106-130 for a run of items whose pre trackers are the candidates at indices[b][0..ell) of the list as it stands after items
  // 0..b-1 were written back; the leading accepted items are written back to the resident list when n_applied is not null (a dry run otherwise)
  void whisk_verify_shuffle_run(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                                size_t* n_applied);
  void whisk_verify_shuffle_run_grouped(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                                        size_t* n_applied, size_t* n_rechecked);

  // ---- measurement ----
  void set_profiling(bool on) { profiling_ = on; }
  void reset_stats() { stats_.clear(); }
  const std::map<std::string, KernelStat>& stats() const { return stats_; }
  double bench_fpmul(int blocks, int iters, int reps);   // returns Fp products per second
  void set_host_threads(int t) {
    host_threads_ = t;
    pool_.reset();
  }
  // per-context tunables (kernels.h `Options`; cpx_ctx_set_option).  fix_bits takes effect at the next set_crs; a change invalidates
  // the cached device plans (their task layouts depend on the kernel selection).
  bool set_option(const char* key, long value);
  // read-only beside the tunables: "fix_bits_effective" = the radix of the fixed-base table in use (set_crs falls back 19 -> 16 -> 8 when
  // free HBM is short; 0 before the first set_crs)
  bool get_option(const char* key, long* value) const {
    if (key && !strcmp(key, "fix_bits_effective")) {
      if (value) *value = crs_tab_ ? fix_bits_ : 0;
      return true;
    }
    // "tbl_segments_effective" = the layout of the per-proof tables the loaded batch proves with (0 before the first batch_load)
    if (key && !strcmp(key, "tbl_segments_effective")) {
      if (value) *value = B_ ? tbl_segments_for(B_) : 0;
      return true;
    }
    // "tier0_scratch_bytes" = the device memory the tier-0 and batched Whisk scratch holds between calls (Tier0, ShuffleBufs below)
    if (key && !strcmp(key, "tier0_scratch_bytes")) {
      size_t sum = 0;
      const auto add = [&](const auto& b) { sum += b.bytes(); };
      Tier0::each(t0_, add);
      ShuffleBufs::each(sh_, add);
      if (value) *value = (long)sum;
      return true;
    }
    // "rng_g1_last_rounds" = the rounds the last G1 draw call took (the most over its chunks of streams; rng_g1_plan.hpp)
    if (key && !strcmp(key, "rng_g1_last_rounds")) {
      if (value) *value = (long)rng_g1_rounds_;
      return true;
    }
    return cpx::get_option(opt_, key, value);
  }
  hipStream_t stream() const { return stream_; }
  void sync() { CPX_HIP(hipStreamSynchronize(stream_)); }

 private:
  struct MsmReq {
    const Aff* bases;
    const uint32_t* idx;
    const host::S* scalars;   // host pointer, n entries
    uint32_t n;
    uint32_t dst;             // index into d_pp_ (Aff units) receiving the affine result
  };
  // second stream + private staging for work that is off the critical path of the phase sequence
  struct SideBufs {
    hipStream_t stream = nullptr;
    hipStream_t hi_stream = nullptr;   // high-priority stream: the transcript prefix of a small batch (its waves are placed before those of the table build)
    hipStream_t lat_stream = nullptr, lat_main = nullptr;   // the host-driven prover's side / main stream: CU-masked (create_masked_stream)
    hipEvent_t lat_ev = nullptr;
    hipEvent_t ev = nullptr, ev2 = nullptr;
    DevBuf<MsmTask> tasks;
    DevBuf<SmulTask> stasks;
    DevBuf<Fr> scal;
    MsmScratch scr;
    DevBuf<TblTask> ttasks;
    DevBuf<uint32_t> digits;
    DevBuf<TAff> conv;
    DevBuf<Jac> res;
    DevBuf<uint32_t> dst;
    DevBuf<uint8_t> comp;
    PinBuf<uint8_t> stage, hcomp;
  };
  SideBufs side_;
  // third stream of the host-driven prover: the per-proof tables of T and U and the two commitments that need them first (B_t, B_u of
  // SameMSM step 1) are not on the critical path of a lone proof until the SameMSM transcript step — they run here, beside phases 1..3
  // and the IPA rounds
  struct TabBufs {
    hipStream_t stream = nullptr;
    hipStream_t dstream = nullptr;   // the device-resident prover's table stream (plain): table build + B_t, B_u beside phase 1 (engine_device.cpp)
    hipEvent_t ev_start = nullptr, ev_m = nullptr, ev_done = nullptr;   // M finalised (main) / M's table row built / B_t, B_u compressed
    DevBuf<uint8_t> blob;      // scalars | TblTask | per-request arrays (enqueue_tbl_phase)
    PinBuf<uint8_t> stage;
    MsmScratch scr;
    DevBuf<uint8_t> comp;
    PinBuf<uint8_t> hcomp;
  };
  TabBufs tab_;
  struct Timed {
    hipEvent_t a, b;
    std::string name;
    double bytes, units;
  };

  void set_crs_impl(size_t ell, const uint8_t* points);
  hipStream_t create_masked_stream(bool upper);
  hipStream_t prefix_stream();
  bool table_stream_on() const;
  const Aff& generator();
  void compress_affine(const Aff* pts, size_t n, uint8_t* out);
  bool unzip_trackers(const uint8_t* trackers, size_t n, std::vector<Aff>& vec_r, std::vector<Aff>& vec_s);
  Aff gen_;
  bool have_gen_ = false;
  const TAff* generator_table();   // the fixed-base table of G (gen_table.hpp), built on the device at first use
  DevBuf<TAff> gen_tab_;
  bool have_gen_tab_ = false;
  std::vector<Aff> crs_host_;   // the ell + 7 CRS points (host copy: M of the Whisk shuffle is an MSM over vec_G | vec_H)
  // ---- device-resident batch prover / verifier (engine_device.cpp) ----
  struct TblPlan : TblShape {   // task descriptors of one table-backed MSM phase whose scalars live in device memory, built once
    bool table_stream = false;   // runs beside the main stream's plans (phase 1t): its own write-only dummy slot
    bool combined = false;       // fused SameMSM rounds: wave w of a proof runs fixed-base block w and table block w (RoundDev::combine)
    bool keep_order = false;     // tasks stay in request (= proof-major) order: the fused round kernels address them by proof (round.hip)
    int force_fix_wpw = 0, force_tbl_wpw = 0;   // != 0: the windows per wave instead of the launch-size heuristics
    DevBuf<TblTask> ttasks;
    DevBuf<FixTask> ftasks;
    DevBuf<uint32_t> meta;   // first partial | partial count | affine destination | compressed-bytes slot | addends[3], per request
  };
  struct DevProver {
    std::vector<const void*> signature;   // buffer addresses + shape the plans were built for
    ProveDev dev;
    DevBuf<uint32_t> perm, mdst;
    DevBuf<Fr> k, mbl, rnd, vec, sc, rvec2;
    DevBuf<uint8_t> slotcomp, proofs;
    TblPlan p1, p1b, p1t, p2, p3;   // p1t: B_t, B_u — the two commitments of phase 1 over per-proof tables, on the table stream
    std::vector<std::unique_ptr<TblPlan>> ipa, smsm;
    // fused log rounds (round.hip; options fused_rounds_max, fused_fix_wpw, fused_tbl_wpw): the plans above in proof-major order, one launch per round
    bool fused = false, fused_smsm = false;   // the IPA rounds / the SameMSM rounds (and the small-batch form of phase 2)
    DevBuf<TAcc> rpart;          // XYZZ partial sums of a round's MSM waves
    DevBuf<uint32_t> rcount;     // [B] arrival counters
    // the last log rounds on materialised folded bases (late.hip; options late_rounds, late_min_batch)
    struct Late {
      bool on = false;
      int m = 16, nr = 4;               // materialised bases per family, late rounds = log2(m)
      size_t j0 = 0;                    // first late round
      DevBuf<TJac> jac;                 // [LATE_FAMILIES][B][m] materialised points
      DevBuf<TAff> tab;                 // [LATE_FAMILIES][B][m][late_tab_entries()] their small multiples
      DevBuf<TJac> part, extra;         // window-group partial sums of a round's outputs [6 B][slices]; the IPA rounds' CRS terms [4 B]
      const uint32_t* h_col = nullptr;
      DevBuf<uint32_t> meta;            // iota | ones | compressed-bytes slots of every late round's outputs
      std::vector<LateRound> ipa, smsm;
      std::vector<size_t> ipa_comp, smsm_comp;   // offsets of a round's slot list inside meta
      const uint32_t* gb_cols = nullptr;
    } late;
    const uint32_t* side_cols = nullptr;
    // R and S from the per-proof tables (option rs_from_tables; prove_reqs.hpp prove_rs_tables / prove_rs_sums): k R, k S as table requests
    // behind the table build, cm_T.T_2 and cm_U.T_2 as sums on the side stream, whose four scalar multiplications become stasks_tbl
    TblPlan prs, prs_sum;
    DevBuf<SmulTask> stasks_tbl;
    const uint32_t* side_cols_tbl = nullptr;   // R, S, cm_A.T_2, cm_B.T_2: the side stream's points that prs_sum has not compressed
    bool rs_tables = false;                    // this prove takes that path (batch_prove_device decides: the option, no k = 0, k on the host)
    hipEvent_t ev_ap = nullptr, ev_rs = nullptr;   // ap: V_APERM and the side stream's scalars are there, rs: k R and k S are in their slots
    hipEvent_t ev_a = nullptr, ev_b = nullptr, ev_c = nullptr, ev_d = nullptr, ev_t1 = nullptr, ev_t2 = nullptr, ev_a2 = nullptr;   // t1: tables built, t2: B_t, B_u in the registry, a2: the prefix stream is about to launch
  };
  DevProver dprove_;
  // Scratch of the tier-0 calls (msm, fold, scale, normalize, decompress, sum_jac): kept between calls — a call used to allocate and free up to ten
  // device buffers of its own (hipMalloc + hipFree: 1.9 ms per 256-point cpx_g1_msm, most of it the allocator).  The contract: every buffer of
  // this set and of ShuffleBufs that has grown beyond kTier0Keep bytes for one large call is given back at the end of that call, on every exit
  // path — CallScope does it, through each(), which is the one place besides its declaration where a buffer is named.
  struct Tier0 {
    DevBuf<Aff> a0, a1;
    DevBuf<Fr> fr;
    DevBuf<MsmTask> mtask;
    DevBuf<SmulTask> stask;
    DevBuf<TJac> w, pt, part;
    DevBuf<Jac> res, jin;
    DevBuf<TAff> conv;
    DevBuf<TblTask> ttask;
    DevBuf<uint32_t> dig;
    DevBuf<uint8_t> bytes, status;
    DevBuf<int> flag;
    DevBuf<Aff> gen;      // copies of the generator: the base of the batched tracker prover's k G and blinder G (whisk.cpp)
    size_t gen_n = 0;     // how many of them are filled in
    // the group tasks of the tracker check (tracker_check_plan.hpp): their bases, scalars and sums live beside the verifier's own buffers
    // above, which the MSM chain would otherwise take; tw: the weights, then stage 2's dense challenges
    DevBuf<Aff> tbase;
    DevBuf<Fr> tscal, tw;
    DevBuf<Jac> tres;
    // what the log-round loops need beside the MSM chain's buffers (loop_plan.hpp): the index lists of every round, the transcript states
    DevBuf<uint32_t> lidx;
    DevBuf<uint64_t> lstate;
    template <class Self, class F> static void each(Self& s, F&& f) {   // (Self: Tier0 or const Tier0)
      each_buf(f, s.a0, s.a1, s.fr, s.mtask, s.stask, s.w, s.pt, s.part, s.res, s.jin, s.conv, s.ttask, s.dig, s.bytes, s.status, s.flag, s.gen, s.tbase, s.tscal, s.tw, s.tres,
               s.lidx, s.lstate);
    }
  } t0_;
  // Scratch of the batched shuffle calls (whisk.cpp), kept and trimmed like the tier-0 set
  struct ShuffleBufs {
    DevBuf<uint8_t> bytes, status, bad;   // uploaded encodings, then the compressed post trackers; decoding verdicts; per-item flags
    DevBuf<uint32_t> off, perm;
    DevBuf<Aff> pts, kpts, tu, zip;       // decoded planes R | S (| T | U | M); k R | k S; T | U; (T_j, U_j) interleaved
    DevBuf<Fr> fr;                        // k | blinders | the scalars of M
    DevBuf<Jac> mjac;
    DevBuf<SmulTask> stask;
    template <class Self, class F> static void each(Self& s, F&& f) {
      each_buf(f, s.bytes, s.status, s.bad, s.off, s.perm, s.pts, s.kpts, s.tu, s.zip, s.fr, s.mjac, s.stask);
    }
  } sh_;
  // vec_T, vec_U and M of the plan's items from the device-resident vec_R | vec_S (sh_.pts), permutations, k and M scalars; loads the batch
  void shuffle_device(const ShufflePlan& pl, std::vector<SmulTask>& tasks);
  static constexpr size_t kTier0Keep = (size_t)64 << 20;
  // One tier-0 or batched Whisk call's hold on the two scratch sets, opened after the argument checks and before the first ensure.  The
  // constructor selects the device; finish() ends the call's device work (stream synchronisation + flush_timers: both can throw, so it is not
  // the destructor); the destructor never throws and keeps the contract above on every exit path.  Left by an exception, it first waits for
  // the stream (best effort) and drops the profiling state of the call: the bound launch events and the events of pending_, unread.
  // Scopes do not nest (std::logic_error): an inner scope's trim would release buffers the outer call still holds pointers into.
  // Host memory that an enqueued copy reads or writes (task lists, offset tables, downloaded verdicts) is declared ABOVE the scope object,
  // empty, and sized where it is needed: it must outlive the destructor's wait.
  struct CallScope {
    explicit CallScope(Engine* e);
    void finish();
    ~CallScope();
    CallScope(const CallScope&) = delete;
    Engine* e_;
    const int uncaught_;
  };
  bool in_call_ = false;
  size_t rng_g1_rounds_ = 0;
  // the bucket-list form of msm / msm_many and the body of fold / fold_many (engine.cpp): the single calls are the many-calls of one task
  void msm_lists(Tier0MsmPlan& pl, const uint32_t* lens, const uint8_t* bases, const uint8_t* scalars, uint8_t* out_jac, uint8_t* out_comp);
  void fold_lanes(size_t families, size_t half, uint8_t* PL, const uint8_t* PR, const uint8_t* gammas, long quad_max);
  // msm_lists without its upload and download (engine.cpp): the chain's own scratch, then launch_msm_endo -> reduce_sets -> launch_msm_tail on
  // device-resident bases and scalars, inside the caller's scope
  void msm_chain_reserve(const Tier0MsmPlan& pl);
  void msm_chain(const Tier0MsmPlan& pl, const uint32_t* lens, const Aff* d_bases, const Fr* d_scalars, Jac* d_res, std::vector<MsmTask>& tasks);
  void msm_chain_run(const Tier0MsmPlan& pl, const MsmTask* d_tasks, Jac* d_res);   // its launches, on pl.count uploaded tasks
  // the one body of ipa_rounds / same_msm_rounds (engine_subarg.cpp).  fam: G | G' | H resp. G | T | U; vec: c | d resp. x
  void loop_rounds(bool ipa, size_t count, size_t n, const uint8_t* const fam[3], const uint8_t* const vec[2], uint8_t* transcripts, uint8_t* rounds_comp,
                   uint8_t* rounds_aff, uint8_t* finals, uint8_t* gammas);
  // its two halves, which the sub-argument provers share (engine_subarg.cpp): the index lists and tasks of every round, uploaded; the rounds
  // themselves on device-resident vectors, bases and states
  void loop_rounds_lists(const LoopPlan& lp, const Tier0MsmPlan& pl, std::vector<uint32_t>& idx, std::vector<MsmTask>& tasks);
  void loop_rounds_resident(const LoopPlan& lp, const Tier0MsmPlan& pl);
  // The one driver of ipa_prove / same_msm_prove / gprod_prove / same_perm_prove and the one of the four verifiers (engine_subarg.cpp): a
  // fixed list of phases, in each of them the parts of the layers in use — same permutation, grand product, then the core (inner product
  // or same multiscalar).  The entry points name the depth in the argument struct; one call's plans, totals, host memory and device
  // pointers are one SubargProveCall / SubargVerifyCall, constructed above the CallScope.
  void subarg_prove(const SubargProveArgs& a);
  void subarg_prove_reserve(SubargProveCall& c);
  void gprod_prove_upload_bases(SubargProveCall& c);
  void same_perm_prove_upload(SubargProveCall& c);
  void gprod_prove_upload(SubargProveCall& c);
  void core_prove_upload(SubargProveCall& c);
  void subarg_prove_upload_tasks(SubargProveCall& c);
  void subarg_prove_draw(SubargProveCall& c);
  void same_perm_prove_steps(SubargProveCall& c);
  void gprod_prove_steps(SubargProveCall& c);
  void core_prove_blinders(SubargProveCall& c);
  void gprod_prove_rdu(SubargProveCall& c);
  void core_prove_steps(SubargProveCall& c);
  void subarg_prove_download(SubargProveCall& c);
  void subarg_verify(const SubargVerifyArgs& a);
  void subarg_verify_reserve(SubargVerifyCall& c);
  void gprod_verify_upload_bases(SubargVerifyCall& c);
  void same_perm_verify_upload(SubargVerifyCall& c);
  void gprod_verify_upload(SubargVerifyCall& c);
  void core_verify_upload(SubargVerifyCall& c);
  void subarg_verify_upload_lists(SubargVerifyCall& c);
  void core_verify_decode(SubargVerifyCall& c);
  void gprod_verify_decode(SubargVerifyCall& c);
  void same_perm_verify_steps(SubargVerifyCall& c);
  void gprod_verify_steps(SubargVerifyCall& c);
  void core_verify_statement(SubargVerifyCall& c);
  void core_verify_scalars(SubargVerifyCall& c);
  void same_perm_verify_weights(SubargVerifyCall& c);
  void subarg_verify_download(SubargVerifyCall& c);
  // n trackers -> the planes r_G | k_r_G: upload + k_decompress of the tracker prover, find-trackers and the candidate list (whisk.cpp)
  void decode_tracker_planes(size_t n, const uint8_t* trackers, std::vector<uint8_t>& canon, std::vector<uint32_t>& off, uint8_t* d_bytes, uint32_t* d_off, Aff* d_pts,
                             uint8_t* d_status);
  // What the batched tracker verifiers begin with (whisk.cpp), inside the caller's scope: upload, k_decompress, k_tracker_challenge.  The host
  // side (rewritten copies of the three inputs, the offset table) is the caller's, declared above its scope; the pointers are into the scratch
  struct TrackerFrontHost {
    std::vector<uint8_t> canon[3];
    std::vector<uint32_t> off;
  };
  struct TrackerFront {
    const uint8_t *d_prf, *d_bad;   // the proofs as uploaded; per item: 0 = every point decoded and s is reduced
    const Aff* pts;                 // planes A | B | k_r_G | r_G | k_G
    const Fr* chal;
  };
  TrackerFront tracker_front(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, TrackerFrontHost& h);
  // the grouped / fused check of tracker proofs (tracker_check_plan.hpp, whisk.cpp): verdict != null = grouped, else partial_jac + n_invalid
  void tracker_check(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand, int* verdict, size_t* n_rechecked,
                     uint8_t* partial_jac, int* n_invalid);
  void enqueue_prove_device();
  void exec_late_round(const LateRound& r, size_t comp_off, const char* what);
  // proofs per launch of the device prover's table build (option table_chunks).  Default: ALL rows in one launch while its scratch (15 doubled
  // copies of every base: 13.5 GB at 8192 proofs of ell = 252) stays below 16 GiB, equal chunks of that size above.  Round 5 shipped two chunks of
  // 4096 (6.7 GB of scratch) on a cross-box comparison; the in-process A/B of round 6 (bench.py --ab table_chunks=0,1, profiles/r06_ab_table_chunks.json)
  // has all rows 0.53 % faster in six of six rounds (every chunk launch ends in a tail of long waves) — and HBM footprint is not the metric.
  size_t table_chunk_rows(size_t batch) const {
    const size_t bytes = batch * np() * (size_t)(pcopies_for(batch) / 2 - 1) * sizeof(TblTmp);
    const size_t nch = opt_.table_chunks > 0 ? std::min<size_t>((size_t)opt_.table_chunks, std::max<size_t>(1, batch))
                                             : std::max<size_t>(1, (bytes + ((size_t)16 << 30) - 1) >> 34);
    return (batch + nch - 1) / nch;
  }
  struct DevVerifier {
    std::vector<const void*> signature;
    VerifyDev dev;
    DevBuf<uint8_t> proofs, slotcomp, status;
    DevBuf<Fr> rnd, vsc, scal, scal_crs;
    DevBuf<uint32_t> flags, src_off, dst, mdst, gidx;
    DevBuf<MsmTask> mtasks, gtasks;
    DevBuf<FixTask> ftasks;
    TblPlan pd;                                  // D and A'
    int fix_wpw = 16, fix_parts = 1, fix_wpw1 = 2, fix_parts1 = 8;
    // the accumulated check (check_plan.hpp): the builders of its task lists over scal | scal_crs | lsum.  mtasks / ftasks[0 .. B): per proof;
    // gtasks / ftasks[B]: fused, its summed CRS scalars behind the point scalars in `scal`
    CheckPlan cplan;
    LocatePlan fplan;                            // fused batch: its groups
    // grouped verifier (locate_plan.hpp): its own group tasks for option locate_groups_max, one fixed-base task per group over the group's
    // summed CRS scalars (lsum), and room for the task lists of the second stage, which located_check writes per call
    LocatePlan lplan;
    DevBuf<MsmTask> ltasks, l2tasks;
    DevBuf<FixTask> lftasks, l2ftasks;
    DevBuf<Fr> lsum;
    int lfix_wpw = 16, lfix_parts = 1;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;
  };
  DevVerifier dverify_;
  void prepare_device_verifier(size_t rand_stride);
  void verify_core_device(const uint8_t* proofs, const uint8_t* rand, size_t rand_stride, int* verdict, uint8_t* fused_partial, int* fused_invalid, size_t* grouped);
  // Where the scalars of a request are: the ONE thing the host-driven and the device-resident path answer differently (prove_reqs.hpp).
  // Staged host scalars (uploaded with the phase) or device memory; the rows of round scalars are d_rout_ on both paths (make_reqs).
  struct ScalAddr {
    const host::S* host = nullptr;
    const Fr* dev = nullptr;
  };
  using ScalAt = std::function<ScalAddr(size_t p, const ReqScal& sc)>;
  // the requests of `list` for every loaded proof, proof by proof: segments, kept point, addends and scalars resolved to addresses;
  // comp_index (optional): the slot of the registry [B][SlotMap::count()] that receives a request's compressed bytes
  std::vector<TblReq> make_reqs(const ReqList& list, const ScalAt& scal_at, std::vector<uint32_t>* comp_index = nullptr);
  void build_plan(TblPlan& pl, const ReqList& list, const ScalAt& scal_at);
  void exec_plan(const TblPlan& pl, uint8_t* d_comp_registry, bool on_table_stream = false);
  // the launches of one table-backed phase (fixed-base kernel, table kernel, reduction, k_finalize_ranges) on stream `st` in scratch `sc`;
  // timed = false: none of them enters the statistics
  void launch_tbl_phase(const TblShape& sh, const TblTask* d_tt, const FixTask* d_ft, const uint32_t* d_meta, uint8_t* d_comp, hipStream_t st, MsmScratch& sc,
                        bool timed = true);
  // host-driven form: plans `reqs`, stages scalars, tasks and per-request arrays in ONE pinned buffer, uploads it with ONE copy and launches
  void enqueue_tbl_phase(const std::vector<TblReq>& reqs, uint32_t dummy_dst, PinBuf<uint8_t>& stage, DevBuf<uint8_t>& blob, DevBuf<uint8_t>& comp, hipStream_t st,
                         MsmScratch& sc, bool timed);
  // R = a x vec_R, S = a x vec_S (and whatever further tasks side_.tasks holds) through the endomorphism bucket-list kernel on stream `st`;
  // the first nfinal results go to their slots (side_.dst)
  void launch_rs(size_t ntasks, size_t nfinal, int slices, bool pairs, hipStream_t st, bool timed);
  // the verifier's accumulated check, per proof and fused (config 5), up to the device-to-host copy of the result into h_comp_
  void launch_check(const MsmTask* d_mt, const FixTask* d_ft, size_t B, size_t NPT, int fix_wpw, int fix_parts, size_t slices);
  void launch_check_fused(const MsmTask* d_gt, const FixTask* d_ft, size_t NT, size_t G, size_t NPT, size_t N, int fix_wpw, int fix_parts);
  bool check_passed(size_t p) const { return h_comp_.p[p * 48] == kCompIdentity; }   // the accumulated check of a valid proof sums to the identity
  // The grouped check (locate_plan.hpp) from its staged scalars on, for both paths: stage 1 (the uploaded lists mt1 / ft1 of lp.NT group tasks,
  // fix_wpw / fix_parts as ft1 was built) -> wait -> the failing groups' flag-free proofs -> their own tasks, written to mt2 / ft2 (room for
  // lp.B) -> wait -> verdict[lp.B].  flags: the proofs' flag words on the host, valid at the latest behind the first wait.  resident: the
  // device-resident path (one wave per window, sleeping waits); otherwise msm_tblw_slices decides and the waits spin.  Returns the proofs rechecked.
  struct LocateTasks {
    const MsmTask* mt1;
    const FixTask* ft1;
    int fix_wpw, fix_parts;
    MsmTask* mt2;
    FixTask* ft2;
  };
  size_t located_check(const CheckPlan& cp, const LocatePlan& lp, const LocateTasks& t, const uint32_t* flags, bool resident, int* verdict);
  struct Untimed {   // keeps a launch sequence out of the statistics
    bool& on;
    const bool was;
    Untimed(Engine* e, bool timed) : on(e->profiling_), was(e->profiling_) { on = was && timed; }
    ~Untimed() { on = was; }
  };
  void prepare_device_prover();
  void ensure_rs_scratch();
  // Where the device-resident prover finds its witnesses and draws.  kind: the side of perm / k / mbl (host: uploaded, device: copied on the
  // device).  rand: the 3n + 9 draws per proof on the host, or null: k_rng_draw makes them in dp.rnd from the states in rng_.states, which
  // states_in (host, nullable: they are there already) fills first and states_out (host) receives, advanced, when the prove has ended.
  struct ProveDraws {
    const uint32_t* perm;
    const uint8_t *k, *mbl;
    hipMemcpyKind kind;
    const uint8_t* rand;
    const uint8_t* states_in;
    uint8_t* states_out;
  };
  void batch_prove_device(const ProveDraws& dr, uint8_t* proofs_out);
  // Device memory that outlives the scratch scope of a `_rng` shuffle call: the states, and the witnesses the shuffle step consumed, until the
  // prover that follows has copied them.  Trimmed like the scratch sets when the call ends (trim_rng).
  struct RngBufs {
    DevBuf<uint8_t> states, mid;
    DevBuf<uint32_t> perm;
    DevBuf<Fr> kb;   // k [count] | blinders [count][4]
  } rng_;
  void trim_rng();
  // the body of the two many-per-call shuffle provers; states != null: the draws come from k_rng_draw and never leave the device
  void whisk_generate_shuffle_proofs_with(size_t count, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                                          const uint8_t* rand, uint8_t* states, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status);

  void run_msm_phase(const std::vector<MsmReq>& reqs, std::vector<uint8_t>* comp_out);
  void run_tbl_phase(const std::vector<TblReq>& reqs, std::vector<uint8_t>* comp_out);
  void reduce_sets(hipStream_t st, MsmScratch& sc, size_t nplain, size_t nweighted, TJac* part = nullptr);
  void verify_core(const uint8_t* proofs, const uint8_t* rand, size_t rand_stride, int* verdict, uint8_t* fused_partial, int* fused_invalid, size_t* grouped = nullptr);
  // The many-per-call shuffle verifiers (whisk.cpp): one body for the explicit pre side and the run's, `verify` on the dense proofs of the
  // loaded batch (plain or grouped).  Host memory of the body: the caller's, declared above its scope
  using ShuffleVerifyFn = std::function<void(const uint8_t* dense, int* verdict)>;
  struct ShuffleVerifyHost {
    std::vector<uint8_t> canon[3], dense, bad;
    std::vector<uint32_t> off;
  };
  bool shuffle_verify_begin(size_t count, int* verdict);
  void shuffle_verify_body(CallScope& call, ShuffleVerifyHost& h, const ShufflePlan& pl, const Aff& G, const uint8_t* pre_trackers, const uint32_t* src,
                           const uint8_t* post_trackers, const uint8_t* proofs, int* verdict, const ShuffleVerifyFn& verify);
  void whisk_verify_shuffle_proofs_with(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, int* verdict,
                                        const ShuffleVerifyFn& verify);
  // The resident candidate list: outside the scratch sets (no call trims it), replaced by the next load only
  struct Candidates {
    size_t n = 0;
    long strict = 0;                // option strict_infinity at load: a run under another value would read the bytes differently
    DevBuf<Aff> pts;                // cand_R | cand_S, n points each
    DevBuf<uint8_t> status;         // the decoder's codes, same layout
    std::vector<uint8_t> bytes;     // n * 96, exactly as given / as the applied items spelt their post trackers
  } cand_;
  // the run beside whisk_verify_shuffle_proofs_with: the same body with the pre side from the list, then the write-back
  void whisk_verify_shuffle_run_with(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, int* verdict, size_t* n_applied,
                                     const ShuffleVerifyFn& verify);
  void batch_prove_tables(const uint32_t* permutation, const uint8_t* k, const uint8_t* m_blinders, const uint8_t* rand, uint8_t* proofs_out);
  // option strict_infinity = 0: `bytes` with every non-canonical infinity encoding (at `offsets` of each of the nrec records) rewritten to
  // the canonical one, in the caller's `store` (canon_infinity.hpp; declared above the caller's CallScope: an enqueued copy reads it); `bytes`
  // itself, with `store` left alone, when there is none or the option is set
  const uint8_t* canonical_infinities(const uint8_t* bytes, size_t nbytes, size_t nrec, size_t rec_stride, const std::vector<size_t>& offsets,
                                      std::vector<uint8_t>& store) const;
  void run_smul(const std::vector<SmulTask>& tasks, int cnt, const host::S* scalars, size_t nscalars, double alg_bytes);
  const uint32_t* idx_list(const std::vector<uint32_t>& v);
  void tick(const char* name, double bytes, double units, bool span = false);
  bool span_ = false;
  void tock();
  // the launch "k_smul" times ran as k_smul_quad (what launch_smul reports): counted under a name of its own, launches only
  void count_smul_quad(bool quad) {
    if (profiling_ && quad) stats_["k_smul_quad"].launches++;
  }
  // One k_smul over ntasks uploaded tasks of `each` elements (whisk.cpp: the tracker prover, find-trackers, the shuffle step): the tasks
  // carry smul_flag(), option scale_any_point as in Engine::scale, and the quad form is off under it
  uint32_t smul_flag() const { return opt_.scale_any_point ? SMUL_PLAIN : 0u; }
  void smul_tasks(const SmulTask* d_tasks, size_t ntasks, size_t each, double units) {
    tick("k_smul", 224.0 * units, units);
    count_smul_quad(launch_smul(d_tasks, (int)ntasks, (int)each, stream_, false, smul_flag() ? 0 : opt_.smul_quad_max));
    tock();
  }
  void flush_timers();
  template <class F> void parallel_for(size_t n, F&& f);
  std::unique_ptr<SpinTeam> team_;
  static std::atomic<int>& live_engines();   // engine contexts alive in this process (bounds the spin team)
  struct TeamScope {   // engages the spin team for a small batch's call
    SpinTeam* t = nullptr;
    TeamScope(Engine* e, size_t batch);
    ~TeamScope() {
      if (t) t->release();
    }
  };
  struct HostSpan {
    HostSpan(Engine* e, const char* name);
    ~HostSpan();
    Engine* e_;
    const char* name_;
    std::chrono::steady_clock::time_point t0_;
  };
  void wait_stream();
  void wait_stream_blocking();                // sleeps instead of spinning: the one wait of a device-resident call lasts tens of milliseconds
  hipEvent_t ev_block_ = nullptr;
  void wait_side();                          // blocks on the side stream's event (side_.ev)
  void transcript_prefix_async(size_t B);
  bool device_prefix(size_t B) const;         // run the whole protocol on the GPU (batches >= CPX_DEVICE_MIN_BATCH) or drive it from the host

  // per-proof table row: copy-major [copies][NP]
  size_t np() const { return PtabRow(n_).count(); }   // M | T_b | U_b
  TAff* ptab(size_t p) const { return d_ptab_.p + p * (size_t)pcopies_ * np(); }
  TblSeg pseg(size_t p, size_t off, uint32_t cnt, const uint32_t* idx = nullptr) const { return TblSeg{ptab(p) + off, idx, (uint32_t)np(), cnt}; }
  TblSeg cseg(size_t off, uint32_t cnt, const uint32_t* idx = nullptr) const { return TblSeg{ctab() + off, idx, (uint32_t)nc(), cnt}; }
  size_t nc() const { return CtabCols(n_).count(); }   // CRS table columns: G | Hvec | H | G_t | G_u | G_sum | H_sum
  Aff* pp(size_t p) const { return d_pp_.p + p * pp_stride_; }
  Aff* slot(size_t p, int s) const { return pp(p) + 4 * ell_ + s; }
  uint32_t slot_index(size_t p, int s) const { return (uint32_t)(p * pp_stride_ + 4 * ell_ + s); }

  int device_;
  Options opt_ = default_options();
  hipStream_t stream_ = nullptr;
  bool profiling_ = false;
  int host_threads_ = 0;
  std::unique_ptr<WorkerPool> pool_;
  std::map<std::string, KernelStat> stats_;
  std::vector<Timed> pending_;

  // CRS
  size_t ell_ = 0, n_ = 0, L_ = 0;
  DevBuf<Aff> d_crs_;        // [n+1] G | Hvec | H      (IPA basis + H)
  DevBuf<Aff> d_crs_gb_;     // [n]   G | Hvec[0..2) | G_t | G_u   (SameMSM basis)
  Aff crs_single_[5];        // H, G_t, G_u, G_sum, H_sum (host copies)
  uint8_t crs_H_comp_[48];

  // shifted-base tables (all-MSM prover)
  static constexpr int copies_ = 32;   // copies per base of the CRS table: 2^(8c) P and z^2 2^(8c) P, c < 16: one per radix-256 window of the split scalar
  // The per-proof tables have a copy count of their own, 32 / segments (kernels.h "table-backed MSM").  Two segments where the batch's
  // path reads them through the stand-alone bucket-list waves and k_late_uniform: the device-resident prover whose SameMSM rounds are not
  // fused.  The fused rounds (round.hip), the lone-proof kernels and the host-driven prover keep one-segment tables.
  struct LateShape {
    int m, nr;
    bool on;
  };
  LateShape late_shape(size_t batch) const;   // the late rounds of a device-resident batch (options late_rounds, late_m, late_min_batch)
  bool smsm_may_fuse(size_t batch) const;     // whether the batch's SameMSM rounds may run as fused launches (options fused_smsm_max, ...)
  int tbl_segments_for(size_t batch) const;
  int pcopies_for(size_t batch) const { return copies_ / tbl_segments_for(batch); }
  int pcopies_ = copies_;              // copy count of d_ptab_ as the prover in progress lays it out (set when a prove starts)
  // CRS tables are immutable once built and large (15 GB at ell = 252): engines on the same device that are
  // given the same CRS share one copy (process-wide registry in engine.cpp).
  struct CrsTables {
    int device = 0, fix_bits = 0;
    std::vector<uint8_t> key;   // the CRS points the tables were built from
    DevBuf<TAff> ctab;         // shifted copies [copies][n+3] : G | Hvec | H | G_t | G_u   (table representation)
    DevBuf<TFix> fixtab;       // multiples [256/c][2^(c-1)][n+5], one 128-byte line per entry
  };
  std::shared_ptr<CrsTables> crs_tab_;
  const TAff* ctab() const { return crs_tab_ ? crs_tab_->ctab.p : nullptr; }
  const TFix* fixtab() const { return crs_tab_ ? crs_tab_->fixtab.p : nullptr; }
  DevBuf<TAff> d_ptab_;      // per-proof tables [B][copies][NP]
  MsmScratch main_;                      // the main stream's MSM scratch: shared by the prover's phases, the verifier and the tier-0 calls
  DevBuf<uint32_t> d_digits_;            // recoded scalars of the endomorphism bucket MSM (9 words per point)
  DevBuf<Aff> d_psrc_;       // their standard-form sources [B][NP] : M | T_b | U_b
  DevBuf<TblTmp> d_tbltmp_;
  DevBuf<TblTask> d_ttasks_;
  int fix_bits_cfg_ = 16;    // configured radix of the fixed-base CRS table of multiples: 2^16 (15 GB at ell = 252) or 2^8 (0.1 GB)
  int fix_bits_ = 16;        // radix of the table in use (set_crs falls back to 2^8 when the 2^16 table does not fit in free HBM)
  DevBuf<FixTask> d_ftasks_;
  DevBuf<uint8_t> d_blob_;   // scalars + task descriptors + ranges of a host-driven table phase, one upload (run_tbl_phase)

  // batch
  size_t B_ = 0;
  size_t consts_rows_ = 0;   // rows of d_pp_ / d_psrc_ whose per-CRS constants are in place (load_rows)
  void load_rows(size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M, bool from_device);
  struct Stage {   // device staging area of batch_load_begin
    DevBuf<Aff> R, S, T, U;
    DevBuf<Jac> M;
    hipStream_t stream = nullptr;
    hipEvent_t uploaded = nullptr, consumed = nullptr;
    bool have_consumed = false;
    size_t batch = 0, ell = 0;
  } stage_;
  size_t pp_stride_ = 0;     // 4*ell + NSLOT
  DevBuf<Aff> d_pp_;         // per proof: R|S|T|U | slots
  DevBuf<Jac> d_Mjac_;

  // phase scratch
  DevBuf<MsmTask> d_tasks_;
  DevBuf<SmulTask> d_stasks_;
  DevBuf<Fr> d_scal_;
  DevBuf<TJac> d_wsum_, d_part_;   // window sums / Horner partials of the bucket MSM (table representation)
  DevBuf<Jac> d_res_;
  DevBuf<uint32_t> d_big_idx_;   // gather list of the fused verifier's per-proof points
  DevBuf<TAff> d_conv_;            // table-form copies of the bases of a bucket-MSM phase
  DevBuf<uint32_t> d_dst_;
  DevBuf<uint8_t> d_comp_;
  PinBuf<uint8_t> h_stage_;
  PinBuf<uint8_t> h_comp_;
  PinBuf<uint8_t> h_inst_comp_, h_mcomp_, h_pts_, h_status_;   // compressed instance vectors / M, proof points in, decompression status
  PinBuf<uint32_t> h_u32_;
  DevBuf<Fr> d_rvec_, d_rout_, d_rgam_, d_rbeta_;   // device-resident round vectors, per-round scalars, challenges
  PinBuf<Fr> h_rvec_, h_rgam_, h_rfin_;
  DevBuf<uint8_t> d_mcomp_;                 // compressed M of every proof
  DevBuf<uint64_t> d_tstate_;               // transcript states after the prefix [B][27]
  DevBuf<Fr> d_veca_;                       // vec_a [B][ell]
  DevBuf<uint8_t> d_vin_;
  DevBuf<uint32_t> d_vdst_;
  std::map<std::vector<uint32_t>, uint32_t*> idx_cache_;
  std::vector<uint32_t*> idx_allocs_;
  DevBuf<uint8_t> d_bytes_;
  DevBuf<uint8_t> d_status_;
};

}  // namespace cpx
