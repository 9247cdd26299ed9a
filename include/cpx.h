/* cpx.h — C-ABI of the MI355X (gfx950) Curdleproofs G1 core.
 *
 * This is the drop-in boundary for the one hot path of asn-d6/curdleproofs: the BLS12-381 G1 group
 * arithmetic behind `CurdleproofsProof::{new,verify}`.  The reference is a pure-Rust crate with no
 * FFI of its own; the functions below are what an FFI for this path would bind, each one citing the
 * reference interface it replaces (paths relative to the reference repo, file:line).
 * INTEGRATION.md shows the Rust-side `extern "C"` block and the three edits that route the crate here.
 *
 * Data layouts — exactly arkworks' in-memory limbs, so a Rust caller passes slices through untouched:
 *   Fr     32 B   4 x u64 little-endian limbs, Montgomery form (R = 2^256)      = ark_bls12_381::Fr
 *   Fp     48 B   6 x u64 little-endian limbs, Montgomery form (R = 2^384)
 *   affine 96 B   x || y ; the point at infinity is encoded as 96 zero bytes     ~ G1Affine {x,y,infinity}
 *   jac   144 B   X || Y || Z Jacobian ; infinity <=> Z == 0                     = G1Projective
 *   compressed 48 B  zcash/ark-serialize compressed encoding
 *
 * Ownership: the caller owns every buffer it passes (valid for the duration of the call only); the
 * library owns device memory, the HIP stream and the device-resident CRS inside the opaque cpx_ctx.
 * Threading: one ctx = one HIP device + one stream; a ctx is not re-entrant, distinct ctxs may be driven
 * from distinct host threads.  Errors: int return, 0 = ok, negative = CPX_ERR_*; nothing unwinds
 * across this boundary (the reference's panics — util.rs:20, inner_product_argument.rs:115-116 —
 * become error codes).  There is NO CPU fallback: without a usable HIP device every call fails.
 */
#ifndef CPX_H
#define CPX_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPX_OK 0
#define CPX_ERR_ARG (-1)         /* bad length / null pointer                                   */
#define CPX_ERR_NOT_POW2 (-2)    /* ell + 4 not a power of two (inner_product_argument.rs:116)  */
#define CPX_ERR_HIP (-3)         /* HIP runtime failure (no device, OOM, launch error)          */
#define CPX_ERR_VERIFY (-4)      /* ProofError::VerificationError (errors.rs:9)                 */
#define CPX_ERR_DESERIALIZE (-5) /* ark_serialize::SerializationError                           */
#define CPX_ERR_STATE (-6)       /* call order: CRS / batch not set                             */
#define CPX_ERR_INTERNAL (-7)

typedef struct cpx_ctx cpx_ctx;

/* ---- context ------------------------------------------------------------------------------- */
/* cpx_ctx_create fails with CPX_ERR_HIP when there is no such HIP device (there is no CPU fallback) and with CPX_ERR_STATE when the host
 * CPU lacks AVX2 / BMI2 / FMA / ADX (the library's host code is built for x86-64-v3 + ADX; every EPYC that hosts an MI355X has them) —
 * instead of dying of SIGILL later.  cpx_last_error(NULL) then says why the calling thread's last cpx_ctx_create failed.
 * The library does not touch the process environment.  HIP maps streams onto GPU_MAX_HW_QUEUES hardware queues (default 4) and a context
 * owns four streams that are meant to overlap: export GPU_MAX_HW_QUEUES=8 before the process's first HIP call when two or more contexts
 * share a process (the Python package and bench.py do). */
int cpx_ctx_create(int device_id, cpx_ctx** out);
void cpx_ctx_destroy(cpx_ctx* ctx);
const char* cpx_last_error(const cpx_ctx* ctx); /* message of the last failing call on this ctx    */
int cpx_device_count(void);

/* Per-context tunables (kernel selection thresholds, radix of the fixed-base table, batch size from which the protocol runs on the
 * device, ...): key = one of the names listed in curdleproofs_amd/csrc/kernels.h `struct Options` ("fix_bits", "device_min_batch",
 * "tbw_wpw", "reduce_wave_max", "fold_quad_max", ...).  A new context starts from the built-in defaults, overridden by CPX_<KEY> environment
 * variables read once per process; everything after that goes through these calls and concerns this context only.  Results never
 * depend on an option (tests/test_gpu_parity.py::test_engine_variants_stay_bit_exact), only speed does.  "fix_bits" takes effect at
 * the next cpx_ctx_set_crs.  Unknown key / value out of range -> CPX_ERR_ARG.  cpx_ctx_get_option also answers the read-only key
 * "fix_bits_effective": the radix of the fixed-base table this context actually uses (the fallback of cpx_ctx_set_crs; 0 = no CRS),
 * "tbl_segments_effective": the layout of the per-proof tables the loaded batch proves with (1 = 16 + 16 shifted copies per
 * base, 2 = 8 + 8; option "tbl_segments"; 0 = no batch loaded), and "tier0_scratch_bytes": the device memory the context keeps between
 * calls as scratch of the cpx_g1_* and the many-per-call cpx_whisk_* functions (0 on a new context; a buffer that one large call grew
 * beyond 64 MiB is given back when that call ends, however it ends, so the value stays below 64 MiB per buffer). */
int cpx_ctx_set_option(cpx_ctx* ctx, const char* key, long long value);
int cpx_ctx_get_option(const cpx_ctx* ctx, const char* key, long long* value);

/* Optional: page-locked host buffers.  Any host memory may be passed to the calls below; buffers obtained here let the batch calls
 * move their inputs / outputs by asynchronous DMA (no staging copies, transfers overlap the kernels of other contexts). */
void* cpx_host_alloc(size_t bytes);
void cpx_host_free(void* p);

/* crs.rs:37-58 `CurdleproofsCrs::from_points(ell, points)`: ell + 7 affine points in the order
 * vec_G[ell] | vec_H[4] | H | G_t | G_u.  Uploads them, computes G_sum / H_sum on the device and builds the fixed-base
 * tables (option "fix_bits": radix 2^16 by default, 17.5 GB at ell = 252; 2^19 = 122 GB; falls back 19 -> 16 -> 8 when free HBM is short).  `n_points` is the number of
 * points behind `points`: fewer than ell + 7 is the reference's "not enough points" error (crs.rs:40-42) ->
 * CPX_ERR_ARG; surplus points are ignored, as the reference's slicing does.  On failure the context holds no CRS. */
int cpx_ctx_set_crs(cpx_ctx* ctx, size_t ell, const uint8_t* points, size_t n_points);
int cpx_crs_sums(const cpx_ctx* ctx, uint8_t g_sum[96], uint8_t h_sum[96]);
size_t cpx_proof_size(const cpx_ctx* ctx); /* 48*(18+10*log2(ell+4)) + 32*7, e.g. 4928 at ell = 252 */
size_t cpx_batch_size(const cpx_ctx* ctx); /* instances currently loaded (cpx_batch_load; 1 after a cpx_whisk_*_shuffle_proof call, count after the batched ones); 0 = none */

/* ---- tier 0: the reference's MSM funnel and the loops that bypass it ------------------------- */
/* util.rs:19-22 `msm(points: &[G1Affine], scalars: &[Fr]) -> G1Projective` */
int cpx_g1_msm(cpx_ctx* ctx, const uint8_t* bases /* n*96 */, const uint8_t* scalars /* n*32 */, size_t n, uint8_t out[144]);
/* util.rs:25-29 `msm_from_projective(points: &[G1Projective], scalars: &[Fr])` */
int cpx_g1_msm_jac(cpx_ctx* ctx, const uint8_t* bases /* n*144 */, const uint8_t* scalars, size_t n, uint8_t out[144]);
/* inner_product_argument.rs:177-178, same_multiscalar_argument.rs:128-130:
 *   PL[i] <- (PL[i] + PR[i] * gamma).into_affine(), i < half, in place */
int cpx_g1_fold(cpx_ctx* ctx, uint8_t* PL /* half*96 */, const uint8_t* PR /* half*96 */, const uint8_t gamma[32], size_t half);
/* grand_product_argument.rs:90-102 (per-element scalars, scalar_stride = 32) and util.rs:94-95
 * (one shared scalar, scalar_stride = 0):  out[i] <- (P[i] * s_i).into_affine()
 * PRECONDITION of cpx_g1_fold / cpx_g1_scale (as of arkworks' G1Affine, whose deserialisation checks it): the points lie in the order-r
 * subgroup — the scalar is split by the G1 endomorphism, k P = t P + q (-phi(P)), an identity of that subgroup only; on a point of
 * E(Fp) outside it a scalar >= z^2 / 2 gives a wrong result.  Context option "scale_any_point" = 1 selects the plain 257-step
 * double-and-add for both calls, valid on all of E(Fp) (the cofactor multiplication of the hash-to-curve CRS, tests/crs.rs:38). */
int cpx_g1_scale(cpx_ctx* ctx, const uint8_t* P /* n*96 */, const uint8_t* scalars, size_t scalar_stride, size_t n, uint8_t* out /* n*96 */);
/* The calls of ONE log round in two calls.  Within a round the cross terms do not depend on each other, nor do the basis folds; only the
 * challenge stands between the two groups.  cpx_g1_msm_many takes the cross terms, cpx_g1_fold_many the folds: each is one upload, one chain of
 * kernel launches whose length does not depend on the count, one download and ONE stream synchronisation, so a round costs two calls and two
 * synchronisations instead of 4 + 2 (IPA) or 6 + 3 (SameMSM).  Conventions of the batched tracker calls: scalars are 32-byte Montgomery limbs;
 * count = 0 (families = 0, half = 0) is a no-op returning CPX_OK; a NULL input with work to do is CPX_ERR_ARG and nothing is written; no CRS is
 * needed and the loaded batch is untouched (cpx_batch_size is unchanged).  Same subgroup precondition as the single calls' default paths.
 * COST.  Every tier-0 call above is its own upload, kernel chain, download and synchronisation: by the library's own figures
 * (curdleproofs_amd/csrc/kernels.h, kernels.hip) a cpx_g1_msm of 1 - 63 points takes 0.72 - 0.77 ms and the one-lane scalar multiplication
 * behind cpx_g1_fold is a chain of 4.6 ms, which at 8 + 8 rounds (ell = 252: about 94 MSM calls and 41 fold / scale calls per proof) comes to
 * well over 200 ms per proof.  What a round costs through the two calls below is measured by scripts/tier0_round_timing.py and recorded in
 * INTEGRATION.md section 3. */
/* util.rs:19-22 `msm` for `count` independent (points, scalars) pairs: the cross terms of one log round —
 * inner_product_argument.rs:158-161, same_multiscalar_argument.rs:107-112.
 *   lens     count lengths, ragged on purpose (L_C = msm(G_R, c_L) + <c_L, d_R> H is one task of n/2 + 1 points beside L_D of n/2);
 *            a task of length 0 gives the identity: Z == 0 in out_jac, 0xc0 || 0^47 in out_compressed
 *   bases, scalars  the tasks' points and scalars back to back, task after task
 * Every task takes the endomorphism bucket-list path whatever its length (option "msm_endo_min" is not consulted).  Either output may be
 * NULL.  At most 2^16 tasks and 2^24 points per call: more is CPX_ERR_ARG before anything else is read. */
int cpx_g1_msm_many(cpx_ctx* ctx, size_t count, const uint32_t* lens /* count */, const uint8_t* bases /* sum(lens)*96, task after task */,
                    const uint8_t* scalars /* sum(lens)*32 */, uint8_t* out_jac /* count*144 */, uint8_t* out_compressed /* count*48 */);
/* inner_product_argument.rs:177-178, same_multiscalar_argument.rs:128-130 for `families` vectors of `half` elements:
 *   PL[f][i] <- (PL[f][i] + PR[f][i] * gammas[f]).into_affine(), in place
 * Option "fold_quad_max" (default 1536): a call of at most that many elements (families * half) runs with a quad of lanes per element
 * (k_smul_quad, a third of the one-lane chain's latency); above it, at 0, or with "scale_any_point" = 1 it runs as the one-lane k_smul that
 * cpx_g1_fold always takes.  At most 2^24 elements per call (CPX_ERR_ARG, PL untouched). */
int cpx_g1_fold_many(cpx_ctx* ctx, size_t families, size_t half, uint8_t* PL /* families*half*96 */, const uint8_t* PR /* families*half*96 */,
                     const uint8_t* gammas /* families*32 */);
/* ---- The log-round loops themselves, one call each, and the transcript as a value ----
 * The reference's sub-argument provers spend their time in two loops: InnerProductProof::new (inner_product_argument.rs:150-186) and
 * SameMultiscalarProof::new (same_multiscalar_argument.rs:99-136).  Through the two calls above a round still crosses the bus and
 * synchronises twice, because the Fiat-Shamir challenge between them is drawn on the host.  The two calls below run all L = log2 n rounds of
 * `count` independent items on the device, transcript included: one upload, one download, ONE stream synchronisation per call, and a number
 * of kernel launches that depends on L only (per round the chain of cpx_g1_msm_many, k_finalize and one k_loop_step), never on count.  What that saves is measured by
 * scripts/loop_rounds_timing.py (profiles/loop_rounds.md).
 *
 * A transcript state is CPX_TRANSCRIPT_BYTES = 216 bytes = 27 little-endian u64: the 25 Keccak lanes of merlin's STROBE-128 state, then
 * `pos`, then `pos_begin`.  merlin's `cur_flags` is not part of it: between whole Merlin messages it has no effect.  The five
 * cpx_transcript_* calls are host only (no context, no GPU, like cpx_rng_from_u64) and are merlin::Transcript / the crate's
 * CurdleproofsTranscript operation by operation; labels are byte strings with a length.  A state with pos > 165 or pos_begin > 166 is
 * CPX_ERR_ARG in every call that takes one, the two device calls included (checked on the host before anything is launched: pos indexes
 * the state); so are a NULL with work to do and a message or challenge longer than 2^32 - 1 bytes.  On any error the state is left as it was. */
#define CPX_TRANSCRIPT_BYTES 216
int cpx_transcript_new(const uint8_t* label, size_t label_len, uint8_t state_out[CPX_TRANSCRIPT_BYTES]);   /* merlin::Transcript::new */
int cpx_transcript_append_message(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, const uint8_t* msg, size_t len);
/* transcript.rs:29-33 `append` on an Fr: its 32 canonical little-endian bytes as one message.  A scalar >= r is CPX_ERR_ARG. */
int cpx_transcript_append_scalar(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, const uint8_t scalar_mont[32]);
int cpx_transcript_challenge_bytes(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, uint8_t* out, size_t len);
/* transcript.rs:41-54 `get_and_append_challenge`: 64 challenge bytes, Fr::from_random_bytes, retried until canonical and non-zero, and the
 * accepted scalar appended back under the same label.  out_mont: Montgomery limbs. */
int cpx_transcript_challenge_scalar(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, uint8_t out_mont[32]);
/* inner_product_argument.rs:150-186 for `count` items of n = 2^L elements each, item by item exactly the reference's loop:
 *   every round appends L_C, L_D, R_C, R_D (one append_message of the 48 compressed bytes each, label "ipa_loop"; the identity as
 *   0xc0 || 0^47), draws gamma under "ipa_gamma" (retries and the append-back included), and folds c_L += gamma^-1 c_R, d_L += gamma d_R.
 *   G, G_prime  the bases as they enter the loop, item after item          H       the point the loop uses (the reference's local
 *   vec_c, vec_d  the vectors as they enter the loop (:136-139)                    `H = crs_H.mul(beta)`, :140), one per item
 *   transcripts  in: the states at loop entry; out: advanced by all L rounds
 *   rounds_compressed / rounds_affine  per item and round L_C, L_D, R_C, R_D; either may be NULL
 *   finals  per item c_final, d_final                                      gammas  per item the L challenges; may be NULL
 * The outputs are the group elements the reference computes, so the bytes are bit-exact, though no basis is ever folded here: every cross
 * term is an MSM over the uploaded bases (curdleproofs_amd/csrc/loop_plan.hpp).  Conventions of the batched tier-0 calls: scalars are
 * Montgomery limbs, and a scalar >= r is CPX_ERR_ARG for the whole call; points must lie in the subgroup; the identity (96 zero bytes) is a
 * legal base; count = 0 is a no-op returning CPX_OK; n = 1 runs no round (finals = the inputs, states unchanged); n = 0 or not a power of
 * two is CPX_ERR_NOT_POW2; NULL with work to do is CPX_ERR_ARG; on any return other than CPX_OK nothing is written, states included; no CRS
 * is needed and the loaded batch is untouched.  A round is one cpx_g1_msm_many of 4 count tasks: at most 16384 items and
 * count (2 n + 2) <= 2^24 points per round; more is CPX_ERR_ARG before anything is read.  Scratch is the tier-0 set (two of its 23 buffers
 * serve these calls alone), trimmed by the same 64 MiB rule. */
int cpx_ipa_rounds(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G /* count*n*96 */, const uint8_t* G_prime /* count*n*96 */, const uint8_t* H /* count*96 */,
                   const uint8_t* vec_c /* count*n*32 */, const uint8_t* vec_d /* count*n*32 */, uint8_t* transcripts /* count*216, in/out */,
                   uint8_t* rounds_compressed /* count*L*4*48, may be NULL */, uint8_t* rounds_affine /* count*L*4*96, may be NULL */,
                   uint8_t* finals /* count*2*32 */, uint8_t* gammas /* count*L*32, may be NULL */);
/* same_multiscalar_argument.rs:99-136 likewise: per round L_A, L_T, L_U, R_A, R_T, R_U under "same_msm_loop", gamma under "same_msm_gamma",
 * x_L += gamma^-1 x_R; finals = x_final.  At most 10922 items and 3 count n <= 2^24 points per round. */
int cpx_same_msm_rounds(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U /* count*n*96 each */,
                        const uint8_t* vec_x /* count*n*32 */, uint8_t* transcripts /* count*216, in/out */, uint8_t* rounds_compressed /* count*L*6*48, may be NULL */,
                        uint8_t* rounds_affine /* count*L*6*96, may be NULL */, uint8_t* finals /* count*32 */, uint8_t* gammas /* count*L*32, may be NULL */);
/* InnerProductProof::verify (inner_product_argument.rs:202-326, its scalars :202-262) for `count` independent stand-alone proofs over n = 2^L
 * bases each, item by item what the reference computes against an MsmAccumulator of its own (msm_accumulator.rs:37-68):
 *   G, crs_H     the bases (`crs_G_vec`, affine) and the point crs_H     C, D, z   the statement; vec_u as in :262, :308-317
 *   proofs       the reference's own `serialize` bytes (inner_product_argument.rs:328-338): B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D
 *                compressed, then c_final, d_final as canonical little-endian scalars
 *   rand         per item the two values `accumulate_check` would draw (msm_accumulator.rs:44), in call order; a zero or unreduced value
 *                is CPX_ERR_ARG for the whole call, as in cpx_accum_check
 *   transcripts  in: the states before `verify`; out: advanced by the whole `verify`, step 1 (:283-287) included, whatever the verdict
 *   challenges   per item alpha, beta, gamma_1..L (Montgomery limbs); may be NULL
 *   verdicts     per item CPX_OK, CPX_ERR_VERIFY (the item's accumulator does not verify, :55-68), or CPX_ERR_DESERIALIZE: a point that
 *                does not decode or lies outside the subgroup, or a scalar >= r.  The reference never reaches `verify` for such bytes: the
 *                item's state is returned unchanged and its challenges are zero.
 * crs_H, C, D are 144-byte Jacobian points, any representative, Z = 0 for the identity (what cpx_g1_msm* return and cpx_accum_check takes);
 * G is affine under the tier-0 precondition (in the subgroup, the identity legal); z, vec_u are Montgomery limbs, a value >= r is CPX_ERR_ARG.
 * Encodings of the identity inside a proof follow option strict_infinity as in the batched verifiers.  n = 1 is a real check (L = 0, no round
 * points, s = [1]); n = 0 or not a power of two is CPX_ERR_NOT_POW2; count = 0 is a no-op returning CPX_OK; NULL with work to do and an
 * invalid transcript state are CPX_ERR_ARG.  An item is one task of one cpx_g1_msm_many over its n + 4 L + 5 points
 * (curdleproofs_amd/csrc/subarg_check_plan.hpp): at most 2^16 items and 2^24 points per call, checked before anything is read.  On any
 * return other than CPX_OK nothing is written.  One upload, one download, one stream synchronisation; launches that depend on L only; no
 * CRS is needed and the loaded batch is untouched.  Scratch is the tier-0 set. */
int cpx_ipa_verify(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G /* count*n*96 */, const uint8_t* crs_H /* count*144 */, const uint8_t* C /* count*144 */,
                   const uint8_t* D /* count*144 */, const uint8_t* z /* count*32 */, const uint8_t* vec_u /* count*n*32 */,
                   const uint8_t* proofs /* count*(48*(2+4L)+64) */, const uint8_t* rand /* count*2*32 */, uint8_t* transcripts /* count*216, in/out */,
                   uint8_t* challenges /* count*(2+L)*32, may be NULL */, int* verdicts /* count */);
/* SameMultiscalarProof::verify (same_multiscalar_argument.rs:153-261) likewise: bases G, T, U (vec_T and vec_U are hashed in step 1 from
 * their encodings, :230-233), statement A, Z_t, Z_u; proofs are B_a, B_t, B_u, vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final
 * (same_multiscalar_argument.rs:263-275); three random factors per item; challenges are alpha, gamma_1..L; 3 n + 6 L + 6 points per item. */
int cpx_same_msm_verify(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U /* count*n*96 each */, const uint8_t* A,
                        const uint8_t* Z_t, const uint8_t* Z_u /* count*144 each */, const uint8_t* proofs /* count*(48*(3+6L)+32) */,
                        const uint8_t* rand /* count*3*32 */, uint8_t* transcripts /* count*216, in/out */, uint8_t* challenges /* count*(1+L)*32, may be NULL */,
                        int* verdicts /* count */);
/* InnerProductProof::new (inner_product_argument.rs:98-199) for `count` independent stand-alone statements over n = 2^L bases each, the
 * whole function in ONE call: generate_ipa_blinders (:42-82), B_c = <r_c, G>, B_d = <r_d, G'>, step 1 of the transcript (C, D, z, B_c, B_d
 * under "ipa_step1", alpha under "ipa_alpha", beta under "ipa_beta"), the rewrite of the vectors by alpha, H = beta crs_H, and the L rounds
 * of cpx_ipa_rounds on the same device memory.
 *   G, G_prime   the bases (`crs_G_vec`, `crs_G_prime_vec`), affine          crs_H, C, D   144-byte Jacobian points, any representative,
 *   z, vec_c, vec_d  the statement's scalar and the witness                                Z = 0 for the identity
 *   rand         per item the 2 n - 2 values the reference draws, in its order: r [n], then z [n - 2] (:46-47)
 *   transcripts  in: the states before `new`; out: advanced by the whole `new`: step 1, alpha, beta and all L rounds
 *   proofs       the reference's `serialize` of what `new` returns (:328-338): B_c, B_d, vec_L_C, vec_R_C, vec_L_D, vec_R_D compressed,
 *                then c_final, d_final as canonical little-endian scalars — what cpx_ipa_verify takes
 *   challenges   per item alpha, beta, gamma_1..L (Montgomery limbs); may be NULL
 *   status       per item CPX_OK, or CPX_ERR_ARG where the reference panics in generate_ipa_blinders: c[n-2] = 0 (:69) or the denominator
 *                -r[n-2] c[n-2]^-1 c[n-1] + r[n-1] = 0 (:71).  Such an item's proof bytes and challenges are zero and its transcript state
 *                is unchanged; the other items are unaffected and the call returns CPX_OK.  Pre-fill `status` with a non-zero code, as for
 *                the other batched calls: an entry the library has not written is then never read as a proof.
 * Conventions of cpx_ipa_rounds / cpx_ipa_verify: scalars are Montgomery limbs and a value >= r anywhere is CPX_ERR_ARG for the call; the
 * identity is a legal base and a legal statement point; count = 0 is a no-op returning CPX_OK; n = 0 or not a power of two is
 * CPX_ERR_NOT_POW2; n = 1 is CPX_ERR_ARG (the reference's n - 2 underflows), n = 2 is real (no free z draw, delta an empty sum); NULL with
 * work to do and an invalid transcript state are CPX_ERR_ARG; the limits are those of one cpx_ipa_rounds (16384 items,
 * count (2 n + 2) <= 2^24), checked before anything is read; on any return other than CPX_OK nothing is written, states included.  One
 * upload, one download, ONE stream synchronisation; launches that depend on L only (curdleproofs_amd/csrc/subarg_prove_plan.hpp,
 * subarg_prove.hip); no CRS is needed and the loaded batch is untouched.  Scratch is the tier-0 set (no buffer beyond its 23), trimmed by
 * the same 64 MiB rule.  Measurements: profiles/subarg_prove.md. */
int cpx_ipa_prove(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime /* count*n*96 each */, const uint8_t* crs_H, const uint8_t* C,
                  const uint8_t* D /* count*144 each */, const uint8_t* z /* count*32 */, const uint8_t* vec_c, const uint8_t* vec_d /* count*n*32 each */,
                  const uint8_t* rand /* count*(2n-2)*32 */, uint8_t* transcripts /* count*216, in/out */, uint8_t* proofs /* count*(48*(2+4L)+64) */,
                  uint8_t* challenges /* count*(2+L)*32, may be NULL */, int* status /* count */);
/* SameMultiscalarProof::new (same_multiscalar_argument.rs:69-150) likewise: bases G, T, U, statement A, Z_t, Z_u, witness vec_x; rand is
 * vec_r, n values per item (:78); step 1 hashes A, Z_t, Z_u, vec_T, vec_U, B_a, B_t, B_u under "same_msm_step1" and draws alpha under
 * "same_msm_alpha"; proofs are B_a, B_t, B_u, vec_L_A, vec_L_T, vec_L_U, vec_R_A, vec_R_T, vec_R_U, x_final (:263-275); challenges are
 * alpha, gamma_1..L.  n = 1 is real: L = 0, the proof is the three B points and x_final = r_0 + alpha x_0.  Every item's status is CPX_OK.
 * Limits of one cpx_same_msm_rounds: 10922 items, 3 count n <= 2^24. */
int cpx_same_msm_prove(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U /* count*n*96 each */, const uint8_t* A,
                       const uint8_t* Z_t, const uint8_t* Z_u /* count*144 each */, const uint8_t* vec_x /* count*n*32 */, const uint8_t* rand /* count*n*32 */,
                       uint8_t* transcripts /* count*216, in/out */, uint8_t* proofs /* count*(48*(3+6L)+32) */, uint8_t* challenges /* count*(1+L)*32, may be NULL */,
                       int* status /* count */);
/* The same two with the reference's `rng: &mut T` in place of the draws ("the reference's rng as a ChaCha12 state", below): item i draws
 * Fr::rand 2 n - 2 (IPA) or n (SameMSM) times from states[i] on the device — the stream cpx_rng_fr would give — and the 40-byte state comes
 * back advanced; the draws never leave the device.  A refused IPA item's state is advanced too: the reference had drawn before it panicked.
 * A state whose word_pos is within 2^32 words of 2^64 is CPX_ERR_ARG, as are more than 2^20 draws per stream or 2^26 per call. */
int cpx_ipa_prove_rng(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D,
                      const uint8_t* z, const uint8_t* vec_c, const uint8_t* vec_d, uint8_t* states /* count*40, in/out */, uint8_t* transcripts, uint8_t* proofs,
                      uint8_t* challenges, int* status);
int cpx_same_msm_prove_rng(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t,
                           const uint8_t* Z_u, const uint8_t* vec_x, uint8_t* states /* count*40, in/out */, uint8_t* transcripts, uint8_t* proofs,
                           uint8_t* challenges, int* status);
/* GrandProductProof::new (grand_product_argument.rs:43-166) for `count` independent stand-alone statements of ell factors and n_blinders
 * blinders each, n = ell + n_blinders = 2^L, the whole function in ONE call: step 1 of the transcript (B, gprod_result under "gprod_step1",
 * alpha under "gprod_alpha", :63-65), the prefix products vec_c (:69-73), C = <vec_c, G> + <vec_c_blinders, H> (:76), r_p (:79-81), step 2
 * (C, r_p under "gprod_step2", beta under "gprod_beta", :83-85), vec_d and D (:105-132), inner_prod (:141-142), and then everything
 * cpx_ipa_prove does (:152-163) on G | H, crs_U, C, D, inner_prod, vec_c | vec_c_blinders and vec_d | vec_d_blinders.  The rescaled basis
 * G' of :90-102 is never formed: its factors beta^-(i+1) seed the loop's fold coefficients and multiply the scalars of B_d.
 *   G, H         the bases (`crs_G_vec`, ell per item; `crs_H_vec`, n_blinders per item), affine
 *   crs_U, B     144-byte Jacobian points, any representative, Z = 0 for the identity
 *   gprod_result, vec_b, vec_b_blinders   the statement's scalar and the witness
 *   rand         per item the n_blinders + 2 n - 2 values the reference draws, in its order: vec_c_blinders [n_blinders] (:75), then those
 *                of generate_ipa_blinders: r [n], then z [n - 2] (inner_product_argument.rs:46-47)
 *   transcripts  in: the states before `new`; out: advanced by the whole `new`: gprod_step1, gprod_alpha, gprod_step2, gprod_beta, then
 *                everything cpx_ipa_prove appends
 *   proofs       the reference's `serialize` (:248-253): C compressed, r_p as a canonical little-endian scalar, then the InnerProductProof
 *                bytes exactly as cpx_ipa_prove writes them
 *   challenges   per item gprod alpha, gprod beta, ipa alpha, ipa beta, gamma_1..L (Montgomery limbs); may be NULL
 *   status       per item CPX_OK, or CPX_ERR_ARG where the reference panics: in generate_ipa_blinders on c = vec_c | vec_c_blinders and
 *                d = vec_d | vec_d_blinders (inner_product_argument.rs:69, :71), or where beta has no inverse (:86).  Such an item's proof
 *                bytes and challenges are zero and its transcript state is unchanged; the other items are unaffected.
 * Conventions of cpx_ipa_prove: scalars are Montgomery limbs and a value >= r anywhere is CPX_ERR_ARG for the call; the identity is a legal
 * base and a legal B; count = 0 is a no-op returning CPX_OK; ell = 0 is CPX_ERR_ARG (the reference's ell - 1 underflows, :71), n = 1 is
 * CPX_ERR_ARG (the IPA's n - 2), n not a power of two is CPX_ERR_NOT_POW2; n_blinders = 0 is legal, H and vec_b_blinders may then be NULL;
 * NULL with work to do and an invalid transcript state are CPX_ERR_ARG; the limits are those of one cpx_ipa_rounds on n elements (16384
 * items, count (2 n + 2) <= 2^24), checked before anything is read; on any return other than CPX_OK nothing is written, states included.
 * One upload, one download, ONE stream synchronisation; launches that depend on L only (curdleproofs_amd/csrc/gprod_plan.hpp, gprod.hip);
 * no CRS is needed and the loaded batch is untouched.  Scratch is the tier-0 set under the same call scope.  The _rng form draws the same
 * stream on the device from states[i], with the limits of cpx_ipa_prove_rng on n_blinders + 2 n - 2 draws; a refused item's stream has drawn
 * too.  Measurements: profiles/gprod.md. */
int cpx_gprod_prove(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G /* count*ell*96 */, const uint8_t* H /* count*n_blinders*96 */,
                    const uint8_t* crs_U, const uint8_t* B /* count*144 each */, const uint8_t* gprod_result /* count*32 */, const uint8_t* vec_b /* count*ell*32 */,
                    const uint8_t* vec_b_blinders /* count*n_blinders*32 */, const uint8_t* rand /* count*(n_blinders+2n-2)*32 */,
                    uint8_t* transcripts /* count*216, in/out */, uint8_t* proofs /* count*(48*(3+4L)+96) */, uint8_t* challenges /* count*(4+L)*32, may be NULL */,
                    int* status /* count */);
int cpx_gprod_prove_rng(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
                        const uint8_t* gprod_result, const uint8_t* vec_b, const uint8_t* vec_b_blinders, uint8_t* states /* count*40, in/out */, uint8_t* transcripts,
                        uint8_t* proofs, uint8_t* challenges, int* status);
/* GrandProductProof::verify (grand_product_argument.rs:180-246) for `count` independent stand-alone proofs given as the bytes
 * cpx_gprod_prove writes (:248-253), each against an MsmAccumulator of its own with the caller's two draws, in ONE call: gprod_step1,
 * alpha, gprod_step2 (the proof's C and r_p), beta (:201-210), vec_u and inner_prod from beta (:214-231),
 * D = B - beta^-1 crs_G_sum + alpha crs_H_sum (:223) — formed on the device, because ipa_step1 hashes its encoding — and then everything
 * cpx_ipa_verify does on G | H, crs_U, C, D.
 *   crs_G_sum, crs_H_sum   affine, taken from the caller and NOT recomputed, as in the reference: a wrong sum gives CPX_ERR_VERIFY.  They are
 *                multiplied by -beta^-1 and alpha the way cpx_g1_scale multiplies: by the endomorphism split, which holds on the order-r
 *                subgroup only.  Like the bases they are not checked for membership; sums of points outside the subgroup need the
 *                context option scale_any_point (the plain 255-bit chain), as cpx_g1_scale does.
 *   rand         two non-zero reduced factors per item            challenges   as cpx_gprod_prove returns them; may be NULL
 *   verdicts     per item CPX_OK, CPX_ERR_VERIFY, or CPX_ERR_DESERIALIZE where C or a point of the inner-product proof does not decode
 *                or lies outside the subgroup, or r_p, c_final or d_final >= r: that item's state is unchanged and its challenges are zero
 * Conventions of cpx_ipa_verify: scalars are Montgomery limbs and a value >= r is CPX_ERR_ARG for the call; the identity is a legal base
 * and a legal B; count = 0 is a no-op; ell = 0 is CPX_ERR_ARG; n = ell + n_blinders = 1 is a real check; n not a power of two is
 * CPX_ERR_NOT_POW2; n_blinders = 0 is legal, H may then be NULL (crs_H_sum is the identity: 96 zero bytes); the limits are those of
 * cpx_ipa_verify on n elements, checked before anything is read; nothing is written on any return other than CPX_OK.  One upload, one
 * download, ONE stream synchronisation; launches that do not depend on count; tier-0 scratch; no CRS, the loaded batch is untouched.
 * beta = 0 (:86, :210) cannot be reached by a test: get_and_append_challenge never returns zero; the prover's flag for it is defensive. */
int cpx_gprod_verify(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G /* count*ell*96 */, const uint8_t* H /* count*n_blinders*96 */,
                     const uint8_t* crs_U /* count*144 */, const uint8_t* crs_G_sum, const uint8_t* crs_H_sum /* count*96 each */, const uint8_t* B /* count*144 */,
                     const uint8_t* gprod_result /* count*32 */, const uint8_t* proofs /* count*(48*(3+4L)+96) */, const uint8_t* rand /* count*2*32 */,
                     uint8_t* transcripts /* count*216, in/out */, uint8_t* challenges /* count*(4+L)*32, may be NULL */, int* verdicts /* count */);
/* SamePermutationProof::new (same_permutation_argument.rs:40-99) for `count` independent stand-alone statements of ell elements and
 * n_blinders blinders each, n = ell + n_blinders = 2^L, the whole function in ONE call: step 1 of the transcript (A, M under
 * "same_perm_step1", then vec_a as ONE message under the same label — its u64 little-endian length, then the canonical scalars, 8 + 32 ell
 * bytes —, alpha under "same_perm_alpha", beta under "same_perm_beta", :60-63), the permuted factors a_sigma(i) + sigma(i) alpha + beta and
 * their product (:66-73), B = A + alpha M + beta sum G (:76) — formed literally for arbitrary A and M: one multi-scalar multiplication over
 * G and M, to which A is added —, vec_b_blinders = vec_a_blinders + alpha vec_m_blinders (:78-81), and then everything cpx_gprod_prove does
 * (:83-93) on B, the product, the factors and vec_b_blinders, which stay in device memory.
 *   G, H         the bases (`crs_G_vec`, ell per item; `crs_H_vec`, n_blinders per item), affine
 *   crs_U, A, M  144-byte Jacobian points, any representative, Z = 0 for the identity
 *   vec_a, vec_a_blinders, vec_m_blinders   the statement's scalars and the witness's blinders
 *   permutation  ell u32 values per item.  An entry >= ell is CPX_ERR_ARG for the call (the reference indexes out of bounds, util.rs:78),
 *                found before anything is uploaded or written.  Repeated entries are legal, as in the reference, which does not check
 *                bijectivity: such an item gets the reference's bytes, and the proof does not verify.
 *   rand         the draws of cpx_gprod_prove, in its order: this layer draws nothing
 *   transcripts  in: the states before `new`; out: advanced by the whole `new`
 *   proofs       the reference's `serialize` (:173-177): B compressed, then the grand-product proof bytes exactly as cpx_gprod_prove writes them
 *   challenges   per item same-perm alpha, beta, then the 4 + L of cpx_gprod_prove (Montgomery limbs); may be NULL
 *   status       as cpx_gprod_prove: CPX_OK, or CPX_ERR_ARG where the reference panics; such an item's proof bytes and challenges are zero
 *                and its transcript state is unchanged
 * Conventions of cpx_gprod_prove: a scalar >= r anywhere is CPX_ERR_ARG for the call; the identity is a legal base and a legal A or M;
 * count = 0 is a no-op; ell = 0 and n = 1 are CPX_ERR_ARG, n not a power of two is CPX_ERR_NOT_POW2; n_blinders = 0 is legal, H and the two
 * blinder vectors may then be NULL; the limits are those of cpx_gprod_prove, checked before anything is read; on any return other than
 * CPX_OK nothing is written, states included.  There is no further cap on ell: vec_a is converted and absorbed in pieces of 128 scalars
 * (curdleproofs_amd/csrc/same_perm_plan.hpp, same_perm.hip).  One upload, one download, ONE stream synchronisation; launches that depend on
 * L only; no CRS is needed and the loaded batch is untouched.  The _rng form draws cpx_gprod_prove_rng's stream; a refused item's stream has
 * drawn too.  Measurements: profiles/same_perm.md. */
int cpx_same_perm_prove(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G /* count*ell*96 */, const uint8_t* H /* count*n_blinders*96 */,
                        const uint8_t* crs_U, const uint8_t* A, const uint8_t* M /* count*144 each */, const uint8_t* vec_a /* count*ell*32 */,
                        const uint32_t* permutation /* count*ell */, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders /* count*n_blinders*32 each */,
                        const uint8_t* rand /* count*(n_blinders+2n-2)*32 */, uint8_t* transcripts /* count*216, in/out */,
                        uint8_t* proofs /* count*(48*(4+4L)+96) */, uint8_t* challenges /* count*(6+L)*32, may be NULL */, int* status /* count */);
int cpx_same_perm_prove_rng(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A,
                            const uint8_t* M, const uint8_t* vec_a, const uint32_t* permutation, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders,
                            uint8_t* states /* count*40, in/out */, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status);
/* SamePermutationProof::verify (same_permutation_argument.rs:112-171) for `count` independent stand-alone proofs given as the bytes
 * cpx_same_perm_prove writes (:173-177), each against an MsmAccumulator of its own with the caller's THREE draws, in draw order: the factor
 * of the same-permutation check (:149), then the two of the inner-product check.  In ONE call: step 1 as in the prover (:134-137),
 * gprod_result = prod (a_i + i alpha + beta) (:140-145), the relation beta <1, G> - (B - A - alpha M) == O (:149), which joins the item's
 * single multi-scalar multiplication — a_0 beta more on the weights of G_0..G_{ell-1}, and B, A, M behind the statement points of the item's
 * row with the weights -a_0, +a_0, +a_0 alpha —, and then everything cpx_gprod_verify does on the proof's B and gprod_result.
 *   crs_G_sum, crs_H_sum   the caller's, as in cpx_gprod_verify: a wrong sum gives CPX_ERR_VERIFY
 *   rand         three non-zero reduced factors per item         challenges   as cpx_same_perm_prove returns them; may be NULL
 *   verdicts     per item CPX_OK, CPX_ERR_VERIFY, or CPX_ERR_DESERIALIZE where B, C or a point of the inner-product proof does not decode
 *                or lies outside the subgroup, or a proof scalar is >= r: that item's state is unchanged and its challenges are zero.  A
 *                proof that deserialises advances its state by the whole `verify`, whatever the verdict.
 * Conventions of cpx_gprod_verify: count = 0 is a no-op; ell = 0 is CPX_ERR_ARG; n = 1 (ell = 1, n_blinders = 0) is a real check; n not a
 * power of two is CPX_ERR_NOT_POW2; a scalar of vec_a >= r is CPX_ERR_ARG; the limits are those of cpx_ipa_verify on n elements with three
 * more points per item; nothing is written on any return other than CPX_OK.  Launches that do not depend on count. */
int cpx_same_perm_verify(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G /* count*ell*96 */, const uint8_t* H /* count*n_blinders*96 */,
                         const uint8_t* crs_U /* count*144 */, const uint8_t* crs_G_sum, const uint8_t* crs_H_sum /* count*96 each */, const uint8_t* A,
                         const uint8_t* M /* count*144 each */, const uint8_t* vec_a /* count*ell*32 */, const uint8_t* proofs /* count*(48*(4+4L)+96) */,
                         const uint8_t* rand /* count*3*32 */, uint8_t* transcripts /* count*216, in/out */, uint8_t* challenges /* count*(6+L)*32, may be NULL */,
                         int* verdicts /* count */);
/* ark_ec `CurveGroup::normalize_batch` (+ optional `serialize_compressed`); either output may be NULL */
int cpx_g1_normalize(cpx_ctx* ctx, const uint8_t* jac /* n*144 */, size_t n, uint8_t* out_affine /* n*96 */, uint8_t* out_compressed /* n*48 */);
/* whisk.rs:318-320 `from_bytes_g1affine` = deserialize_compressed with on-curve + subgroup validation */
int cpx_g1_decompress(cpx_ctx* ctx, const uint8_t* compressed /* n*48 */, size_t n, uint8_t* out_affine /* n*96 */, int check_subgroup);

/* The same with one verdict per point instead of one for the call: status[i] = 0 ok (out_affine[i] valid), 1 malformed encoding or x
 * not on the curve, 2 on the curve but outside the order-r subgroup.  Returns CPX_OK whatever the verdicts are.  This is the
 * device square root behind a try-and-increment hash to the curve: tests/crs.rs:13-52 `generate_random_points` maps a hash to x and
 * keeps `get_point_from_x_unchecked(x, false)` when it exists (curdleproofs_amd/crs.py::generate_random_points). */
int cpx_g1_decompress_status(cpx_ctx* ctx, const uint8_t* compressed /* n*48 */, size_t n, uint8_t* out_affine /* n*96 */, int check_subgroup, uint8_t* status /* n */);

/* ---- tier 1: msm_accumulator.rs:22-68 `MsmAccumulator` -------------------------------------- */
typedef struct cpx_accum cpx_accum;
int cpx_accum_new(cpx_ctx* ctx, cpx_accum** out);
void cpx_accum_free(cpx_accum* acc);
/* `accumulate_check(&mut self, C, vec_x, vec_V, rng)`; the caller passes the `Fr::rand(rng)` value it drew: a uniform,
 * reduced, NON-ZERO field element (zero or >= r -> CPX_ERR_ARG: a zero factor would drop the check) */
int cpx_accum_check(cpx_accum* acc, const uint8_t C[144], const uint8_t* vec_x /* n*32 */, const uint8_t* vec_V /* n*96 */, size_t n,
                    const uint8_t random_factor[32]);
/* `verify(self)`: CPX_OK or CPX_ERR_VERIFY */
int cpx_accum_verify(cpx_accum* acc);

/* ---- tier 2: whole proofs, batched, instance data resident in HBM --------------------------- */
/* Uploads `batch` instances (vec_R, vec_S, vec_T, vec_U: batch*ell*96 each; M: batch*144 Jacobian):
 * the public inputs of curdleproofs.rs:59-70 / :197-207. */
int cpx_batch_load(cpx_ctx* ctx, size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U,
                   const uint8_t* M);
/* The same upload in two halves, for a caller that always has a next batch (a service draining a queue of shuffles): _begin starts moving the
 * NEXT batch's instance to a staging area in HBM on an upload stream of its own and returns at once — the batch loaded before stays loaded, and
 * cpx_batch_prove / cpx_batch_verify on it run beside the transfer; _end waits for the transfer (the host buffers, which must stay untouched
 * from _begin to _end, are free again when it returns) and makes the staged batch the loaded one (device-to-device, behind the context's last
 * kernel).  97 KB per proof at ell = 252 cross PCIe per instance: with cpx_batch_load in every pass the bench rate is 5 % lower, with
 * _begin before the prove and _end after the verify it is within 1 % (bench.py `value_incl_instance_upload`).  Page-locked buffers
 * (cpx_host_alloc) make the transfer asynchronous; pageable ones work, the copy then happens inside _begin.
 * _end without _begin, or a cpx_ctx_set_crs in between -> CPX_ERR_STATE. */
int cpx_batch_load_begin(cpx_ctx* ctx, size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U,
                         const uint8_t* M);
int cpx_batch_load_end(cpx_ctx* ctx);
/* curdleproofs.rs:59 `CurdleproofsProof::new` for every loaded instance.
 *   permutation  batch*ell u32          k  batch*32          vec_m_blinders  batch*4*32
 *   rand         batch*(3n+9)*32, n = ell+4: the `Fr::rand(rng)` draws in the reference's order —
 *                vec_a_blinders[2] (curdleproofs.rs:86), vec_c_blinders[4] (grand_product_argument.rs:75),
 *                IPA r[n], z[n-2] (inner_product_argument.rs:46-47), r_t, r_u (curdleproofs.rs:110-111),
 *                r_a, r_b, r_k (same_scalar_argument.rs:56-58), vec_r[n] (same_multiscalar_argument.rs:78)
 *   proofs_out   batch*cpx_proof_size() bytes = `CurdleproofsProof::serialize` (curdleproofs.rs:300-310)
 * The witness is taken to be CONSISTENT with the loaded instance: vec_T[j] = k vec_R[permutation[j]], vec_U[j] = k vec_S[permutation[j]]
 * (util.rs:94-95).  From option "device_min_batch" proofs on (option "rs_from_tables", default 1) the prover then takes k R = msm(vec_T,
 * a_sigma) and k S = msm(vec_U, a_sigma) from the per-proof tables and R, S, cm_T.T_2, cm_U.T_2, cm_A.T_2, cm_B.T_2 from those: the same
 * group elements, hence the reference's proof bytes.  For an INCONSISTENT witness the reference emits a proof that does not verify, and
 * this call emits another proof that does not verify; with "rs_from_tables" = 0 R and S are msm(vec_R, a), msm(vec_S, a) as the reference
 * computes them and the bytes are the reference's for every witness.  A batch in which some k is zero (the reference proves it: vec_T and
 * vec_U all identity) is proved that way as a whole, whatever the option. */
int cpx_batch_prove(cpx_ctx* ctx, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders, const uint8_t* rand,
                    uint8_t* proofs_out);
/* curdleproofs.rs:197 `verify` (after `deserialize`, :312-323) for every loaded instance.
 *   rand     batch*8*32: the eight `accumulate_check` factors (msm_accumulator.rs:44) in call order.  They must be
 *            independent uniform non-zero reduced field elements (what `Fr::rand` returns but for the zero it may
 *            return with probability 1/r); zero or >= r -> CPX_ERR_ARG.
 *   verdict  batch ints: CPX_OK, CPX_ERR_VERIFY or CPX_ERR_DESERIALIZE
 * One deliberate difference in HOW (not in what) is checked: the reference tests the four SameScalar relations
 * (same_scalar_argument.rs:127-137) as direct equalities; here they join the accumulated MSM with the weights
 * a1*a2, a3*a4, a5*a6, a7*a8 built from the caller's factors.  The accumulated sum is then a polynomial of total degree 2
 * in independent uniform factors whose coefficients are the individual check values, so a false relation survives with
 * probability <= 2/r (Schwartz-Zippel) — the same bound every other check of `MsmAccumulator` already rests on.  The
 * verdict therefore equals the reference's except with probability < 2^-253 over the caller's factors
 * (tests/test_gpu_parity.py::test_same_scalar_relations_are_checked isolates these relations).
 * Point encodings with the INFINITY FLAG set (context option "strict_infinity"): ark-bls12-381 ^0.4's `read_g1_compressed` — behind
 * `G1Affine::deserialize_compressed`, curdleproofs.rs:312-323, whisk.rs:313-320 — returns the identity as soon as the compression and
 * the infinity flag are set and looks at neither the sort flag nor the remaining 381 bits (ark-bls12-381 0.4.0 `curves/util.rs`, recalled:
 * the crate is not in the build image; version 0.5 rejects both).  strict_infinity = 0 (default) reproduces that: such an encoding IS the
 * identity — and is hashed in its canonical form 0xc0 || 0^47, as the reference hashes the deserialised point — so a proof carrying one
 * gets the verdict the reference gives it (normally CPX_ERR_VERIFY, not CPX_ERR_DESERIALIZE).  strict_infinity = 1: only 0xc0 || 0^47
 * is the identity, anything else with the flag set is CPX_ERR_DESERIALIZE (the zcash specification's wording).  The option also governs
 * cpx_g1_decompress / cpx_g1_decompress_status and the cpx_whisk_* entry points. */
int cpx_batch_verify(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand, int* verdict);
/* BASELINE config 5: the batched verifier.  Every `accumulate_check` of every loaded proof goes into
 * ONE accumulated MSM — the reference's `MsmAccumulator` (msm_accumulator.rs:22-68; `new` is pub(crate), :28, and
 * `CurdleproofsProof::verify` makes one per call, curdleproofs.rs:215) shared by all verify calls; the SameScalar
 * equalities (same_scalar_argument.rs:127-137) join it with their own random weights.
 *   rand         batch*12*32: per proof the eight `accumulate_check` factors, then four weights for the equalities
 *   partial_jac  144 B: this context's share  sum (lhs - rhs)  of the accumulated check (Jacobian, standard form).
 *                The batch is accepted iff the partial sums of all contexts / GPUs add up to the identity
 *                (all-gather the 144-byte partials, add them with cpx_g1_sum_jac) and no context reports invalid proofs.
 *   n_invalid    number of loaded proofs that failed deserialisation or the structural checks (curdleproofs.rs:218)
 * All-or-nothing: a rejected batch does not say which proof is wrong (cpx_batch_verify_grouped below names the wrong proofs at close to this
 * call's cost). */
int cpx_batch_verify_fused(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand, uint8_t* partial_jac, int* n_invalid);
/* curdleproofs.rs:197 `verify` for every loaded instance, one verdict per proof, through the grouped form of the accumulated check
 * (msm_accumulator.rs:22-68 shared by the proofs of a group).
 *   rand         batch*12*32, as for cpx_batch_verify_fused (zero or >= r -> CPX_ERR_ARG)
 *   verdict      batch ints: CPX_OK, CPX_ERR_VERIFY or CPX_ERR_DESERIALIZE; the call returns CPX_OK whatever they are
 *   n_rechecked  (may be NULL) the number of proofs that went through stage 2; deterministic given the inputs and the option below
 * The batch is cut into NT groups of G consecutive proofs, G = ceil(batch / locate_groups_max), NT = ceil(batch / G); the last group may be
 * short.  Context option "locate_groups_max" (default 256, 1 .. 256) concerns the grouped calls only: cpx_batch_verify_fused keeps its 256
 * groups.  Results never depend on it, only n_rechecked and speed do.
 *   Stage 1  every group's accumulated sum — the fused check restricted to that group — is computed and tested for the identity.
 *   Stage 2  every flag-free proof of a group whose sum is not the identity gets its own accumulated check, from the scalars stage 1
 *            computed (nothing is hashed or decoded again).  With G = 1 stage 1 already is that check and there is no stage 2.
 * Verdicts: a proof that does not decode is CPX_ERR_DESERIALIZE; one with the structural flag (vec_T[0] is zero, curdleproofs.rs:218) is
 * CPX_ERR_VERIFY; a flag-free proof of a passing group is CPX_OK; any other proof has the verdict of its own check.  An undecodable proof
 * contributes nothing to its group, so it does not send its neighbours to stage 2.  A structurally rejected proof keeps its scalars (as in
 * the fused call) and therefore DOES drag its group into stage 2: its neighbours are rechecked and counted in n_rechecked.
 * Soundness.  A group's sum is a polynomial of total degree 2 in the independent factors of its proofs whose coefficients are the individual
 * check values, so a group that contains a false relation passes stage 1 with probability <= 2/r — the bound cpx_batch_verify already rests
 * on (Schwartz-Zippel).  Stage 2 reuses a proof's own 12 factors: a valid proof's check is identically zero, an invalid one survives with
 * probability <= 2/r over its own factors.  The per-proof verdicts therefore equal cpx_batch_verify's except with probability < 2^-252.
 * strict_infinity applies as for cpx_batch_verify.  Without a loaded batch: CPX_ERR_STATE.  NULL proofs, rand or verdict: CPX_ERR_ARG and
 * nothing is written.  What the call costs beside the other two is measured by scripts/grouped_verify_rate.py (profiles/grouped_verify.md). */
int cpx_batch_verify_grouped(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand /* batch*12*32, as cpx_batch_verify_fused */,
                             int* verdict /* batch: CPX_OK / CPX_ERR_VERIFY / CPX_ERR_DESERIALIZE */, size_t* n_rechecked /* may be NULL */);
/* sum of n Jacobian points (n*144 B) -> out (144 B); *is_identity = 1 iff the sum is the point at infinity */
int cpx_g1_sum_jac(cpx_ctx* ctx, const uint8_t* points_jac, size_t n, uint8_t* out_jac, int* is_identity);

/* ---- Whisk byte-level API: whisk.rs (the reference's `pub fn`s, source-compatible at the byte level) ------------------
 * A tracker is 96 bytes: r_G (48, compressed) || k_r_G (48)  (`WhiskTracker`, whisk.rs:36-42).  ell is the CRS's ell
 * (the reference hard-codes N = 128, ell = 124, whisk.rs:27-28; any power-of-two ell + 4 works here).  A bad point or
 * scalar encoding anywhere is the reference's `Err(SerializationError)` -> CPX_ERR_DESERIALIZE.  The RNG stays with the
 * caller: every draw the reference makes from `rng` is an argument, in the reference's order.  (A caller whose rng is a ChaCha12Rng can
 * hand over its state instead and have the draws made on the device: the cpx_rng_* and *_rng calls further down.) */
/* whisk.rs:144-179 `generate_whisk_shuffle_proof(rng, crs, pre_trackers)`.
 *   permutation     ell u32: `(0..ELL).collect().shuffle(rng)` (:152-155)      k  `Fr::rand(rng)` (:156)
 *   vec_m_blinders  4*32: `generate_blinders(rng, N_BLINDERS)` inside shuffle_permute_and_commit_input (util.rs:91)
 *   rand            (3n+9)*32: the draws of `CurdleproofsProof::new` (see cpx_batch_prove)
 *   post_trackers_out  ell*96       proof_out  48 + cpx_proof_size() = M || CurdleproofsProof::serialize (4496 B at ell = 124)
 * Replaces the batch loaded into ctx (it loads the one instance it proves). */
int cpx_whisk_generate_shuffle_proof(cpx_ctx* ctx, const uint8_t* pre_trackers /* ell*96 */, const uint32_t* permutation, const uint8_t k[32],
                                     const uint8_t* vec_m_blinders, const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proof_out);
/* whisk.rs:106-130 `is_valid_whisk_shuffle_proof(rng, crs, pre_trackers, post_trackers, proof_bytes)`;
 *   rand 8*32: the verifier's `accumulate_check` factors (see cpx_batch_verify).  *valid = 1 / 0 = Ok(true) / Ok(false). */
int cpx_whisk_is_valid_shuffle_proof(cpx_ctx* ctx, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proof, const uint8_t* rand,
                                     int* valid);
/* whisk.rs:228-263 `generate_whisk_tracker_proof(rng, tracker, k)`; blinder = its one `Fr::rand(rng)` (:238).
 *   proof_out 128 B = A (48) || B (48) || s (32 LE)  (`TrackerProof`, whisk.rs:69-73) */
int cpx_whisk_generate_tracker_proof(cpx_ctx* ctx, const uint8_t tracker[96], const uint8_t k[32], const uint8_t blinder[32], uint8_t proof_out[128]);
/* whisk.rs:183-226 `is_valid_whisk_tracker_proof(tracker, k_commitment, tracker_proof)` */
int cpx_whisk_is_valid_tracker_proof(cpx_ctx* ctx, const uint8_t tracker[96], const uint8_t k_commitment[48], const uint8_t proof[128], int* valid);
/* The two tracker-proof functions for `count` independent items per call: a constant number of kernel launches and ONE stream
 * synchronisation whatever the count (the single calls above cost several synchronisations per proof).  Scalars as above: k and
 * blinders are 32-byte Montgomery limbs, s inside a proof is 32 bytes little-endian canonical.  Both return CPX_OK whatever the
 * per-item results are (the convention of cpx_batch_verify and cpx_g1_decompress_status); NULL pointers with count > 0 are CPX_ERR_ARG,
 * count = 0 is a no-op.  Neither needs a CRS, neither touches the loaded batch (cpx_batch_size is unchanged).  At most 2^23 items per call. */
/* whisk.rs:228-263 `generate_whisk_tracker_proof` for `count` independent (tracker, k, blinder) triples.
 *   status[i]: CPX_OK, or CPX_ERR_DESERIALIZE (undecodable tracker; proofs_out[i] is then 128 zero bytes). */
int cpx_whisk_generate_tracker_proofs(cpx_ctx* ctx, size_t count, const uint8_t* trackers /* count*96 */, const uint8_t* k /* count*32 */,
                                      const uint8_t* blinders /* count*32 */, uint8_t* proofs_out /* count*128 */, int* status /* count */);
/* whisk.rs:183-226 `is_valid_whisk_tracker_proof` for `count` independent (tracker, k_commitment, proof) triples.
 *   verdict[i]: CPX_OK = Ok(true), CPX_ERR_VERIFY = Ok(false), CPX_ERR_DESERIALIZE = Err(SerializationError). */
int cpx_whisk_verify_tracker_proofs(cpx_ctx* ctx, size_t count, const uint8_t* trackers /* count*96 */, const uint8_t* k_commitments /* count*48 */,
                                    const uint8_t* proofs /* count*128 */, int* verdict /* count */);
/* whisk.rs:183-226 for `count` triples as ONE multi-scalar multiplication: the fused and the grouped form of the call above, as
 * cpx_batch_verify_fused / cpx_batch_verify_grouped are of cpx_batch_verify.  rand holds two weights per item, a_i then b_i, Montgomery limbs
 * as every scalar of this header; they must be independent, uniform, non-zero and reduced — a zero or a value >= r anywhere is CPX_ERR_ARG for
 * the call before anything is written (the rule of cpx_batch_verify).  With c_i the challenge of whisk.rs:205-220 and s_i the proof's response,
 * item i stands for
 *     a_i (s_i G + c_i k_G_i - A_i) + b_i (s_i r_G_i + c_i k_r_G_i - B_i)
 * and a group of items is one MSM: the generator with sum a_i s_i, and per item k_G (a c), A (-a), r_G (b s), k_r_G (b c), B (-b) — 5 points
 * per item on the radix-256 endomorphism bucket path of cpx_g1_msm_many instead of two 129-step ladders (layout and scalar rules in
 * curdleproofs_amd/csrc/tracker_check_plan.hpp).  SOUNDNESS: the sum is linear in the independent factors, so a group that contains a false
 * relation sums to the identity with probability <= 1 / r over the caller's draws; weights an adversary can predict or influence void that.
 * An item is FLAGGED when a point does not decode or lies outside the subgroup, or s >= r (option "strict_infinity" governs infinity encodings
 * as in the per-item call).  A flagged item contributes nothing to any sum.
 * Conventions of the batched tracker calls: count = 0 is a no-op returning CPX_OK; NULL with work to do is CPX_ERR_ARG and nothing is written;
 * no CRS is needed and the loaded batch is untouched; the number of kernel launches does not depend on count.  At most 2^21 items per call
 * (5 count + 256 points within the 2^24 of cpx_g1_msm_many); more is CPX_ERR_ARG before anything is read.  Scratch is the tier-0 set and is
 * trimmed on every exit path: "tier0_scratch_bytes" stays within 35 buffers x 64 MiB afterwards (23 of the tier-0 set, 12 of the shuffle set).  Measurements: profiles/tracker_proofs_grouped.md. */
/* Fused: partial_jac = the sum over all unflagged items (Jacobian, standard form; Z = 0 for the identity), *n_invalid = the flagged items.  The
 * batch is accepted iff n_invalid == 0 and the partials of all calls / contexts / GPUs — these and those of cpx_batch_verify_fused — add up to
 * the identity (cpx_g1_sum_jac).  count = 0: the identity and n_invalid = 0 (both outputs are always required).  ONE stream synchronisation. */
int cpx_whisk_verify_tracker_proofs_fused(cpx_ctx* ctx, size_t count, const uint8_t* trackers /* count*96 */, const uint8_t* k_commitments /* count*48 */,
                                          const uint8_t* proofs /* count*128 */, const uint8_t* rand /* count*2*32 */, uint8_t partial_jac[144], int* n_invalid);
/* Grouped: the items are cut into groups exactly as cpx_batch_verify_grouped cuts proofs (option "locate_groups_max", decode flag only).  Stage 1
 * tests every group's sum for the identity; stage 2 runs only when a group fails: every unflagged item of a failing group gets the per-item
 * relations of cpx_whisk_verify_tracker_proofs.  verdict[i]: CPX_OK, CPX_ERR_VERIFY, or CPX_ERR_DESERIALIZE for a flagged item; pre-filled with
 * CPX_ERR_INTERNAL; the call returns CPX_OK whatever the items say.  *n_rechecked (may be NULL) = the items stage 2 looked at, deterministic given
 * the inputs and the option.  With one item per group (count <= locate_groups_max) stage 1 is the per-item check and there is no stage 2.  ONE
 * stream synchronisation when every group passes, two when stage 2 runs. */
int cpx_whisk_verify_tracker_proofs_grouped(cpx_ctx* ctx, size_t count, const uint8_t* trackers /* count*96 */, const uint8_t* k_commitments /* count*48 */,
                                            const uint8_t* proofs /* count*128 */, const uint8_t* rand /* count*2*32 */, int* verdict /* count */,
                                            size_t* n_rechecked /* may be NULL */);

/* What the batched tracker calls consume, made `count` per call.  Every point below is a multiple of the BLS12-381 G1 generator G — r G, k G and
 * k (r G) = (k r mod r_order) G — and comes from a fixed-base table of G (curdleproofs_amd/csrc/gen_table.hpp: radix 256 over the endomorphism
 * split, 225 KB, at most 32 mixed additions per scalar and no doubling) that a context builds on the device at its first such call.  Conventions
 * of the batched tracker calls: scalars are 32-byte Montgomery limbs; count = 0 is a no-op returning CPX_OK; a NULL input with count > 0 is
 * CPX_ERR_ARG and nothing is written; at most 2^23 items per call; no CRS is needed and the loaded batch is untouched (cpx_batch_size is
 * unchanged); a call costs a constant number of kernel launches and ONE stream synchronisation whatever the count.  A zero scalar gives the
 * identity: 96 zero bytes affine, 0xc0 || 0^47 compressed.  A scalar whose limbs are not a reduced field element (>= r) is NOT rejected: as with
 * the k of cpx_whisk_generate_tracker_proofs, the limbs are taken for the Montgomery form they are and stand for limbs / 2^256 mod r. */
/* out[i] = scalars[i] * G for the BLS12-381 G1 generator (whisk.rs:318,323 with g1 = generator). Either output may be NULL. */
int cpx_g1_generator_mul(cpx_ctx* ctx, size_t count, const uint8_t* scalars /* count*32 */, uint8_t* out_affine /* count*96 */,
                         uint8_t* out_compressed /* count*48 */);
/* whisk.rs:45-55 WhiskTracker::from_k_r and whisk.rs:370 get_k_commitment for `count` (k, r) pairs.
 * trackers_out[i] = r_i G || k_i r_i G (compressed); k_commitments_out[i] = k_i G; either may be NULL. */
int cpx_whisk_trackers_from_k_r(cpx_ctx* ctx, size_t count, const uint8_t* k /* count*32 */, const uint8_t* r /* count*32 */,
                                uint8_t* trackers_out /* count*96 */, uint8_t* k_commitments_out /* count*48 */);

/* Which trackers belong to a set of keys: the defining relation of a tracker, k * r_G == k_r_G, tested for every (tracker, key) pair in one call.
 * A validator tests the shuffled trackers against its k; an operator tests them against all of its keys — n_trackers * n_keys independent scalar
 * multiplications.  With fewer than option "find_table_min_keys" keys (default 256) every pair is one element of the scalar-multiplication kernel
 * (k_smul) and one kernel compares; from that many keys on the trackers are processed in chunks: per chunk a table of the multiples
 * m * 256^w * r_G (m = 1..128, 32 windows, 0.56 MiB per tracker; a chunk's table and build scratch stay within option "find_table_mb", default
 * 1024 MiB) is built on the device and scanned with at most 32 mixed additions per pair, no doubling and no inversion (k_find_scan; plan in
 * curdleproofs_amd/csrc/find_plan.hpp, measurements in profiles/find_trackers.md).  The answers do not depend on the path.
 *   owner[i]   the smallest j with k_j * r_G_i == k_r_G_i, or CPX_NO_OWNER if no key opens tracker i
 *   status[i]  CPX_OK, or CPX_ERR_DESERIALIZE when either half does not decode (on the curve, in the subgroup, option "strict_infinity" governing
 *              infinity encodings as in the tracker calls); such a tracker has owner[i] = CPX_NO_OWNER
 * Two consequences of the relation: a tracker whose r_G is the identity is opened by EVERY key iff its k_r_G is the identity too (its owner is then 0,
 * provided n_keys > 0), and of duplicate keys the smaller index is reported.  Conventions of the batched tracker calls: CPX_OK whatever the items say;
 * status is pre-filled with CPX_ERR_INTERNAL and owner with CPX_NO_OWNER; n_trackers = 0 is a no-op; with n_keys = 0 the trackers are still decoded and
 * none has an owner (k may then be NULL); a NULL pointer with work to do is CPX_ERR_ARG and nothing is written; no CRS is needed and the loaded batch is
 * untouched.  Keys are 32-byte Montgomery limbs; limbs >= r are NOT rejected and stand for limbs / 2^256 mod r, as k does in the other calls.
 * Limits: n_trackers <= 2^23, n_keys <= 2^20, n_trackers * n_keys <= 2^32; beyond them the call is CPX_ERR_ARG before anything is read.  The ladder
 * path holds all n_trackers * n_keys products (96 B each) on the device.  ONE stream synchronisation per call; the number of kernel launches depends
 * on the number of table chunks only, never on n_keys. */
#define CPX_NO_OWNER 0xffffffffu
/* whisk.rs:36-55 (a tracker is r_G || k_r_G with k_r_G = k * r_G) and whisk.rs:323 for every (tracker, key) pair */
int cpx_whisk_find_trackers(cpx_ctx* ctx, size_t n_trackers, const uint8_t* trackers /* n_trackers*96 */,
                            size_t n_keys, const uint8_t* k /* n_keys*32, Montgomery limbs */,
                            uint32_t* owner /* n_trackers */, int* status /* n_trackers */);

/* The shuffle half of the byte-level API for `count` independent shuffles per call: compressed bytes in, compressed bytes out, and between
 * the uploads and the downloads every step runs on the device in a number of kernel launches that does not depend on count — decoding, the
 * scalar multiplications, the permutation, M (the fixed-base CRS table), normalisation and compression; the proving and verifying is
 * cpx_batch_prove / cpx_batch_verify on the count instances, which become the loaded batch (cpx_batch_size == count).  Conventions of the batched
 * tracker calls: CPX_OK whatever the per-item results are, count = 0 is a no-op, NULL pointers with count > 0 are CPX_ERR_ARG and nothing is
 * written, no CRS is CPX_ERR_STATE; status / verdict are pre-filled with CPX_ERR_INTERNAL.  A row of `permutation` that is not a permutation of
 * 0..ell makes the whole call CPX_ERR_ARG before anything is launched (the loaded batch stays).  Options "strict_infinity" and
 * "scale_any_point" govern these calls as they govern the single ones.  An item whose points do not decode keeps its slot of the batch as a
 * placeholder instance (every point the generator); the other items are not affected.  count * ell < 2^28 per call; beyond that what
 * cpx_batch_load accepts at this ell. */
/* util.rs:83-106 shuffle_permute_and_commit_input for `count` instances, device-resident:
 * T_i = permute(k_i * R_i), U_i = permute(k_i * S_i), M_i = msm(vec_G, sigma_i) + msm(vec_H, blinders_i).
 * The count instances (R, S, T, U, M) become the loaded batch (cpx_batch_size == count).  Either output may be NULL. */
int cpx_batch_shuffle(cpx_ctx* ctx, size_t count, const uint8_t* vec_R /* count*ell*96 */, const uint8_t* vec_S, const uint32_t* permutation /* count*ell */,
                      const uint8_t* k /* count*32 */, const uint8_t* vec_m_blinders /* count*4*32 */, uint8_t* vec_T_out /* count*ell*96 */,
                      uint8_t* vec_U_out, uint8_t* M_out /* count*144 */);
/* whisk.rs:144-179 generate_whisk_shuffle_proof for `count` independent shuffles.
 *   status[i]: CPX_OK, or CPX_ERR_DESERIALIZE (an undecodable pre tracker; the item's post trackers and proof are then zero bytes). */
int cpx_whisk_generate_shuffle_proofs(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers /* count*ell*96 */, const uint32_t* permutation /* count*ell */,
                                      const uint8_t* k /* count*32 */, const uint8_t* vec_m_blinders /* count*4*32 */, const uint8_t* rand /* count*(3n+9)*32 */,
                                      uint8_t* post_trackers_out /* count*ell*96 */, uint8_t* proofs_out /* count*(48+cpx_proof_size) */, int* status /* count */);
/* whisk.rs:106-130 is_valid_whisk_shuffle_proof for `count` independent (pre, post, proof) triples.
 *   verdict[i]: CPX_OK = Ok(true), CPX_ERR_VERIFY = Ok(false), CPX_ERR_DESERIALIZE = Err (an undecodable tracker on either side, an
 *   undecodable M, a failed CurdleproofsProof::deserialize).  rand as for cpx_batch_verify (zero or >= r -> CPX_ERR_ARG for the call). */
int cpx_whisk_verify_shuffle_proofs(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers,
                                    const uint8_t* proofs /* count*(48+cpx_proof_size) */, const uint8_t* rand /* count*8*32 */, int* verdict /* count */);
/* whisk.rs:106-130 for `count` triples: cpx_whisk_verify_shuffle_proofs with 12 factors per item and the grouped check behind it
 * (cpx_batch_verify_grouped: stages, verdicts, soundness, option "locate_groups_max").  Everything else is cpx_whisk_verify_shuffle_proofs:
 * verdict is pre-filled with CPX_ERR_INTERNAL, an item whose trackers or M do not decode keeps its slot as a placeholder instance and is
 * CPX_ERR_DESERIALIZE whatever the placeholder's verdict (the placeholder fails its group's sum, so the items beside it are rechecked and
 * counted).  n_rechecked may be NULL. */
int cpx_whisk_verify_shuffle_proofs_grouped(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers,
                                            const uint8_t* proofs, const uint8_t* rand /* count*12*32 */, int* verdict, size_t* n_rechecked);

/* ---- a run of shuffles against a resident candidate list ----------------------------------------------------------
 * A node holds ONE list of candidate trackers; every block's shuffle reads the trackers at ell indices of it and the shuffled trackers go
 * back to the same indices.  The list lives in the context, decoded once; a run of such blocks is verified in one call that uploads and
 * decodes the post side only.  Trackers are 96 bytes (r_G then k_r_G, compressed) as in the calls above, whose conventions hold: CPX_OK
 * whatever the per-item results, count = 0 is a no-op, NULL data pointers with count > 0 are CPX_ERR_ARG (checked before the context is
 * looked at), verdict is pre-filled with CPX_ERR_INTERNAL. */
/* Loads n <= 2^24 candidates, replacing any earlier list (n = 0 drops it).  The 2n points are decoded on the device, subgroup-checked,
 * under option "strict_infinity"; the context keeps the decoded points, a status per point and the bytes exactly as given.
 *   status (may be NULL) [i]: the code of cpx_g1_decompress_status for r_G if that is non-zero, else the one for k_r_G.
 * An undecodable candidate is no error of the load: it makes every item that reads it CPX_ERR_DESERIALIZE (the reference fails in
 * unzip_trackers only, whisk.rs:106-130).  The list survives cpx_ctx_set_crs, batch loads and every other call, and goes with the context. */
int cpx_whisk_candidates_load(cpx_ctx* ctx, size_t n, const uint8_t* trackers /* n*96 */, uint8_t* status /* n, may be NULL */);
/* the length of the resident list (0: none) */
size_t cpx_whisk_candidates_size(cpx_ctx* ctx);
/* The bytes of candidates first .. first+count-1, verbatim: as loaded, or as the post trackers of an applied item spelt them.  A range
 * outside the list is CPX_ERR_ARG. */
int cpx_whisk_candidates_read(cpx_ctx* ctx, size_t first, size_t count, uint8_t* trackers_out /* count*96 */);
/* whisk.rs:106-130 is_valid_whisk_shuffle_proof for a run of `count` items over the resident list.
 *   Item b's pre tracker j is candidate indices[b][j] of the list AS IT STANDS AFTER ITEMS 0..b-1 HAVE ALL BEEN WRITTEN BACK, whatever their
 *   verdicts.  Writing item b back is list[indices[b][j]] = post[b][j] for j = 0..ell-1 in that order: an index may repeat inside an item,
 *   the item then reads the same tracker twice and the highest slot wins the write.
 *   verdict[b]: exactly what cpx_whisk_verify_shuffle_proofs returns for that explicit (pre, post, proof, rand), the same three codes.
 *   *n_applied: the number of leading items with CPX_OK.  Those items, and no others, are written back to the resident list.  The verdicts
 *   behind the first failure stay defined by the as-if list above, NOT by the list the call leaves: they say what each later item would be
 *   worth had every earlier one been applied.  n_applied == NULL is a dry run: verdicts only, the list stays as it was.
 * An index >= cpx_whisk_candidates_size is CPX_ERR_ARG before anything is launched.  No list or no CRS is CPX_ERR_STATE, and so is a
 * "strict_infinity" value other than the one the list was loaded under.  Any return other than CPX_OK leaves the list untouched: the
 * write-back is the call's last step.  The count instances become the loaded batch, as with cpx_whisk_verify_shuffle_proofs; count * ell
 * < 2^28 per call as there. */
int cpx_whisk_verify_shuffle_run(cpx_ctx* ctx, size_t count, const uint32_t* indices /* count*ell */, const uint8_t* post_trackers /* count*ell*96 */,
                                 const uint8_t* proofs /* count*(48+cpx_proof_size) */, const uint8_t* rand /* count*8*32 */, int* verdict /* count */,
                                 size_t* n_applied /* may be NULL */);
/* whisk.rs:106-130 for a run: cpx_whisk_verify_shuffle_run with 12 factors per item and the grouped check behind it, as
 * cpx_whisk_verify_shuffle_proofs_grouped sits on cpx_whisk_verify_shuffle_proofs.  n_rechecked may be NULL. */
int cpx_whisk_verify_shuffle_run_grouped(cpx_ctx* ctx, size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs,
                                         const uint8_t* rand /* count*12*32 */, int* verdict, size_t* n_applied /* may be NULL */, size_t* n_rechecked);

/* ---- the reference's `rng: &mut T` as a ChaCha12 state, the draws made on the device ------------------------------
 * Every proving function of the reference takes `rng: &mut T`; its tests and README use `StdRng::seed_from_u64(0)` (rand 0.8: StdRng =
 * ChaCha12Rng).  The calls above keep the RNG with the caller and take every draw as an argument.  The calls below take the STATE of a
 * ChaCha12Rng instead, make the draws on the device word for word as the reference makes them (curdleproofs_amd/csrc/rng.hpp: the block
 * function, the word stream, Fr::rand's rejection sampling, rand 0.8's SliceRandom::shuffle with UniformInt<u32>::sample_single; kernel
 * k_rng_draw), consume them where they lie and return the advanced state: a service hands over a seed as it would hand the crate an rng and
 * gets the crate's bytes back (whisk.rs:416-456 from the number 0 alone: tests/test_gpu_rng.py).  The explicit-draw calls stay the route for
 * callers with an RNG of their own.
 *   state   40 bytes per stream: key[32] || word_pos (u64 little-endian) = ChaCha12Rng::get_seed() and the low 64 bits of get_word_pos();
 *           on return set_word_pos(word_pos) continues the Rust object where the library stopped.  A state whose word_pos is >= 2^64 - 2^32 is
 *           CPX_ERR_ARG for the call, before anything else is read.  `states` arguments are in/out, count x 40 bytes, and are written only
 *           when the call returns CPX_OK.
 * SECRECY AND REUSE.  A state is the prover's secret randomness.  Two streams with IDENTICAL states draw identical permutations, k and
 * blinders: the witnesses repeat and zero knowledge is gone.  Never pass one state twice, and never copy one state into several slots of a
 * call: derive the `count` states of a batch from one parent with cpx_rng_split, which advances the parent.
 * Word consumption as recalled from rand_core 0.6 / rand_chacha 0.3 (the crates are not in the build image; the infinity-flag note of
 * cpx_batch_verify is written the same way): BlockRng::next_u32 takes one word of the stream, next_u64 two (low word first, also across a
 * block boundary), fill_bytes of 32 bytes eight; SeedableRng::from_rng fills the 32-byte seed with fill_bytes; seed_from_u64 expands the
 * u64 with PCG32 into the key.  The two known-answer tests of whisk.rs pin all of it but from_rng, which nothing in the reference calls.
 * Conventions of the batched tracker calls: count = 0 is a no-op returning CPX_OK; NULL with work to do is CPX_ERR_ARG and nothing is
 * written. */
/* StdRng::seed_from_u64(seed).  Host only: no context, no GPU. */
int cpx_rng_from_u64(uint64_t seed, uint8_t state_out[40]);
/* `count` times ChaCha12Rng::from_rng(&mut parent): child i's key is the parent's next eight words, its word_pos 0; the parent is advanced by
 * 8 * count words.  THE way to get the states of a batch from one stream.  Host only.  At most 2^28 children per call. */
int cpx_rng_split(uint8_t parent[40] /* in/out */, size_t count, uint8_t* states_out /* count*40 */);
/* Fr::rand(rng) n_each times per stream, Montgomery limbs as every scalar argument of this header: the verifier's 8 / 12 factors per proof,
 * tracker blinders, the k and r of WhiskTracker::from_rand.  Needs no CRS, leaves the loaded batch untouched.  count <= 2^23, n_each <= 2^20,
 * count * n_each <= 2^26; n_each = 0 is a no-op. */
int cpx_rng_fr(cpx_ctx* ctx, size_t count, uint8_t* states /* count*40, in/out */, size_t n_each, uint8_t* out /* count*n_each*32 */);
/* The draws of ONE whisk.rs:144-179 generate_whisk_shuffle_proof per stream at the context's ell, in the reference's order — the shuffle of
 * 0..ell (:152-155), k (:156), the 4 blinders (util.rs:91), the 3n + 9 of CurdleproofsProof::new — downloaded: the bridge to the explicit-draw
 * calls (feed them to cpx_whisk_generate_shuffle_proofs and get what the _rng call gives).  Any output may be NULL; the states advance by the
 * whole set whatever is downloaded.  Needs a CRS (for ell: CPX_ERR_STATE without), leaves the loaded batch untouched.  ell <= 12288. */
int cpx_rng_shuffle_draws(cpx_ctx* ctx, size_t count, uint8_t* states /* count*40, in/out */, uint32_t* permutation_out /* count*ell */,
                          uint8_t* k_out /* count*32 */, uint8_t* blinders_out /* count*4*32 */, uint8_t* rand_out /* count*(3n+9)*32 */);
/* cpx_whisk_generate_shuffle_proofs with the draws of item i made on the device from states[i].  From option "device_min_batch" items on no
 * draw crosses the bus in either direction: 40 bytes of randomness go up per proof instead of (3n + 9 + 5) * 32 + 4 ell.  Below it the draws
 * are downloaded and the explicit-draw call runs; the bytes are the same.  The reference returns Err from unzip_trackers AFTER it has drawn
 * the permutation and k and BEFORE the blinders (whisk.rs:150-157): an item with status CPX_ERR_DESERIALIZE gets its state back advanced by
 * those two draws only, every other item by the full set. */
int cpx_whisk_generate_shuffle_proofs_rng(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers /* count*ell*96 */, uint8_t* states /* count*40, in/out */,
                                          uint8_t* post_trackers_out /* count*ell*96 */, uint8_t* proofs_out /* count*(48+cpx_proof_size) */, int* status /* count */);
/* cpx_batch_prove on the loaded instances with `rand` replaced by one state per instance: only the 3n + 9 draws of CurdleproofsProof::new
 * are taken from each stream; the witnesses stay arguments — and are taken to be consistent with the instance, as cpx_batch_prove says
 * (option "rs_from_tables"; 0 gives the reference's bytes for every witness).  (cpx_whisk_generate_shuffle_proofs_rng, whose witnesses
 * never leave the device, keeps the reference's evaluation order: there k cannot be looked at without a synchronisation.) */
int cpx_batch_prove_rng(cpx_ctx* ctx, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders, uint8_t* states /* batch*40, in/out */,
                        uint8_t* proofs_out);

/* ---- group elements from a state: G1Projective::rand, generate_crs, the README's instance draws ---------------------
 * `G1Projective::rand(rng)` (ark-ec 0.4 / ark-ff 0.4, recalled as the word consumption above is; pinned through the oracle by the KAT of
 * whisk.rs:416-456, whose CRS and trackers are made of these draws) reads the word stream as a sequence of TOKENS:
 *   candidate  twelve words = six next_u64, low word first: the twelve 32-bit limbs of an Fp, least significant first; the top word is
 *              masked with 0x1fffffff (381 bits).  A value >= p is rejected: nothing else is drawn and the next candidate starts twelve
 *              words on (about 19 % are: p / 2^381 = 0.8126).  Otherwise the limbs ARE the Montgomery form of x (R = 2^384).
 *   bool       an accepted candidate is followed by ONE word whose top bit is `greatest` (rand's Standard for bool); the next candidate
 *              starts thirteen words on, whether or not x gives a point.
 *   point      if x^3 + 4 is a square, y is the root whose canonical integer is the larger of (y, p - y) when `greatest`, else the smaller,
 *              and the draw is [h](x, y) as an affine point, h = 0x396c8c005555e1568c00aaab0000aaab the full cofactor; the stream stands
 *              behind the bool.  Otherwise the loop goes on with the next candidate.  x = 0 gives (0, +-2), of order 3: the identity.
 * Where a token ends depends on the compare with p alone, whether it yields a point on a square root: the library walks the tokens of a
 * stream in one wave (k_rng_g1_scan) and takes the roots of all candidates of all streams in parallel (k_rng_g1_sqrt), keeps per stream
 * the first n_each hits (k_rng_g1_select) and multiplies those by h (k_clear_cofactor); a stream that comes out short takes another
 * round (curdleproofs_amd/csrc/rng_g1_plan.hpp; option "rng_g1_round_cap", read-only "rng_g1_last_rounds").
 * Conventions are those of cpx_rng_fr: count = 0 or n_each = 0 is a no-op returning CPX_OK, NULL with work to do is CPX_ERR_ARG, so is a
 * word_pos >= 2^64 - 2^32, and on any error nothing is written, states included.
 * The SECRECY note above does not apply to the seed of a public CRS (the crate's is the number 0); it does apply to instance streams: the
 * k of cpx_rng_instance_draws is the shuffler's secret. */
/* G1Projective::rand(rng).into_affine() n_each times per stream; out_compressed (nullable) receives the 48-byte encodings as well.  Needs no
 * CRS, leaves the loaded batch untouched.  count <= 2^20, n_each <= 2^16, count * n_each <= 2^22. */
int cpx_rng_g1(cpx_ctx* ctx, size_t count, uint8_t* states /* count*40, in/out */, size_t n_each, uint8_t* out_affine /* count*n_each*96 */,
               uint8_t* out_compressed /* count*n_each*48, may be NULL */);
/* The draws that open the reference's README example (README.md:85-95) per stream at the context's ell, in its order: the shuffle of 0..ell,
 * k = Fr::rand, vec_R (ell points), vec_S (ell points).  Any output may be NULL; the states advance by the whole set regardless.  Needs a
 * CRS (for ell: CPX_ERR_STATE without one).  What follows in the README exists above: cpx_rng_fr(4) -> cpx_batch_shuffle ->
 * cpx_batch_prove_rng -> cpx_rng_fr(8) -> cpx_batch_verify. */
int cpx_rng_instance_draws(cpx_ctx* ctx, size_t count, uint8_t* states /* count*40, in/out */, uint32_t* permutation_out /* count*ell */,
                           uint8_t* k_out /* count*32 */, uint8_t* vec_R_out /* count*ell*96 */, uint8_t* vec_S_out /* count*ell*96 */);
/* crs.rs:61-69 generate_crs: ell + 7 draws from the state, then exactly what cpx_ctx_set_crs(ctx, ell, points, ell + 7) does; the crate's
 * generate_crs(ell) is this call on cpx_rng_from_u64(0).  Every refusal cpx_ctx_set_crs would make for this ell (CPX_ERR_NOT_POW2) is made
 * before a word is drawn, with the state untouched.  ell + 7 <= 2^16. */
int cpx_crs_generate(cpx_ctx* ctx, size_t ell, uint8_t state[40] /* in/out */, uint8_t* points_out /* (ell+7)*96, may be NULL */);
/* [h] P for n affine points of E(Fp) — on the curve, NOT necessarily in the subgroup; points of small order included — by a compiled-in
 * addition chain (ark-ec mul_by_cofactor; independent of option "scale_any_point").  The identity goes in and comes out as 96 zero bytes;
 * as for cpx_g1_scale the points are taken as given (nothing is decoded or checked).  n <= 2^24. */
int cpx_g1_clear_cofactor(cpx_ctx* ctx, const uint8_t* points /* n*96 */, size_t n, uint8_t* out_affine /* n*96 */);

/* ---- measurement --------------------------------------------------------------------------- */
int cpx_set_profiling(cpx_ctx* ctx, int on); /* time every kernel group with HIP events on the ctx stream */
int cpx_reset_stats(cpx_ctx* ctx);
/* name = kernel name as rocprofv3 reports it, template arguments included: "k_msm_fix<16, 16>", "k_msm_tblw<32, false>",
 * "k_msm_tblw<2, true>", "k_msm_accw", "k_reduce_sets", "k_finalize_ranges", "k_table_build", "k_msm_tail", "k_smul",
 * "k_finalize", "k_compress", "k_decompress", "k_shuffle_status", "k_shuffle_gather", "k_shuffle_commit", "k_run_gather", "k_run_commit", "k_gen_table", "k_gen_mul", "k_fix_build", "k_find_scan", "k_find_compare", "k_tracker_check_scalars", "k_tracker_gather", "k_vs_crs_sum_groups", "k_rng_draw", "k_rng_g1_scan", "k_rng_g1_sqrt", "k_rng_g1_select", "k_clear_cofactor" (+ the host spans "host_prove_wall", "host_verify_wall", ...);
 * "k_smul" times the one-lane and the quad form alike; "k_smul_quad" counts (launches only) those of them that ran as k_smul_quad;
 * units = MSM points / scalar-mul elements / points; out pointers may be NULL */
int cpx_get_stat(const cpx_ctx* ctx, const char* name, uint64_t* launches, double* total_ms, double* algorithmic_bytes, double* units);
int cpx_set_host_threads(cpx_ctx* ctx, int threads);
/* dependent Fp multiply chains: returns achieved Fp products per second */
int cpx_bench_fpmul(cpx_ctx* ctx, int blocks, int iters, int reps, double* products_per_second);

#ifdef __cplusplus
}
#endif
#endif /* CPX_H */
