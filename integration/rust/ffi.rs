//! `src/ffi.rs` — bindings to the MI355X core (`include/cpx.h`, `libcpx.so`).  NOT COMPILED in the build image (no rustc there).
//!
//! arkworks 0.4 keeps `Fr` / `Fq` as `BigInt<N>([u64; N])` in Montgomery form and `G1Projective` as `{x, y, z}` of `Fq`:
//! the limb layout of the C-ABI (Fr 32 B, Fp 48 B).  `Fr` is `repr(transparent)`-like over `[u64; 4]` (a newtype chain of single
//! fields), so scalar slices are passed as the memory they occupy (checked once at start-up by `layout_self_check`).  Points are
//! NOT: `G1Affine {x, y, infinity}` and `G1Projective {x, y, z}` are `repr(Rust)` structs whose field order and padding the
//! compiler may choose, so both are marshalled field by field — affine points to 96 bytes `x || y` (the point at infinity as 96 zero
//! bytes), projective points to 144 bytes `X || Y || Z`.
#![allow(non_snake_case, non_camel_case_types, dead_code)]

use ark_bls12_381::{Fq, Fr, G1Affine, G1Projective};
use ark_ff::Zero;
use std::cell::RefCell;
use std::os::raw::{c_char, c_int, c_longlong, c_void};

#[repr(C)]
pub struct cpx_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct cpx_accum {
    _private: [u8; 0],
}

pub const CPX_OK: c_int = 0;
pub const CPX_ERR_ARG: c_int = -1;
pub const CPX_ERR_NOT_POW2: c_int = -2;
pub const CPX_ERR_HIP: c_int = -3;
pub const CPX_ERR_VERIFY: c_int = -4;
pub const CPX_ERR_DESERIALIZE: c_int = -5;
pub const CPX_ERR_STATE: c_int = -6;
pub const CPX_NO_OWNER: u32 = 0xffff_ffff;
pub const CPX_ERR_INTERNAL: c_int = -7;

extern "C" {
    pub fn cpx_ctx_create(device_id: c_int, out: *mut *mut cpx_ctx) -> c_int;
    pub fn cpx_ctx_destroy(ctx: *mut cpx_ctx);
    pub fn cpx_last_error(ctx: *const cpx_ctx) -> *const c_char;
    pub fn cpx_device_count() -> c_int;
    pub fn cpx_ctx_set_option(ctx: *mut cpx_ctx, key: *const c_char, value: c_longlong) -> c_int;
    pub fn cpx_ctx_get_option(ctx: *const cpx_ctx, key: *const c_char, value: *mut c_longlong) -> c_int;
    pub fn cpx_host_alloc(bytes: usize) -> *mut c_void;
    pub fn cpx_host_free(p: *mut c_void);
    // crs.rs:37-58
    pub fn cpx_ctx_set_crs(ctx: *mut cpx_ctx, ell: usize, points: *const u8, n_points: usize) -> c_int;
    pub fn cpx_crs_sums(ctx: *const cpx_ctx, g_sum: *mut u8, h_sum: *mut u8) -> c_int;
    pub fn cpx_proof_size(ctx: *const cpx_ctx) -> usize;
    pub fn cpx_batch_size(ctx: *const cpx_ctx) -> usize;
    // tier 0: util.rs:19-29 and the loops that bypass it
    pub fn cpx_g1_msm(ctx: *mut cpx_ctx, bases: *const u8, scalars: *const u8, n: usize, out: *mut u8) -> c_int;
    pub fn cpx_g1_msm_jac(ctx: *mut cpx_ctx, bases: *const u8, scalars: *const u8, n: usize, out: *mut u8) -> c_int;
    pub fn cpx_g1_fold(ctx: *mut cpx_ctx, pl: *mut u8, pr: *const u8, gamma: *const u8, half: usize) -> c_int;
    pub fn cpx_g1_scale(ctx: *mut cpx_ctx, p: *const u8, scalars: *const u8, scalar_stride: usize, n: usize, out: *mut u8) -> c_int;
    // one log round in two calls: the cross terms (inner_product_argument.rs:158-161, same_multiscalar_argument.rs:107-112), then the basis folds (:177-178, :128-130)
    pub fn cpx_g1_msm_many(ctx: *mut cpx_ctx, count: usize, lens: *const u32, bases: *const u8, scalars: *const u8, out_jac: *mut u8, out_compressed: *mut u8) -> c_int;
    pub fn cpx_g1_fold_many(ctx: *mut cpx_ctx, families: usize, half: usize, pl: *mut u8, pr: *const u8, gammas: *const u8) -> c_int;
    // the log-round loops themselves in one call each (inner_product_argument.rs:150-186, same_multiscalar_argument.rs:99-136), `count` items per call,
    // and the transcript as a 216-byte value (25 Keccak lanes, pos, pos_begin as u64 LE): subargs_mi355x.rs
    pub fn cpx_transcript_new(label: *const u8, label_len: usize, state_out: *mut u8) -> c_int;
    pub fn cpx_transcript_append_message(state: *mut u8, label: *const u8, label_len: usize, msg: *const u8, len: usize) -> c_int;
    pub fn cpx_transcript_append_scalar(state: *mut u8, label: *const u8, label_len: usize, scalar_mont: *const u8) -> c_int;
    pub fn cpx_transcript_challenge_bytes(state: *mut u8, label: *const u8, label_len: usize, out: *mut u8, len: usize) -> c_int;
    pub fn cpx_transcript_challenge_scalar(state: *mut u8, label: *const u8, label_len: usize, out_mont: *mut u8) -> c_int;
    pub fn cpx_ipa_rounds(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, g_prime: *const u8, h: *const u8, vec_c: *const u8, vec_d: *const u8,
                          transcripts: *mut u8, rounds_compressed: *mut u8, rounds_affine: *mut u8, finals: *mut u8, gammas: *mut u8) -> c_int;
    pub fn cpx_same_msm_rounds(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, t: *const u8, u: *const u8, vec_x: *const u8, transcripts: *mut u8,
                               rounds_compressed: *mut u8, rounds_affine: *mut u8, finals: *mut u8, gammas: *mut u8) -> c_int;
    // the verifiers of the two sub-arguments on the caller's bases (inner_product_argument.rs:202-326, same_multiscalar_argument.rs:153-261), `count`
    // stand-alone proofs per call, each against an accumulator of its own; verdicts[i] = CPX_OK / CPX_ERR_VERIFY / CPX_ERR_DESERIALIZE: subargs_mi355x.rs
    pub fn cpx_ipa_verify(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, crs_h: *const u8, c: *const u8, d: *const u8, z: *const u8, vec_u: *const u8,
                          proofs: *const u8, rand: *const u8, transcripts: *mut u8, challenges: *mut u8, verdicts: *mut c_int) -> c_int;
    pub fn cpx_same_msm_verify(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, t: *const u8, u: *const u8, a: *const u8, z_t: *const u8, z_u: *const u8,
                               proofs: *const u8, rand: *const u8, transcripts: *mut u8, challenges: *mut u8, verdicts: *mut c_int) -> c_int;
    // the provers of the two sub-arguments on the caller's bases (inner_product_argument.rs:98-199, same_multiscalar_argument.rs:69-150), `count`
    // stand-alone statements per call: the reference's `serialize` bytes out; status[i] = CPX_OK / CPX_ERR_ARG (generate_ipa_blinders panics);
    // the _rng forms draw on the device from 40-byte ChaCha12 states: subargs_mi355x.rs
    pub fn cpx_ipa_prove(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, g_prime: *const u8, crs_h: *const u8, c: *const u8, d: *const u8, z: *const u8,
                         vec_c: *const u8, vec_d: *const u8, rand: *const u8, transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_same_msm_prove(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, t: *const u8, u: *const u8, a: *const u8, z_t: *const u8, z_u: *const u8,
                              vec_x: *const u8, rand: *const u8, transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_ipa_prove_rng(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, g_prime: *const u8, crs_h: *const u8, c: *const u8, d: *const u8, z: *const u8,
                             vec_c: *const u8, vec_d: *const u8, states: *mut u8, transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_same_msm_prove_rng(ctx: *mut cpx_ctx, count: usize, n: usize, g: *const u8, t: *const u8, u: *const u8, a: *const u8, z_t: *const u8, z_u: *const u8,
                                  vec_x: *const u8, states: *mut u8, transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    // the grand-product prover on the caller's bases (grand_product_argument.rs:43-166), `count` stand-alone statements of ell factors and
    // n_blinders blinders per call: C, r_p and the InnerProductProof bytes out; rand = vec_c_blinders, then the inner-product prover's draws
    pub fn cpx_gprod_prove(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, b: *const u8,
                           gprod_result: *const u8, vec_b: *const u8, vec_b_blinders: *const u8, rand: *const u8, transcripts: *mut u8, proofs: *mut u8,
                           challenges: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_gprod_prove_rng(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, b: *const u8,
                               gprod_result: *const u8, vec_b: *const u8, vec_b_blinders: *const u8, states: *mut u8, transcripts: *mut u8, proofs: *mut u8,
                               challenges: *mut u8, status: *mut c_int) -> c_int;
    // GrandProductProof::verify on those bytes (grand_product_argument.rs:180-246): crs_g_sum / crs_h_sum affine, taken from the caller
    pub fn cpx_gprod_verify(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, crs_g_sum: *const u8,
                            crs_h_sum: *const u8, b: *const u8, gprod_result: *const u8, proofs: *const u8, rand: *const u8, transcripts: *mut u8,
                            challenges: *mut u8, verdicts: *mut c_int) -> c_int;
    // the same-permutation prover on the caller's bases (same_permutation_argument.rs:40-99), `count` stand-alone statements per call: B and
    // the GrandProductProof bytes out; permutation: ell u32 values below ell per item; rand = the draws of cpx_gprod_prove
    pub fn cpx_same_perm_prove(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, a: *const u8,
                               m: *const u8, vec_a: *const u8, permutation: *const u32, vec_a_blinders: *const u8, vec_m_blinders: *const u8, rand: *const u8,
                               transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_same_perm_prove_rng(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, a: *const u8,
                                   m: *const u8, vec_a: *const u8, permutation: *const u32, vec_a_blinders: *const u8, vec_m_blinders: *const u8, states: *mut u8,
                                   transcripts: *mut u8, proofs: *mut u8, challenges: *mut u8, status: *mut c_int) -> c_int;
    // SamePermutationProof::verify on those bytes (same_permutation_argument.rs:112-171): three factors per item in rand
    pub fn cpx_same_perm_verify(ctx: *mut cpx_ctx, count: usize, ell: usize, n_blinders: usize, g: *const u8, h: *const u8, crs_u: *const u8, crs_g_sum: *const u8,
                                crs_h_sum: *const u8, a: *const u8, m: *const u8, vec_a: *const u8, proofs: *const u8, rand: *const u8, transcripts: *mut u8,
                                challenges: *mut u8, verdicts: *mut c_int) -> c_int;
    pub fn cpx_g1_normalize(ctx: *mut cpx_ctx, jac: *const u8, n: usize, out_affine: *mut u8, out_compressed: *mut u8) -> c_int;
    pub fn cpx_g1_decompress(ctx: *mut cpx_ctx, compressed: *const u8, n: usize, out_affine: *mut u8, check_subgroup: c_int) -> c_int;
    // one verdict per point (0 ok, 1 malformed / not on the curve, 2 outside the subgroup): the square root behind tests/crs.rs:13-52
    pub fn cpx_g1_decompress_status(ctx: *mut cpx_ctx, compressed: *const u8, n: usize, out_affine: *mut u8, check_subgroup: c_int, status: *mut u8) -> c_int;
    // tier 1: msm_accumulator.rs:22-68
    pub fn cpx_accum_new(ctx: *mut cpx_ctx, out: *mut *mut cpx_accum) -> c_int;
    pub fn cpx_accum_free(acc: *mut cpx_accum);
    pub fn cpx_accum_check(acc: *mut cpx_accum, c: *const u8, vec_x: *const u8, vec_v: *const u8, n: usize, random_factor: *const u8) -> c_int;
    pub fn cpx_accum_verify(acc: *mut cpx_accum) -> c_int;
    // tier 2: curdleproofs.rs:59, :197 for batches of instances resident in HBM
    pub fn cpx_batch_load(ctx: *mut cpx_ctx, batch: usize, vec_r: *const u8, vec_s: *const u8, vec_t: *const u8, vec_u: *const u8, m: *const u8) -> c_int;
    pub fn cpx_batch_load_begin(ctx: *mut cpx_ctx, batch: usize, vec_r: *const u8, vec_s: *const u8, vec_t: *const u8, vec_u: *const u8, m: *const u8) -> c_int;
    pub fn cpx_batch_load_end(ctx: *mut cpx_ctx) -> c_int;
    pub fn cpx_batch_prove(ctx: *mut cpx_ctx, permutation: *const u32, k: *const u8, vec_m_blinders: *const u8, rand: *const u8, proofs_out: *mut u8) -> c_int;
    pub fn cpx_batch_verify(ctx: *mut cpx_ctx, proofs: *const u8, rand: *const u8, verdict: *mut c_int) -> c_int;
    pub fn cpx_batch_verify_fused(ctx: *mut cpx_ctx, proofs: *const u8, rand: *const u8, partial_jac: *mut u8, n_invalid: *mut c_int) -> c_int;
    // the grouped form of the accumulated check: one verdict per proof, 12 factors per proof; n_rechecked may be null
    pub fn cpx_batch_verify_grouped(ctx: *mut cpx_ctx, proofs: *const u8, rand: *const u8, verdict: *mut c_int, n_rechecked: *mut usize) -> c_int;
    pub fn cpx_g1_sum_jac(ctx: *mut cpx_ctx, points_jac: *const u8, n: usize, out_jac: *mut u8, is_identity: *mut c_int) -> c_int;
    // whisk.rs byte-level API
    pub fn cpx_whisk_generate_shuffle_proof(ctx: *mut cpx_ctx, pre_trackers: *const u8, permutation: *const u32, k: *const u8, vec_m_blinders: *const u8,
                                            rand: *const u8, post_trackers_out: *mut u8, proof_out: *mut u8) -> c_int;
    pub fn cpx_whisk_is_valid_shuffle_proof(ctx: *mut cpx_ctx, pre_trackers: *const u8, post_trackers: *const u8, proof: *const u8, rand: *const u8,
                                            valid: *mut c_int) -> c_int;
    pub fn cpx_whisk_generate_tracker_proof(ctx: *mut cpx_ctx, tracker: *const u8, k: *const u8, blinder: *const u8, proof_out: *mut u8) -> c_int;
    pub fn cpx_whisk_is_valid_tracker_proof(ctx: *mut cpx_ctx, tracker: *const u8, k_commitment: *const u8, proof: *const u8, valid: *mut c_int) -> c_int;
    // `count` tracker proofs per call: per-item status / verdict, the call itself returns CPX_OK
    pub fn cpx_whisk_generate_tracker_proofs(ctx: *mut cpx_ctx, count: usize, trackers: *const u8, k: *const u8, blinders: *const u8, proofs_out: *mut u8,
                                             status: *mut c_int) -> c_int;
    pub fn cpx_whisk_verify_tracker_proofs(ctx: *mut cpx_ctx, count: usize, trackers: *const u8, k_commitments: *const u8, proofs: *const u8,
                                           verdict: *mut c_int) -> c_int;
    // the verifier as ONE multi-scalar multiplication: rand = two non-zero reduced weights per item (a_i, b_i; Montgomery limbs); fused = the 144-byte
    // partial sum and the number of undecodable items, grouped = one verdict per item and the number of items the second stage rechecked
    pub fn cpx_whisk_verify_tracker_proofs_fused(ctx: *mut cpx_ctx, count: usize, trackers: *const u8, k_commitments: *const u8, proofs: *const u8,
                                                 rand: *const u8, partial_jac: *mut u8, n_invalid: *mut c_int) -> c_int;
    pub fn cpx_whisk_verify_tracker_proofs_grouped(ctx: *mut cpx_ctx, count: usize, trackers: *const u8, k_commitments: *const u8, proofs: *const u8,
                                                   rand: *const u8, verdict: *mut c_int, n_rechecked: *mut usize) -> c_int;
    // what those calls consume, `count` per call, as multiples of the generator on its fixed-base table (whisk.rs:45-55, :370); either output may be null
    pub fn cpx_g1_generator_mul(ctx: *mut cpx_ctx, count: usize, scalars: *const u8, out_affine: *mut u8, out_compressed: *mut u8) -> c_int;
    pub fn cpx_whisk_trackers_from_k_r(ctx: *mut cpx_ctx, count: usize, k: *const u8, r: *const u8, trackers_out: *mut u8, k_commitments_out: *mut u8) -> c_int;
    // which key opens which tracker, k_j * r_G_i == k_r_G_i (whisk.rs:36-55, :323) for every pair: owner[i] = the smallest such j or CPX_NO_OWNER,
    // status[i] = CPX_OK / CPX_ERR_DESERIALIZE; k may be null with n_keys = 0
    pub fn cpx_whisk_find_trackers(ctx: *mut cpx_ctx, n_trackers: usize, trackers: *const u8, n_keys: usize, k: *const u8, owner: *mut u32, status: *mut c_int) -> c_int;
    // `count` shuffles per call (util.rs:83-106, whisk.rs:144-179, :106-130): the instances become the loaded batch; per-item status / verdict
    pub fn cpx_batch_shuffle(ctx: *mut cpx_ctx, count: usize, vec_r: *const u8, vec_s: *const u8, permutation: *const u32, k: *const u8, vec_m_blinders: *const u8,
                             vec_t_out: *mut u8, vec_u_out: *mut u8, m_out: *mut u8) -> c_int;
    pub fn cpx_whisk_generate_shuffle_proofs(ctx: *mut cpx_ctx, count: usize, pre_trackers: *const u8, permutation: *const u32, k: *const u8,
                                             vec_m_blinders: *const u8, rand: *const u8, post_trackers_out: *mut u8, proofs_out: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_whisk_verify_shuffle_proofs(ctx: *mut cpx_ctx, count: usize, pre_trackers: *const u8, post_trackers: *const u8, proofs: *const u8, rand: *const u8,
                                           verdict: *mut c_int) -> c_int;
    pub fn cpx_whisk_verify_shuffle_proofs_grouped(ctx: *mut cpx_ctx, count: usize, pre_trackers: *const u8, post_trackers: *const u8, proofs: *const u8,
                                                   rand: *const u8, verdict: *mut c_int, n_rechecked: *mut usize) -> c_int;
    // the resident candidate tracker list (96 bytes per tracker; status: one decoder code per candidate, may be null) and whisk.rs:106-130 for a
    // run of shuffles over it: item b reads candidates indices[b][..] of the list as it stands after items 0..b-1 were written back; the
    // *n_applied leading accepted items are written back (n_applied null: a dry run)
    pub fn cpx_whisk_candidates_load(ctx: *mut cpx_ctx, n: usize, trackers: *const u8, status: *mut u8) -> c_int;
    pub fn cpx_whisk_candidates_size(ctx: *mut cpx_ctx) -> usize;
    pub fn cpx_whisk_candidates_read(ctx: *mut cpx_ctx, first: usize, count: usize, trackers_out: *mut u8) -> c_int;
    pub fn cpx_whisk_verify_shuffle_run(ctx: *mut cpx_ctx, count: usize, indices: *const u32, post_trackers: *const u8, proofs: *const u8, rand: *const u8,
                                        verdict: *mut c_int, n_applied: *mut usize) -> c_int;
    pub fn cpx_whisk_verify_shuffle_run_grouped(ctx: *mut cpx_ctx, count: usize, indices: *const u32, post_trackers: *const u8, proofs: *const u8,
                                                rand: *const u8, verdict: *mut c_int, n_applied: *mut usize, n_rechecked: *mut usize) -> c_int;
    // the caller's `rng` as ChaCha12 states (40 bytes per stream: get_seed() || get_word_pos() as u64 LE), the draws made on the device
    pub fn cpx_rng_from_u64(seed: u64, state_out: *mut u8) -> c_int;
    pub fn cpx_rng_split(parent: *mut u8, count: usize, states_out: *mut u8) -> c_int;
    pub fn cpx_rng_fr(ctx: *mut cpx_ctx, count: usize, states: *mut u8, n_each: usize, out: *mut u8) -> c_int;
    pub fn cpx_rng_shuffle_draws(ctx: *mut cpx_ctx, count: usize, states: *mut u8, permutation_out: *mut u32, k_out: *mut u8, blinders_out: *mut u8,
                                 rand_out: *mut u8) -> c_int;
    pub fn cpx_whisk_generate_shuffle_proofs_rng(ctx: *mut cpx_ctx, count: usize, pre_trackers: *const u8, states: *mut u8, post_trackers_out: *mut u8,
                                                 proofs_out: *mut u8, status: *mut c_int) -> c_int;
    pub fn cpx_batch_prove_rng(ctx: *mut cpx_ctx, permutation: *const u32, k: *const u8, vec_m_blinders: *const u8, states: *mut u8, proofs_out: *mut u8) -> c_int;
    pub fn cpx_rng_g1(ctx: *mut cpx_ctx, count: usize, states: *mut u8, n_each: usize, out_affine: *mut u8, out_compressed: *mut u8) -> c_int;
    pub fn cpx_rng_instance_draws(ctx: *mut cpx_ctx, count: usize, states: *mut u8, permutation_out: *mut u32, k_out: *mut u8, vec_R_out: *mut u8,
                                  vec_S_out: *mut u8) -> c_int;
    pub fn cpx_crs_generate(ctx: *mut cpx_ctx, ell: usize, state: *mut u8, points_out: *mut u8) -> c_int;
    pub fn cpx_g1_clear_cofactor(ctx: *mut cpx_ctx, points: *const u8, n: usize, out_affine: *mut u8) -> c_int;
}

pub const RNG_STATE: usize = 40;
/// The wire state of a `ChaCha12Rng` (= rand 0.8 `StdRng`): `get_seed()` and the low 64 bits of `get_word_pos()`.
pub fn rng_state(rng: &rand_chacha::ChaCha12Rng) -> [u8; RNG_STATE] {
    let mut s = [0u8; RNG_STATE];
    s[..32].copy_from_slice(&rng.get_seed());
    s[32..].copy_from_slice(&(rng.get_word_pos() as u64).to_le_bytes());
    s
}
/// Continues `rng` where the library stopped.
pub fn rng_resume(rng: &mut rand_chacha::ChaCha12Rng, state: &[u8]) {
    debug_assert_eq!(&state[..32], &rng.get_seed()[..]);
    rng.set_word_pos(u64::from_le_bytes(state[32..40].try_into().unwrap()) as u128);
}

pub const AFF: usize = 96;
pub const JAC: usize = 144;
pub const FR: usize = 32;

fn fq_bytes(x: &Fq) -> [u8; 48] {
    let mut o = [0u8; 48];
    for (i, limb) in x.0 .0.iter().enumerate() {
        o[8 * i..8 * i + 8].copy_from_slice(&limb.to_le_bytes());
    }
    o
}
fn fq_from_bytes(b: &[u8]) -> Fq {
    let mut limbs = [0u64; 6];
    for i in 0..6 {
        limbs[i] = u64::from_le_bytes(b[8 * i..8 * i + 8].try_into().unwrap());
    }
    ark_ff::Fp(ark_ff::BigInt(limbs), core::marker::PhantomData) // limbs already are the Montgomery representation
}

/// 96 bytes per point, the point at infinity as zeros
pub fn affine_to_wire(points: &[G1Affine]) -> Vec<u8> {
    let mut v = vec![0u8; AFF * points.len()];
    for (i, q) in points.iter().enumerate() {
        if !q.infinity {
            v[AFF * i..AFF * i + 48].copy_from_slice(&fq_bytes(&q.x));
            v[AFF * i + 48..AFF * i + 96].copy_from_slice(&fq_bytes(&q.y));
        }
    }
    v
}
pub fn affine_from_wire(b: &[u8]) -> Vec<G1Affine> {
    b.chunks(AFF)
        .map(|c| {
            if c.iter().all(|x| *x == 0) {
                G1Affine::identity()
            } else {
                G1Affine::new_unchecked(fq_from_bytes(&c[..48]), fq_from_bytes(&c[48..]))
            }
        })
        .collect()
}
/// `&[Fr]` already is wire memory (4 x u64 little-endian Montgomery limbs per element); `layout_self_check` asserts it
pub fn scalars_ptr(s: &[Fr]) -> *const u8 {
    s.as_ptr() as *const u8
}
/// 144 bytes per point, `X || Y || Z`, written field by field (`Projective<P>` is `repr(Rust)`: no cast of the struct's memory)
pub fn projective_to_wire(points: &[G1Projective]) -> Vec<u8> {
    let mut v = vec![0u8; JAC * points.len()];
    for (i, q) in points.iter().enumerate() {
        v[JAC * i..JAC * i + 48].copy_from_slice(&fq_bytes(&q.x));
        v[JAC * i + 48..JAC * i + 96].copy_from_slice(&fq_bytes(&q.y));
        v[JAC * i + 96..JAC * i + 144].copy_from_slice(&fq_bytes(&q.z));
    }
    v
}
/// Run once before the first FFI call (`ctx()` does): what the scalar pointer casts rest on — an `Fr` occupies exactly its four
/// Montgomery limbs, in order, little-endian.
pub fn layout_self_check() {
    use ark_ff::One;
    assert_eq!(std::mem::size_of::<Fr>(), FR, "Fr is not 4 x u64");
    assert_eq!(std::mem::align_of::<Fr>(), 8);
    let x = Fr::one() + Fr::one() + Fr::one();
    let bytes: [u8; FR] = unsafe { std::mem::transmute_copy(&x) };
    for i in 0..4 {
        assert_eq!(u64::from_le_bytes(bytes[8 * i..8 * i + 8].try_into().unwrap()), x.0 .0[i], "Fr memory is not its Montgomery limbs in order");
    }
}
pub fn projective_from_wire(b: &[u8; JAC]) -> G1Projective {
    let z = fq_from_bytes(&b[96..]);
    if z.is_zero() {
        return G1Projective::zero();
    }
    G1Projective::new_unchecked(fq_from_bytes(&b[..48]), fq_from_bytes(&b[48..96]), z)
}

/// One context per thread (a ctx = one device + one stream, not re-entrant); device from `CPX_DEVICE` (default 0).
pub struct Ctx(pub *mut cpx_ctx);
impl Drop for Ctx {
    fn drop(&mut self) {
        unsafe { cpx_ctx_destroy(self.0) }
    }
}
thread_local! {
    static CTX: RefCell<Option<Ctx>> = RefCell::new(None);
}
pub fn ctx() -> *mut cpx_ctx {
    CTX.with(|c| {
        let mut c = c.borrow_mut();
        if c.is_none() {
            let dev = std::env::var("CPX_DEVICE").ok().and_then(|s| s.parse().ok()).unwrap_or(0);
            let mut h: *mut cpx_ctx = std::ptr::null_mut();
            let rc = unsafe { cpx_ctx_create(dev, &mut h) };
            assert_eq!(rc, CPX_OK, "cpx_ctx_create: no usable MI355X (there is no CPU fallback)");
            layout_self_check();
            *c = Some(Ctx(h));
        }
        c.as_ref().unwrap().0
    })
}
/// Loads `crs` into the calling thread's context if it is not the one loaded last (tables are shared process-wide per device).
pub fn ctx_with_crs(crs: &crate::crs::CurdleproofsCrs) -> *mut cpx_ctx {
    thread_local! { static LOADED: RefCell<Vec<u8>> = RefCell::new(Vec::new()); }
    let mut pts: Vec<G1Affine> = Vec::with_capacity(crs.vec_G.len() + 7);
    pts.extend_from_slice(&crs.vec_G);
    pts.extend_from_slice(&crs.vec_H);
    pts.push(crs.H.into());
    pts.push(crs.G_t.into());
    pts.push(crs.G_u.into());
    let wire = affine_to_wire(&pts);
    let h = ctx();
    LOADED.with(|l| {
        let mut l = l.borrow_mut();
        if *l != wire {
            let rc = unsafe { cpx_ctx_set_crs(h, crs.vec_G.len(), wire.as_ptr(), pts.len()) };
            assert_eq!(rc, CPX_OK, "cpx_ctx_set_crs");
            *l = wire;
        }
    });
    h
}
