//! The two sub-argument provers with their log-round loops replaced by ONE library call each, and `transcript.rs` backed by the
//! 216-byte transcript value of the C ABI (include/cpx.h `cpx_transcript_*`, `cpx_ipa_rounds`, `cpx_same_msm_rounds`), and the two
//! verifiers as ONE library call each (`cpx_ipa_verify`, `cpx_same_msm_verify`), and the two `new` functions whole as ONE library call each
//! (`cpx_ipa_prove`, `cpx_same_msm_prove`: `ipa_new`, `same_msm_new` at the end of this file), under `--features mi355x`.  NOT COMPILED in the
//! build image.
//!
//! `merlin::Transcript` keeps its state private, so a transcript that the library is to continue has to live on the library's side of
//! the boundary from the start: `Transcript216` below holds the value and implements the crate's `CurdleproofsTranscript` on it.  The
//! provers then keep the crate's control flow up to the loop (commitments through `util::msm`, the step-1 messages, alpha / beta), hand
//! the bases, the vectors and the state to the library, and read the round points, the finals and the advanced state back.
#![allow(non_snake_case)]

use ark_bls12_381::{Fr, G1Affine, G1Projective};
use ark_ff::BigInt;
use ark_serialize::{CanonicalSerialize, SerializationError};
use ark_std::rand::RngCore;
use ark_std::UniformRand;

use crate::ffi::*;

pub const TRANSCRIPT_BYTES: usize = 216; // 25 Keccak lanes, pos, pos_begin as u64 LE

/// 32 bytes of wire memory (4 x u64 little-endian Montgomery limbs, what `scalars_ptr` exposes the other way) as an `Fr`
fn scalar_from_wire(b: &[u8]) -> Fr {
    let mut limbs = [0u64; 4];
    for (i, l) in limbs.iter_mut().enumerate() {
        *l = u64::from_le_bytes(b[8 * i..8 * i + 8].try_into().unwrap());
    }
    Fr::new_unchecked(BigInt::new(limbs))
}

/// transcript.rs:14-60 on the library's transcript value
#[derive(Clone)]
pub struct Transcript216(pub [u8; TRANSCRIPT_BYTES]);

impl Transcript216 {
    /// merlin::Transcript::new
    pub fn new(label: &'static [u8]) -> Self {
        let mut s = [0u8; TRANSCRIPT_BYTES];
        let rc = unsafe { cpx_transcript_new(label.as_ptr(), label.len(), s.as_mut_ptr()) };
        assert_eq!(rc, CPX_OK, "cpx_transcript_new");
        Transcript216(s)
    }
    pub fn append_message(&mut self, label: &'static [u8], message: &[u8]) {
        let rc = unsafe { cpx_transcript_append_message(self.0.as_mut_ptr(), label.as_ptr(), label.len(), message.as_ptr(), message.len()) };
        assert_eq!(rc, CPX_OK, "cpx_transcript_append_message");
    }
    /// transcript.rs:29-33 for any serialisable item: its compressed bytes as one message
    pub fn append<S: CanonicalSerialize>(&mut self, label: &'static [u8], item: &S) {
        let mut bytes = Vec::new();
        item.serialize_compressed(&mut bytes).unwrap();
        self.append_message(label, &bytes);
    }
    /// transcript.rs:35-38
    pub fn append_list<S: CanonicalSerialize>(&mut self, label: &'static [u8], items: &[&S]) {
        for item in items {
            self.append(label, *item);
        }
    }
    /// transcript.rs:41-54: the retries and the append-back happen inside the call
    pub fn get_and_append_challenge(&mut self, label: &'static [u8]) -> Fr {
        let mut out = [0u8; FR];
        let rc = unsafe { cpx_transcript_challenge_scalar(self.0.as_mut_ptr(), label.as_ptr(), label.len(), out.as_mut_ptr()) };
        assert_eq!(rc, CPX_OK, "cpx_transcript_challenge_scalar");
        scalar_from_wire(&out)
    }
}

/// What the loop of inner_product_argument.rs:150-186 leaves: the four point vectors of the proof and the two finals.
pub struct IpaRounds {
    pub vec_L_C: Vec<G1Projective>,
    pub vec_L_D: Vec<G1Projective>,
    pub vec_R_C: Vec<G1Projective>,
    pub vec_R_D: Vec<G1Projective>,
    pub c_final: Fr,
    pub d_final: Fr,
}

/// InnerProductProof::new from :150 on.  `H` is the loop's point (`crs_H * beta`, :140), `vec_c` / `vec_d` the vectors as they enter the
/// loop (:136-139).  Nothing is folded on the host: the library gathers every round's cross terms from the bases as uploaded.
pub fn ipa_rounds(vec_G: &[G1Affine], vec_G_prime: &[G1Affine], H: &G1Affine, vec_c: &[Fr], vec_d: &[Fr], transcript: &mut Transcript216) -> IpaRounds {
    let n = vec_c.len();
    let rounds = n.trailing_zeros() as usize;
    let mut affine = vec![0u8; rounds * 4 * AFF];
    let mut finals = [0u8; 2 * FR];
    let rc = unsafe {
        cpx_ipa_rounds(ctx(), 1, n, affine_to_wire(vec_G).as_ptr(), affine_to_wire(vec_G_prime).as_ptr(), affine_to_wire(std::slice::from_ref(H)).as_ptr(),
                       scalars_ptr(vec_c), scalars_ptr(vec_d), transcript.0.as_mut_ptr(), std::ptr::null_mut(), affine.as_mut_ptr(), finals.as_mut_ptr(),
                       std::ptr::null_mut())
    };
    assert_eq!(rc, CPX_OK, "cpx_ipa_rounds");
    let pts: Vec<G1Projective> = affine_from_wire(&affine).into_iter().map(Into::into).collect();
    let pick = |q: usize| (0..rounds).map(|j| pts[4 * j + q]).collect::<Vec<_>>(); // per round L_C, L_D, R_C, R_D
    IpaRounds { vec_L_C: pick(0), vec_L_D: pick(1), vec_R_C: pick(2), vec_R_D: pick(3), c_final: scalar_from_wire(&finals[..FR]), d_final: scalar_from_wire(&finals[FR..]) }
}

/// What the loop of same_multiscalar_argument.rs:99-136 leaves.
pub struct SameMsmRounds {
    pub vec_L: [Vec<G1Projective>; 3], // L_A, L_T, L_U
    pub vec_R: [Vec<G1Projective>; 3], // R_A, R_T, R_U
    pub x_final: Fr,
}

/// SameMultiscalarProof::new from :99 on; `vec_x` as it enters the loop (:95-97).  The identity entries of vec_T / vec_U (the blinder
/// slots, curdleproofs.rs:141-155) travel as 96 zero bytes.
pub fn same_msm_rounds(vec_G: &[G1Affine], vec_T: &[G1Affine], vec_U: &[G1Affine], vec_x: &[Fr], transcript: &mut Transcript216) -> SameMsmRounds {
    let n = vec_x.len();
    let rounds = n.trailing_zeros() as usize;
    let mut affine = vec![0u8; rounds * 6 * AFF];
    let mut x_final = [0u8; FR];
    let rc = unsafe {
        cpx_same_msm_rounds(ctx(), 1, n, affine_to_wire(vec_G).as_ptr(), affine_to_wire(vec_T).as_ptr(), affine_to_wire(vec_U).as_ptr(), scalars_ptr(vec_x),
                            transcript.0.as_mut_ptr(), std::ptr::null_mut(), affine.as_mut_ptr(), x_final.as_mut_ptr(), std::ptr::null_mut())
    };
    assert_eq!(rc, CPX_OK, "cpx_same_msm_rounds");
    let pts: Vec<G1Projective> = affine_from_wire(&affine).into_iter().map(Into::into).collect();
    let pick = |q: usize| (0..rounds).map(|j| pts[6 * j + q]).collect::<Vec<_>>();
    SameMsmRounds { vec_L: [pick(0), pick(1), pick(2)], vec_R: [pick(3), pick(4), pick(5)], x_final: scalar_from_wire(&x_final) }
}

/// Many proofs of one kind at once (a service proving a queue of shuffles keeps the crate's control flow per proof up to the loop and
/// meets here): the same calls with `count` items, every buffer item after item, one state per item.
pub fn ipa_rounds_many(n: usize, G: &[u8], G_prime: &[u8], H: &[u8], vec_c: &[Fr], vec_d: &[Fr], states: &mut [u8], affine_out: &mut [u8], finals_out: &mut [u8]) {
    let count = states.len() / TRANSCRIPT_BYTES;
    let rc = unsafe {
        cpx_ipa_rounds(ctx(), count, n, G.as_ptr(), G_prime.as_ptr(), H.as_ptr(), scalars_ptr(vec_c), scalars_ptr(vec_d), states.as_mut_ptr(), std::ptr::null_mut(),
                       affine_out.as_mut_ptr(), finals_out.as_mut_ptr(), std::ptr::null_mut())
    };
    assert_eq!(rc, CPX_OK, "cpx_ipa_rounds");
}

/// `count` non-zero draws of `Fr::rand`, what `MsmAccumulator::accumulate_check` would draw (msm_accumulator.rs:44), as wire bytes
fn draw_factors<T: RngCore>(rng: &mut T, count: usize) -> Vec<u8> {
    let mut drawn = Vec::with_capacity(count);
    while drawn.len() < count {
        let a = Fr::rand(rng);
        if a != Fr::from(0u64) {
            drawn.push(a);
        }
    }
    let mut out = vec![0u8; count * FR];
    out.copy_from_slice(unsafe { std::slice::from_raw_parts(scalars_ptr(&drawn), count * FR) });
    out
}

fn verdict(rc: std::os::raw::c_int, v: std::os::raw::c_int, what: &str) -> Result<bool, SerializationError> {
    assert_eq!(rc, CPX_OK, "{}", what);
    match v {
        CPX_OK => Ok(true),
        CPX_ERR_VERIFY => Ok(false),
        _ => Err(SerializationError::InvalidData), // CPX_ERR_DESERIALIZE: the reference fails in `deserialize`, before `verify`
    }
}

/// InnerProductProof::deserialize + verify (inner_product_argument.rs:340-352, :264-326) against an MsmAccumulator of its own, in one
/// call: `proof` holds the bytes `serialize` wrote (:328-338).  Ok(true): the accumulator verifies; Ok(false): it does not; Err: the bytes
/// do not decode, and the transcript is as it was.  Otherwise the transcript is advanced by the whole `verify`.
pub fn ipa_verify<T: RngCore>(proof: &[u8], crs_G_vec: &[G1Affine], crs_H: &G1Projective, C: &G1Projective, D: &G1Projective, z: &Fr, vec_u: &[Fr],
                              transcript: &mut Transcript216, rng: &mut T) -> Result<bool, SerializationError> {
    let n = crs_G_vec.len();
    let rand = draw_factors(rng, 2);
    let mut v: std::os::raw::c_int = CPX_ERR_VERIFY;
    let rc = unsafe {
        cpx_ipa_verify(ctx(), 1, n, affine_to_wire(crs_G_vec).as_ptr(), projective_to_wire(std::slice::from_ref(crs_H)).as_ptr(),
                       projective_to_wire(std::slice::from_ref(C)).as_ptr(), projective_to_wire(std::slice::from_ref(D)).as_ptr(), scalars_ptr(std::slice::from_ref(z)),
                       scalars_ptr(vec_u), proof.as_ptr(), rand.as_ptr(), transcript.0.as_mut_ptr(), std::ptr::null_mut(), &mut v)
    };
    verdict(rc, v, "cpx_ipa_verify")
}

/// SameMultiscalarProof::deserialize + verify (same_multiscalar_argument.rs:276-290, :213-261) likewise; three draws.
pub fn same_msm_verify<T: RngCore>(proof: &[u8], crs_G_vec: &[G1Affine], A: &G1Projective, Z_t: &G1Projective, Z_u: &G1Projective, vec_T: &[G1Affine], vec_U: &[G1Affine],
                                   transcript: &mut Transcript216, rng: &mut T) -> Result<bool, SerializationError> {
    let n = vec_T.len();
    let rand = draw_factors(rng, 3);
    let mut v: std::os::raw::c_int = CPX_ERR_VERIFY;
    let rc = unsafe {
        cpx_same_msm_verify(ctx(), 1, n, affine_to_wire(crs_G_vec).as_ptr(), affine_to_wire(vec_T).as_ptr(), affine_to_wire(vec_U).as_ptr(),
                            projective_to_wire(std::slice::from_ref(A)).as_ptr(), projective_to_wire(std::slice::from_ref(Z_t)).as_ptr(),
                            projective_to_wire(std::slice::from_ref(Z_u)).as_ptr(), proof.as_ptr(), rand.as_ptr(), transcript.0.as_mut_ptr(), std::ptr::null_mut(), &mut v)
    };
    verdict(rc, v, "cpx_same_msm_verify")
}

/// The draws of one `new` in the reference's order, as wire bytes: `generate_blinders(rng, count)` (util.rs:32-34)
fn draw_scalars<T: RngCore>(rng: &mut T, count: usize) -> Vec<u8> {
    let drawn: Vec<Fr> = (0..count).map(|_| Fr::rand(rng)).collect();
    let mut out = vec![0u8; count * FR];
    out.copy_from_slice(unsafe { std::slice::from_raw_parts(scalars_ptr(&drawn), count * FR) });
    out
}

/// InnerProductProof::new + serialize (inner_product_argument.rs:98-199, :328-338) in one call: blinders, B_c, B_d, step 1, alpha, beta,
/// H and all rounds run on the device; the bytes are what `ipa_verify` above takes.  The reference panics where generate_ipa_blinders
/// finds no inverse (:69, :71); so does this, after the call (the transcript is then as it was).  Draws: r [n], then z [n - 2] (:46-47).
pub fn ipa_new<T: RngCore>(crs_G_vec: &[G1Affine], crs_G_prime_vec: &[G1Affine], crs_H: &G1Projective, C: &G1Projective, D: &G1Projective, z: &Fr, vec_c: &[Fr],
                           vec_d: &[Fr], transcript: &mut Transcript216, rng: &mut T) -> Vec<u8> {
    let n = vec_c.len();
    let rounds = n.trailing_zeros() as usize;
    let rand = draw_scalars(rng, 2 * n - 2);
    let mut proof = vec![0u8; 48 * (2 + 4 * rounds) + 2 * FR];
    let mut status: std::os::raw::c_int = CPX_ERR_INTERNAL;
    let rc = unsafe {
        cpx_ipa_prove(ctx(), 1, n, affine_to_wire(crs_G_vec).as_ptr(), affine_to_wire(crs_G_prime_vec).as_ptr(), projective_to_wire(std::slice::from_ref(crs_H)).as_ptr(),
                      projective_to_wire(std::slice::from_ref(C)).as_ptr(), projective_to_wire(std::slice::from_ref(D)).as_ptr(), scalars_ptr(std::slice::from_ref(z)),
                      scalars_ptr(vec_c), scalars_ptr(vec_d), rand.as_ptr(), transcript.0.as_mut_ptr(), proof.as_mut_ptr(), std::ptr::null_mut(), &mut status)
    };
    assert_eq!(rc, CPX_OK, "cpx_ipa_prove");
    assert_eq!(status, CPX_OK, "generate_ipa_blinders: no inverse (inner_product_argument.rs:69, :71)");
    proof
}

/// SameMultiscalarProof::new + serialize (same_multiscalar_argument.rs:69-150, :263-275) likewise; the draws are vec_r (:78).
pub fn same_msm_new<T: RngCore>(crs_G_vec: &[G1Affine], A: &G1Projective, Z_t: &G1Projective, Z_u: &G1Projective, vec_T: &[G1Affine], vec_U: &[G1Affine], vec_x: &[Fr],
                                transcript: &mut Transcript216, rng: &mut T) -> Vec<u8> {
    let n = vec_x.len();
    let rounds = n.trailing_zeros() as usize;
    let rand = draw_scalars(rng, n);
    let mut proof = vec![0u8; 48 * (3 + 6 * rounds) + FR];
    let mut status: std::os::raw::c_int = CPX_ERR_INTERNAL;
    let rc = unsafe {
        cpx_same_msm_prove(ctx(), 1, n, affine_to_wire(crs_G_vec).as_ptr(), affine_to_wire(vec_T).as_ptr(), affine_to_wire(vec_U).as_ptr(),
                           projective_to_wire(std::slice::from_ref(A)).as_ptr(), projective_to_wire(std::slice::from_ref(Z_t)).as_ptr(),
                           projective_to_wire(std::slice::from_ref(Z_u)).as_ptr(), scalars_ptr(vec_x), rand.as_ptr(), transcript.0.as_mut_ptr(), proof.as_mut_ptr(),
                           std::ptr::null_mut(), &mut status)
    };
    assert_eq!(rc, CPX_OK, "cpx_same_msm_prove");
    assert_eq!(status, CPX_OK, "cpx_same_msm_prove: item status");
    proof
}

/// Many statements of one kind at once with the library's rng (include/cpx.h "the reference's rng as a ChaCha12 state"): one 40-byte state
/// and one transcript state per item, both in/out; `status[i]` as in include/cpx.h, pre-filled by the caller with a non-zero code.
pub fn ipa_new_many_rng(n: usize, G: &[u8], G_prime: &[u8], crs_H: &[u8], C: &[u8], D: &[u8], z: &[Fr], vec_c: &[Fr], vec_d: &[Fr], rng_states: &mut [u8],
                        states: &mut [u8], proofs_out: &mut [u8], status: &mut [std::os::raw::c_int]) {
    let count = states.len() / TRANSCRIPT_BYTES;
    let rc = unsafe {
        cpx_ipa_prove_rng(ctx(), count, n, G.as_ptr(), G_prime.as_ptr(), crs_H.as_ptr(), C.as_ptr(), D.as_ptr(), scalars_ptr(z), scalars_ptr(vec_c), scalars_ptr(vec_d),
                          rng_states.as_mut_ptr(), states.as_mut_ptr(), proofs_out.as_mut_ptr(), std::ptr::null_mut(), status.as_mut_ptr())
    };
    assert_eq!(rc, CPX_OK, "cpx_ipa_prove_rng");
}
