//! The four byte-level `pub fn`s of `src/whisk.rs` over `cpx_whisk_*` (reference whisk.rs:106-130, :144-179, :183-226,
//! :228-263) under `--features mi355x`: same signatures, same rng draw order, hence the same bytes.  NOT COMPILED here.
#![allow(non_snake_case)]

use ark_bls12_381::Fr;
use ark_serialize::SerializationError;
use ark_std::rand::seq::SliceRandom;
use ark_std::rand::RngCore;
use ark_std::UniformRand;

use crate::crs::CurdleproofsCrs;
use crate::ffi::*;
use crate::util::generate_blinders;
use crate::whisk::{TrackerProofBytes, WhiskShuffleProofBytes, WhiskTracker, ELL, N, TRACKER_PROOF_SIZE, WHISK_SHUFFLE_PROOF_SIZE};
use crate::N_BLINDERS;

fn trackers_to_wire(trackers: &[WhiskTracker]) -> Vec<u8> {
    trackers.iter().flat_map(|t| t.r_G.iter().chain(t.k_r_G.iter()).copied()).collect() // 96 B: r_G || k_r_G (whisk.rs:36-42)
}
fn map_rc(rc: std::os::raw::c_int) -> Result<(), SerializationError> {
    match rc {
        CPX_OK => Ok(()),
        CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
        rc => panic!("libcpx: {}", rc),
    }
}
fn nonzero_factors<T: RngCore>(count: usize, rng: &mut T) -> Vec<Fr> {
    let mut v = Vec::with_capacity(count);
    while v.len() < count {
        let a = Fr::rand(rng);
        if a != Fr::from(0u64) {
            v.push(a);
        }
    }
    v
}

/// whisk.rs:106-130
pub fn is_valid_whisk_shuffle_proof<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    pre_trackers: &[WhiskTracker],
    post_trackers: &[WhiskTracker],
    whisk_shuffle_proof_bytes: &WhiskShuffleProofBytes,
) -> Result<bool, SerializationError> {
    let factors = nonzero_factors(8, rng); // the accumulate_check draws of CurdleproofsProof::verify
    let mut valid: std::os::raw::c_int = 0;
    map_rc(unsafe {
        cpx_whisk_is_valid_shuffle_proof(ctx_with_crs(crs), trackers_to_wire(pre_trackers).as_ptr(), trackers_to_wire(post_trackers).as_ptr(),
                                         whisk_shuffle_proof_bytes.as_ptr(), scalars_ptr(&factors), &mut valid)
    })?;
    Ok(valid == 1)
}

/// whisk.rs:144-179
pub fn generate_whisk_shuffle_proof<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    pre_trackers: &[WhiskTracker],
) -> Result<(Vec<WhiskTracker>, WhiskShuffleProofBytes), SerializationError> {
    let mut permutation: Vec<u32> = (0..ELL as u32).collect();
    permutation.shuffle(rng); // :152-155
    let k = Fr::rand(rng); // :156
    let vec_m_blinders = generate_blinders(rng, N_BLINDERS); // util.rs:91, inside shuffle_permute_and_commit_input
    let rand: Vec<Fr> = (0..3 * N + 9).map(|_| Fr::rand(rng)).collect(); // the draws of CurdleproofsProof::new
    let mut post = vec![0u8; 96 * ELL];
    let mut proof = [0u8; WHISK_SHUFFLE_PROOF_SIZE];
    map_rc(unsafe {
        cpx_whisk_generate_shuffle_proof(ctx_with_crs(crs), trackers_to_wire(pre_trackers).as_ptr(), permutation.as_ptr(), scalars_ptr(std::slice::from_ref(&k)),
                                         scalars_ptr(&vec_m_blinders), scalars_ptr(&rand), post.as_mut_ptr(), proof.as_mut_ptr())
    })?;
    let post_trackers = post.chunks(96).map(|c| WhiskTracker { r_G: c[..48].try_into().unwrap(), k_r_G: c[48..].try_into().unwrap() }).collect();
    Ok((post_trackers, proof))
}

/// whisk.rs:183-226
pub fn is_valid_whisk_tracker_proof(tracker: &WhiskTracker, k_commitment: &[u8; 48], tracker_proof: &TrackerProofBytes) -> Result<bool, SerializationError> {
    let mut valid: std::os::raw::c_int = 0;
    let t = trackers_to_wire(std::slice::from_ref(tracker));
    map_rc(unsafe { cpx_whisk_is_valid_tracker_proof(ctx(), t.as_ptr(), k_commitment.as_ptr(), tracker_proof.as_ptr(), &mut valid) })?;
    Ok(valid == 1)
}

/// whisk.rs:228-263
pub fn generate_whisk_tracker_proof<T: RngCore>(rng: &mut T, tracker: &WhiskTracker, k: &Fr) -> Result<TrackerProofBytes, SerializationError> {
    let blinder = Fr::rand(rng); // :238
    let mut out = [0u8; TRACKER_PROOF_SIZE];
    let t = trackers_to_wire(std::slice::from_ref(tracker));
    map_rc(unsafe { cpx_whisk_generate_tracker_proof(ctx(), t.as_ptr(), scalars_ptr(std::slice::from_ref(k)), scalars_ptr(std::slice::from_ref(&blinder)), out.as_mut_ptr()) })?;
    Ok(out)
}

/// whisk.rs:183-226 for many (tracker, k_commitment, proof) triples in one library call: one result per item, in order
pub fn are_valid_whisk_tracker_proofs(
    trackers: &[WhiskTracker],
    k_commitments: &[[u8; 48]],
    tracker_proofs: &[TrackerProofBytes],
) -> Vec<Result<bool, SerializationError>> {
    assert!(trackers.len() == k_commitments.len() && trackers.len() == tracker_proofs.len());
    let count = trackers.len();
    let kc: Vec<u8> = k_commitments.iter().flat_map(|c| c.iter().copied()).collect();
    let pf: Vec<u8> = tracker_proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let mut verdict = vec![CPX_ERR_INTERNAL; count]; // an entry the library does not write is never read as accepted
    let rc = unsafe { cpx_whisk_verify_tracker_proofs(ctx(), count, trackers_to_wire(trackers).as_ptr(), kc.as_ptr(), pf.as_ptr(), verdict.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    verdict
        .into_iter()
        .map(|v| match v {
            CPX_OK => Ok(true),
            CPX_ERR_VERIFY => Ok(false),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            v => panic!("libcpx: {}", v),
        })
        .collect()
}

/// The same through the grouped check: two weights per item drawn from `rng` (a_i, b_i, in item order), every group of items one MSM,
/// the per-item relations only for the items of a group whose sum is not the identity.  Returns the results and the number rechecked.
pub fn are_valid_whisk_tracker_proofs_grouped<T: RngCore>(
    rng: &mut T,
    trackers: &[WhiskTracker],
    k_commitments: &[[u8; 48]],
    tracker_proofs: &[TrackerProofBytes],
) -> (Vec<Result<bool, SerializationError>>, usize) {
    assert!(trackers.len() == k_commitments.len() && trackers.len() == tracker_proofs.len());
    let count = trackers.len();
    let kc: Vec<u8> = k_commitments.iter().flat_map(|c| c.iter().copied()).collect();
    let pf: Vec<u8> = tracker_proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let weights: Vec<Fr> = (0..2 * count).map(|_| loop { let w = Fr::rand(rng); if w != Fr::from(0u64) { break w; } }).collect();
    let mut verdict = vec![CPX_ERR_INTERNAL; count];
    let mut rechecked = 0usize;
    let rc = unsafe {
        cpx_whisk_verify_tracker_proofs_grouped(ctx(), count, trackers_to_wire(trackers).as_ptr(), kc.as_ptr(), pf.as_ptr(), scalars_ptr(&weights), verdict.as_mut_ptr(), &mut rechecked)
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    let res = verdict
        .into_iter()
        .map(|v| match v {
            CPX_OK => Ok(true),
            CPX_ERR_VERIFY => Ok(false),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            v => panic!("libcpx: {}", v),
        })
        .collect();
    (res, rechecked)
}

/// The fused form: this call's 144-byte partial sum and the number of undecodable items.  A batch is accepted iff no call reports an invalid
/// item and all partials — those of the shuffle proofs and of other GPUs included — add up to the identity (cpx_g1_sum_jac).
pub fn whisk_tracker_proofs_partial<T: RngCore>(
    rng: &mut T,
    trackers: &[WhiskTracker],
    k_commitments: &[[u8; 48]],
    tracker_proofs: &[TrackerProofBytes],
) -> ([u8; 144], usize) {
    assert!(trackers.len() == k_commitments.len() && trackers.len() == tracker_proofs.len());
    let count = trackers.len();
    let kc: Vec<u8> = k_commitments.iter().flat_map(|c| c.iter().copied()).collect();
    let pf: Vec<u8> = tracker_proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let weights: Vec<Fr> = (0..2 * count).map(|_| loop { let w = Fr::rand(rng); if w != Fr::from(0u64) { break w; } }).collect();
    let mut partial = [0u8; 144];
    let mut n_invalid: std::os::raw::c_int = 0;
    let rc = unsafe {
        cpx_whisk_verify_tracker_proofs_fused(ctx(), count, trackers_to_wire(trackers).as_ptr(), kc.as_ptr(), pf.as_ptr(), scalars_ptr(&weights), partial.as_mut_ptr(), &mut n_invalid)
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    (partial, n_invalid as usize)
}

/// whisk.rs:228-263 for many (tracker, k) pairs in one library call; the blinders are drawn in item order (:238)
pub fn generate_whisk_tracker_proofs<T: RngCore>(rng: &mut T, trackers: &[WhiskTracker], ks: &[Fr]) -> Vec<Result<TrackerProofBytes, SerializationError>> {
    assert!(trackers.len() == ks.len());
    let count = trackers.len();
    let blinders: Vec<Fr> = (0..count).map(|_| Fr::rand(rng)).collect();
    let mut out = vec![0u8; TRACKER_PROOF_SIZE * count];
    let mut status = vec![CPX_ERR_INTERNAL; count];
    let rc = unsafe {
        cpx_whisk_generate_tracker_proofs(ctx(), count, trackers_to_wire(trackers).as_ptr(), scalars_ptr(ks), scalars_ptr(&blinders), out.as_mut_ptr(), status.as_mut_ptr())
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    status
        .iter()
        .zip(out.chunks(TRACKER_PROOF_SIZE))
        .map(|(st, p)| match *st {
            CPX_OK => Ok(p.try_into().unwrap()),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            st => panic!("libcpx: {}", st),
        })
        .collect()
}

/// whisk.rs:45-55 `WhiskTracker::from_k_r` and whisk.rs:370 `get_k_commitment` for many (k, r) pairs in one library call: the trackers and the
/// 48-byte commitments k_i G, in item order (every point is a multiple of the generator: one fixed-base kernel, no per-item call)
pub fn trackers_from_k_r(ks: &[Fr], rs: &[Fr]) -> (Vec<WhiskTracker>, Vec<[u8; 48]>) {
    assert!(ks.len() == rs.len());
    let count = ks.len();
    let mut trk = vec![0u8; 96 * count];
    let mut kc = vec![0u8; 48 * count];
    let rc = unsafe { cpx_whisk_trackers_from_k_r(ctx(), count, scalars_ptr(ks), scalars_ptr(rs), trk.as_mut_ptr(), kc.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    let trackers = trk.chunks(96).map(|c| WhiskTracker { r_G: c[..48].try_into().unwrap(), k_r_G: c[48..].try_into().unwrap() }).collect();
    (trackers, kc.chunks(48).map(|c| c.try_into().unwrap()).collect())
}

/// Which of `ks` opens each tracker: the relation of whisk.rs:36-55, `k * r_G == k_r_G`, for every (tracker, key) pair in one library call.
/// Per tracker `Ok(Some(j))` with the smallest such j, `Ok(None)` when no key opens it, `Err` when one of its halves does not decode.
pub fn find_whisk_trackers(trackers: &[WhiskTracker], ks: &[Fr]) -> Vec<Result<Option<usize>, SerializationError>> {
    let n = trackers.len();
    let wire = trackers_to_wire(trackers);
    let mut owner = vec![CPX_NO_OWNER; n];
    let mut status = vec![CPX_ERR_INTERNAL; n]; // an entry the library does not write is never read as an owner
    let rc = unsafe { cpx_whisk_find_trackers(ctx(), n, wire.as_ptr(), ks.len(), scalars_ptr(ks), owner.as_mut_ptr(), status.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    owner
        .iter()
        .zip(status.iter())
        .map(|(&o, &st)| match st {
            CPX_OK => Ok(if o == CPX_NO_OWNER { None } else { Some(o as usize) }),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            other => panic!("libcpx: {}", other),
        })
        .collect()
}

/// whisk.rs:370 `get_k_commitment` for many k in one library call
pub fn k_commitments(ks: &[Fr]) -> Vec<[u8; 48]> {
    let mut kc = vec![0u8; 48 * ks.len()];
    let rc = unsafe { cpx_g1_generator_mul(ctx(), ks.len(), scalars_ptr(ks), std::ptr::null_mut(), kc.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    kc.chunks(48).map(|c| c.try_into().unwrap()).collect()
}

/// whisk.rs:106-130 for many (pre_trackers, post_trackers, proof) triples in one library call: one result per item, in order.  Like the
/// rest of this file, NOT COMPILED here.
pub fn are_valid_whisk_shuffle_proofs<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    pre_trackers: &[&[WhiskTracker]],
    post_trackers: &[&[WhiskTracker]],
    proofs: &[WhiskShuffleProofBytes],
) -> Vec<Result<bool, SerializationError>> {
    assert!(pre_trackers.len() == post_trackers.len() && pre_trackers.len() == proofs.len());
    assert!(pre_trackers.iter().chain(post_trackers.iter()).all(|t| t.len() == ELL));
    let count = proofs.len();
    let factors = nonzero_factors(8 * count, rng); // the accumulate_check draws of every CurdleproofsProof::verify, in item order
    let pre: Vec<u8> = pre_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let post: Vec<u8> = post_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let pf: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let mut verdict = vec![CPX_ERR_INTERNAL; count]; // an entry the library does not write is never read as accepted
    let rc = unsafe { cpx_whisk_verify_shuffle_proofs(ctx_with_crs(crs), count, pre.as_ptr(), post.as_ptr(), pf.as_ptr(), scalars_ptr(&factors), verdict.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    verdict
        .into_iter()
        .map(|v| match v {
            CPX_OK => Ok(true),
            CPX_ERR_VERIFY => Ok(false),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            v => panic!("libcpx: {}", v),
        })
        .collect()
}

/// The same through the grouped form of the accumulated check (cpx_whisk_verify_shuffle_proofs_grouped, 12 factors per item): close to the
/// rate of the all-or-nothing fused check while few items are wrong.  Also returns how many items went through a check of their own.
pub fn are_valid_whisk_shuffle_proofs_grouped<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    pre_trackers: &[&[WhiskTracker]],
    post_trackers: &[&[WhiskTracker]],
    proofs: &[WhiskShuffleProofBytes],
) -> (Vec<Result<bool, SerializationError>>, usize) {
    assert!(pre_trackers.len() == post_trackers.len() && pre_trackers.len() == proofs.len());
    assert!(pre_trackers.iter().chain(post_trackers.iter()).all(|t| t.len() == ELL));
    let count = proofs.len();
    let factors = nonzero_factors(12 * count, rng); // per item the eight accumulate_check draws, then four weights for the SameScalar equalities
    let pre: Vec<u8> = pre_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let post: Vec<u8> = post_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let pf: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let mut verdict = vec![CPX_ERR_INTERNAL; count];
    let mut rechecked: usize = 0;
    let rc = unsafe {
        cpx_whisk_verify_shuffle_proofs_grouped(ctx_with_crs(crs), count, pre.as_ptr(), post.as_ptr(), pf.as_ptr(), scalars_ptr(&factors), verdict.as_mut_ptr(), &mut rechecked)
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    let res = verdict
        .into_iter()
        .map(|v| match v {
            CPX_OK => Ok(true),
            CPX_ERR_VERIFY => Ok(false),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            v => panic!("libcpx: {}", v),
        })
        .collect();
    (res, rechecked)
}

/// Makes `candidates` the resident candidate list of the context (decoded once on the device); one decoder status per candidate, 0 = fine.
/// An undecodable candidate is no error here: every item of a run that reads it is Err(SerializationError), as in whisk.rs:106-130.
pub fn load_candidate_trackers(crs: &CurdleproofsCrs, candidates: &[WhiskTracker]) -> Vec<u8> {
    let wire = trackers_to_wire(candidates);
    let mut status = vec![0u8; candidates.len()];
    let rc = unsafe { cpx_whisk_candidates_load(ctx_with_crs(crs), candidates.len(), wire.as_ptr(), status.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    status
}

/// whisk.rs:106-130 for a run of shuffles over the resident list in one library call: item b reads the candidates at `indices[b]` of the
/// list as it stands after items 0..b-1 were written back (whatever their results) and `post_trackers[b]` go back to the same indices.
/// Returns one result per item and n_applied: the leading accepted items, and no others, have been written back to the resident list.
pub fn verify_whisk_shuffle_run<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    indices: &[&[u32]],
    post_trackers: &[&[WhiskTracker]],
    proofs: &[WhiskShuffleProofBytes],
) -> (Vec<Result<bool, SerializationError>>, usize) {
    assert!(indices.len() == post_trackers.len() && indices.len() == proofs.len());
    assert!(indices.iter().all(|t| t.len() == ELL) && post_trackers.iter().all(|t| t.len() == ELL));
    let count = proofs.len();
    let factors = nonzero_factors(8 * count, rng);
    let idx: Vec<u32> = indices.iter().flat_map(|t| t.iter().copied()).collect();
    let post: Vec<u8> = post_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let pf: Vec<u8> = proofs.iter().flat_map(|p| p.iter().copied()).collect();
    let mut verdict = vec![CPX_ERR_INTERNAL; count];
    let mut applied: usize = 0;
    let rc = unsafe {
        cpx_whisk_verify_shuffle_run(ctx_with_crs(crs), count, idx.as_ptr(), post.as_ptr(), pf.as_ptr(), scalars_ptr(&factors), verdict.as_mut_ptr(), &mut applied)
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    let res = verdict
        .into_iter()
        .map(|v| match v {
            CPX_OK => Ok(true),
            CPX_ERR_VERIFY => Ok(false),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            v => panic!("libcpx: {}", v),
        })
        .collect();
    (res, applied)
}

/// whisk.rs:144-179 for many lists of pre trackers in one library call; every item draws from `rng` in the single function's order
/// (shuffle, k, blinders, the prover's 3n+9), item after item
pub fn generate_whisk_shuffle_proofs<T: RngCore>(
    rng: &mut T,
    crs: &CurdleproofsCrs,
    pre_trackers: &[&[WhiskTracker]],
) -> Vec<Result<(Vec<WhiskTracker>, WhiskShuffleProofBytes), SerializationError>> {
    assert!(pre_trackers.iter().all(|t| t.len() == ELL));
    let count = pre_trackers.len();
    let (mut permutation, mut k, mut blinders, mut rand) = (Vec::<u32>::new(), Vec::<Fr>::new(), Vec::<Fr>::new(), Vec::<Fr>::new());
    for _ in 0..count {
        let mut p: Vec<u32> = (0..ELL as u32).collect();
        p.shuffle(rng);
        permutation.extend(p);
        k.push(Fr::rand(rng));
        blinders.extend(generate_blinders(rng, N_BLINDERS));
        rand.extend((0..3 * N + 9).map(|_| Fr::rand(rng)));
    }
    let pre: Vec<u8> = pre_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let mut post = vec![0u8; 96 * ELL * count];
    let mut proofs = vec![0u8; WHISK_SHUFFLE_PROOF_SIZE * count];
    let mut status = vec![CPX_ERR_INTERNAL; count];
    let rc = unsafe {
        cpx_whisk_generate_shuffle_proofs(ctx_with_crs(crs), count, pre.as_ptr(), permutation.as_ptr(), scalars_ptr(&k), scalars_ptr(&blinders), scalars_ptr(&rand),
                                          post.as_mut_ptr(), proofs.as_mut_ptr(), status.as_mut_ptr())
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    status
        .iter()
        .zip(post.chunks(96 * ELL).zip(proofs.chunks(WHISK_SHUFFLE_PROOF_SIZE)))
        .map(|(st, (t, p))| match *st {
            CPX_OK => Ok((t.chunks(96).map(|c| WhiskTracker { r_G: c[..48].try_into().unwrap(), k_r_G: c[48..].try_into().unwrap() }).collect(), p.try_into().unwrap())),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            st => panic!("libcpx: {}", st),
        })
        .collect()
}

/// util.rs:83-106 for many instances in one library call (wire forms of ffi.rs: affine 96 B, Jacobian 144 B); the instances stay loaded
pub fn shuffle_permute_and_commit_inputs(crs: &CurdleproofsCrs, vec_r: &[u8], vec_s: &[u8], permutations: &[u32], k: &[Fr], vec_m_blinders: &[Fr]) -> (Vec<u8>, Vec<u8>, Vec<u8>) {
    let count = k.len();
    assert!(vec_r.len() == count * ELL * AFF && vec_s.len() == vec_r.len() && permutations.len() == count * ELL && vec_m_blinders.len() == count * N_BLINDERS);
    let (mut t, mut u, mut m) = (vec![0u8; vec_r.len()], vec![0u8; vec_r.len()], vec![0u8; JAC * count]);
    let rc = unsafe {
        cpx_batch_shuffle(ctx_with_crs(crs), count, vec_r.as_ptr(), vec_s.as_ptr(), permutations.as_ptr(), scalars_ptr(k), scalars_ptr(vec_m_blinders), t.as_mut_ptr(),
                          u.as_mut_ptr(), m.as_mut_ptr())
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    (t, u, m)
}

/// whisk.rs:144-179 for many lists of pre trackers with the draws made ON THE DEVICE (cpx_whisk_generate_shuffle_proofs_rng): `rng` is a
/// `ChaCha12Rng` (rand 0.8 `StdRng` is one), every item gets a stream of its own split off it (`ChaCha12Rng::from_rng`, done by
/// cpx_rng_split), and 40 bytes per item cross the bus instead of the draws.  With ONE item and its state taken from `rng` itself
/// (`rng_state` / `rng_resume` of ffi.rs instead of the split) the bytes are those of the crate's function on the same `rng`.
/// Never hand two items the same state: identical states draw identical witnesses.  Like the rest of this file, NOT COMPILED here.
pub fn generate_whisk_shuffle_proofs_on_device(
    rng: &mut rand_chacha::ChaCha12Rng,
    crs: &CurdleproofsCrs,
    pre_trackers: &[&[WhiskTracker]],
) -> Vec<Result<(Vec<WhiskTracker>, WhiskShuffleProofBytes), SerializationError>> {
    assert!(pre_trackers.iter().all(|t| t.len() == ELL));
    let count = pre_trackers.len();
    let mut parent = rng_state(rng);
    let mut states = vec![0u8; RNG_STATE * count];
    let rc = unsafe { cpx_rng_split(parent.as_mut_ptr(), count, states.as_mut_ptr()) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    rng_resume(rng, &parent);
    let pre: Vec<u8> = pre_trackers.iter().flat_map(|t| trackers_to_wire(t)).collect();
    let mut post = vec![0u8; 96 * ELL * count];
    let mut proofs = vec![0u8; WHISK_SHUFFLE_PROOF_SIZE * count];
    let mut status = vec![CPX_ERR_INTERNAL; count];
    let rc = unsafe {
        cpx_whisk_generate_shuffle_proofs_rng(ctx_with_crs(crs), count, pre.as_ptr(), states.as_mut_ptr(), post.as_mut_ptr(), proofs.as_mut_ptr(), status.as_mut_ptr())
    };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    status
        .iter()
        .zip(post.chunks(96 * ELL).zip(proofs.chunks(WHISK_SHUFFLE_PROOF_SIZE)))
        .map(|(st, (t, p))| match *st {
            CPX_OK => Ok((t.chunks(96).map(|c| WhiskTracker { r_G: c[..48].try_into().unwrap(), k_r_G: c[48..].try_into().unwrap() }).collect(), p.try_into().unwrap())),
            CPX_ERR_DESERIALIZE => Err(SerializationError::InvalidData),
            st => panic!("libcpx: {}", st),
        })
        .collect()
}

/// `Fr::rand(rng)` n times on the device, `rng` advanced as the crate would have advanced it: the verifier's factors, tracker blinders
pub fn fr_rand_on_device(rng: &mut rand_chacha::ChaCha12Rng, n: usize) -> Vec<Fr> {
    let mut state = rng_state(rng);
    let mut out = vec![Fr::from(0u64); n];
    let rc = unsafe { cpx_rng_fr(ctx(), 1, state.as_mut_ptr(), n, out.as_mut_ptr() as *mut u8) };
    assert!(rc == CPX_OK, "libcpx: {}", rc);
    rng_resume(rng, &state);
    out
}
