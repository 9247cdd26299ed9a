// Whisk byte-level API (/root/reference/src/whisk.rs) on top of the engine — product code.
//
// Host glue only: every group operation below is a call into the device engine (decompression + subgroup check,
// scalar multiplications, MSMs, the batch prover / verifier, normalisation + compression); the host hashes the
// six-point transcript of the tracker proofs and moves bytes.  Randomness stays with the caller (SURVEY 8b RNG
// contract): every `Fr::rand(rng)` / `shuffle(rng)` the reference performs is an argument, in the reference's order.
#include <algorithm>
#include <cstring>
#include <vector>
#include "engine.hpp"
#include "find_plan.hpp"
#include "run_plan.hpp"

namespace cpx {

using host::S;
using host::Transcript;

namespace {
const uint8_t GEN_COMP[48] = CPX_G1_GENERATOR_COMPRESSED;   // (kernels.h)

struct DeserializeError {};   // ark_serialize::SerializationError

void jac_from_aff(const Aff* a, size_t n, std::vector<Jac>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) out[i] = Jac::from_affine(a[i]);
}
}  // namespace

const Aff& Engine::generator() {
  if (!have_gen_) {
    if (decompress(GEN_COMP, 1, reinterpret_cast<uint8_t*>(&gen_), 1) != CPX_OK) throw std::logic_error("generator decoding");
    have_gen_ = true;
  }
  return gen_;
}

// affine points -> 48-byte compressed encodings (G1Affine::serialize_compressed)
void Engine::compress_affine(const Aff* pts, size_t n, uint8_t* out) {
  std::vector<Jac> j;
  jac_from_aff(pts, n, j);
  normalize(reinterpret_cast<const uint8_t*>(j.data()), n, nullptr, out);
}

// whisk.rs:265-277 unzip_trackers: r_G (48 B) || k_r_G (48 B) per tracker -> two affine vectors; false on a bad encoding
bool Engine::unzip_trackers(const uint8_t* trackers, size_t n, std::vector<Aff>& vec_r, std::vector<Aff>& vec_s) {
  std::vector<Aff> both(2 * n);
  if (decompress(trackers, 2 * n, reinterpret_cast<uint8_t*>(both.data()), 1) != CPX_OK) return false;
  vec_r.resize(n);
  vec_s.resize(n);
  for (size_t i = 0; i < n; i++) {
    vec_r[i] = both[2 * i];
    vec_s[i] = both[2 * i + 1];
  }
  return true;
}

// whisk.rs:144-179 generate_whisk_shuffle_proof (+ util.rs:83-106 shuffle_permute_and_commit_input)
int Engine::whisk_generate_shuffle_proof(const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                                         const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proof_out) {
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_, n = n_;
  std::vector<Aff> vec_r, vec_s;
  if (!unzip_trackers(pre_trackers, ell, vec_r, vec_s)) return CPX_ERR_DESERIALIZE;
  // vec_T = permute(k * vec_R), vec_U = permute(k * vec_S)   (util.rs:94-97)
  std::vector<Aff> kr(ell), ks(ell), vec_t(ell), vec_u(ell);
  scale(reinterpret_cast<const uint8_t*>(vec_r.data()), k, 0, ell, reinterpret_cast<uint8_t*>(kr.data()));
  scale(reinterpret_cast<const uint8_t*>(vec_s.data()), k, 0, ell, reinterpret_cast<uint8_t*>(ks.data()));
  for (size_t i = 0; i < ell; i++) {
    vec_t[i] = kr[permutation[i]];
    vec_u[i] = ks[permutation[i]];
  }
  // M = msm(vec_G, sigma) + msm(vec_H, blinders)   (util.rs:99-104)
  std::vector<Fr> sc(n);
  for (size_t i = 0; i < ell; i++) sc[i] = S::from_u64(permutation[i]).f;
  memcpy(&sc[ell], vec_m_blinders, 4 * sizeof(Fr));
  Jac M;
  msm(reinterpret_cast<const uint8_t*>(crs_host_.data()), reinterpret_cast<const uint8_t*>(sc.data()), n, reinterpret_cast<uint8_t*>(&M));
  // CurdleproofsProof::new
  batch_load(1, reinterpret_cast<const uint8_t*>(vec_r.data()), reinterpret_cast<const uint8_t*>(vec_s.data()), reinterpret_cast<const uint8_t*>(vec_t.data()),
             reinterpret_cast<const uint8_t*>(vec_u.data()), reinterpret_cast<const uint8_t*>(&M));
  batch_prove(permutation, k, vec_m_blinders, rand, proof_out + 48);
  normalize(reinterpret_cast<const uint8_t*>(&M), 1, nullptr, proof_out);   // WhiskShuffleProof::serialize: M first (whisk.rs:87-91)
  // zip_trackers (whisk.rs:279-293)
  std::vector<Aff> zipped(2 * ell);
  for (size_t i = 0; i < ell; i++) {
    zipped[2 * i] = vec_t[i];
    zipped[2 * i + 1] = vec_u[i];
  }
  compress_affine(zipped.data(), 2 * ell, post_trackers_out);
  return CPX_OK;
}

// whisk.rs:106-130 is_valid_whisk_shuffle_proof
int Engine::whisk_is_valid_shuffle_proof(const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proof, const uint8_t* rand, int* valid) {
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_;
  *valid = 0;
  std::vector<Aff> vec_r, vec_s, vec_t, vec_u;
  if (!unzip_trackers(pre_trackers, ell, vec_r, vec_s) || !unzip_trackers(post_trackers, ell, vec_t, vec_u)) return CPX_ERR_DESERIALIZE;
  Aff m_aff;
  if (decompress(proof, 1, reinterpret_cast<uint8_t*>(&m_aff), 1) != CPX_OK) return CPX_ERR_DESERIALIZE;   // G1Projective::deserialize_compressed
  const Jac M = Jac::from_affine(m_aff);
  batch_load(1, reinterpret_cast<const uint8_t*>(vec_r.data()), reinterpret_cast<const uint8_t*>(vec_s.data()), reinterpret_cast<const uint8_t*>(vec_t.data()),
             reinterpret_cast<const uint8_t*>(vec_u.data()), reinterpret_cast<const uint8_t*>(&M));
  int verdict = CPX_ERR_INTERNAL;
  batch_verify(proof + 48, rand, &verdict);
  if (verdict == CPX_ERR_DESERIALIZE) return CPX_ERR_DESERIALIZE;   // CurdleproofsProof::deserialize failed: Err(SerializationError)
  *valid = verdict == CPX_OK ? 1 : 0;                               // .verify(...).is_ok()
  return CPX_OK;
}

namespace {
// the six-point transcript of both tracker-proof functions (whisk.rs:204-218, :243-257)
S tracker_challenge(const uint8_t comp6[6 * 48]) {
  Transcript tr("whisk_opening_proof");
  for (int i = 0; i < 6; i++) tr.append_point_bytes("tracker_opening_proof", comp6 + 48 * i);
  return tr.get_and_append_challenge("tracker_opening_proof_challenge");
}
}  // namespace

// whisk.rs:228-263 generate_whisk_tracker_proof; `blinder` is the function's one Fr::rand draw
int Engine::whisk_generate_tracker_proof(const uint8_t tracker[96], const uint8_t k[32], const uint8_t blinder[32], uint8_t proof_out[128]) {
  Aff tr[2];   // r_G, k_r_G
  if (decompress(tracker, 2, reinterpret_cast<uint8_t*>(tr), 1) != CPX_OK) return CPX_ERR_DESERIALIZE;
  const Aff& G = generator();
  // k_G = k G, A = blinder G, B = blinder r_G
  const Aff bases[3] = {G, G, tr[0]};
  uint8_t scal[3 * 32];
  memcpy(scal, k, 32);
  memcpy(scal + 32, blinder, 32);
  memcpy(scal + 64, blinder, 32);
  Aff out[3];
  scale(reinterpret_cast<const uint8_t*>(bases), scal, 32, 3, reinterpret_cast<uint8_t*>(out));
  const Aff six[6] = {out[0], G, tr[1], tr[0], out[1], out[2]};
  uint8_t comp[6 * 48];
  compress_affine(six, 6, comp);
  const S challenge = tracker_challenge(comp);
  S kk, bl;
  memcpy(kk.f.v, k, 32);
  memcpy(bl.f.v, blinder, 32);
  const S s = bl - challenge * kk;
  memcpy(proof_out, comp + 4 * 48, 96);   // A, B (TrackerProof::serialize_compressed, whisk.rs:69-73)
  s.to_le_bytes(proof_out + 96);
  return CPX_OK;
}

// whisk.rs:183-226 is_valid_whisk_tracker_proof
int Engine::whisk_is_valid_tracker_proof(const uint8_t tracker[96], const uint8_t k_commitment[48], const uint8_t proof[128], int* valid) {
  *valid = 0;
  S s;
  if (!S::from_le_bytes(proof + 96, &s)) return CPX_ERR_DESERIALIZE;   // TrackerProof::deserialize_compressed
  uint8_t comp5[5 * 48];
  memcpy(comp5, proof, 96);              // A, B
  memcpy(comp5 + 96, tracker + 48, 48);  // k_r_G
  memcpy(comp5 + 144, tracker, 48);      // r_G
  memcpy(comp5 + 192, k_commitment, 48); // k_G
  Aff pts[5];
  if (decompress(comp5, 5, reinterpret_cast<uint8_t*>(pts), 1) != CPX_OK) return CPX_ERR_DESERIALIZE;
  const Aff &A = pts[0], &B = pts[1], &k_r_G = pts[2], &r_G = pts[3], &k_G = pts[4];
  const Aff& G = generator();
  const Aff six[6] = {k_G, G, k_r_G, r_G, A, B};
  uint8_t comp[6 * 48];
  compress_affine(six, 6, comp);   // the canonical encodings the reference hashes (serialize_compressed of the decoded points)
  const S challenge = tracker_challenge(comp);
  // A' = s G + c k_G,  B' = s r_G + c k_r_G
  const Aff ba[2] = {G, k_G}, bb[2] = {r_G, k_r_G};
  Fr sc[2] = {s.f, challenge.f};
  Jac res[2];
  msm(reinterpret_cast<const uint8_t*>(ba), reinterpret_cast<const uint8_t*>(sc), 2, reinterpret_cast<uint8_t*>(&res[0]));
  msm(reinterpret_cast<const uint8_t*>(bb), reinterpret_cast<const uint8_t*>(sc), 2, reinterpret_cast<uint8_t*>(&res[1]));
  uint8_t got[2 * 48];
  normalize(reinterpret_cast<const uint8_t*>(res), 2, nullptr, got);
  *valid = (memcmp(got, comp + 4 * 48, 96) == 0) ? 1 : 0;
  return CPX_OK;
}

// ---------------------------------------------------------------- tracker proofs, `count` per call (tracker.hip)
// Both calls: the inputs go up once, a constant number of kernels runs whatever the count, the results come down and the stream is
// synchronised once.  (The very first call of a context also decodes the generator: Engine::generator.)  Scratch is the tier-0 set.
namespace {
constexpr size_t kTrackerBatchMax = (size_t)1 << 23;   // 32-bit byte offsets into the uploaded inputs (272 B per proof) and int grids
}

// encoding j < planes * count of the decoder = the point at byte plane_off[j / count] + rec * (j % count) of the uploaded inputs:
// plane-major, so that every family of points (all r_G, all A, ...) is one dense array for the kernels behind the decoder
static void tracker_point_offsets(size_t count, const size_t* plane_off, const size_t* plane_rec, int planes, std::vector<uint32_t>& off) {
  off.resize((size_t)planes * count);
  for (int pl = 0; pl < planes; pl++)
    for (size_t i = 0; i < count; i++) off[(size_t)pl * count + i] = (uint32_t)(plane_off[pl] + plane_rec[pl] * i);
}
// n trackers (r_G || k_r_G, 96 bytes each) -> d_pts = every r_G, then every k_r_G, with the decoder's verdict per point in d_status: the
// upload (strict_infinity = 0 applied) and ONE k_decompress, inside the caller's scope.  `canon`, `off`: the caller's, declared above it
void Engine::decode_tracker_planes(size_t n, const uint8_t* trackers, std::vector<uint8_t>& canon, std::vector<uint32_t>& off, uint8_t* d_bytes, uint32_t* d_off,
                                   Aff* d_pts, uint8_t* d_status) {
  trackers = canonical_infinities(trackers, 96 * n, n, 96, {0, 48}, canon);
  const size_t plane_off[2] = {0, 48}, plane_rec[2] = {96, 96};
  tracker_point_offsets(n, plane_off, plane_rec, 2, off);
  CPX_HIP(hipMemcpyAsync(d_bytes, trackers, 96 * n, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_off, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  tick("k_decompress", 0, 2.0 * n);
  launch_decompress(opt_, d_bytes, (int)(2 * n), d_pts, nullptr, d_status, 1, stream_, d_off);
  tock();
}

// What every batched tracker verifier begins with, inside the caller's scope (`h`: the caller's, declared above it): the inputs with
// strict_infinity = 0 applied go up as tracker_input_layout (tracker_check_plan.hpp) says, k_decompress leaves the five planes A, B, k_r_G,
// r_G, k_G and k_tracker_challenge every item's challenge and clear flag.  t0_.dig holds the decoder's offsets (5 count words).
Engine::TrackerFront Engine::tracker_front(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, TrackerFrontHost& h) {
  trackers = canonical_infinities(trackers, 96 * count, count, 96, {0, 48}, h.canon[0]);
  k_commitments = canonical_infinities(k_commitments, 48 * count, count, 48, {0}, h.canon[1]);
  proofs = canonical_infinities(proofs, 128 * count, count, 128, {0, 48}, h.canon[2]);
  const int n = (int)count;
  const TrackerInputLayout in = tracker_input_layout(count);
  DevBuf<uint8_t>&din = t0_.bytes, &dst = t0_.status;   // trackers | k_commitments | proofs; 5 count decoding verdicts | count proof flags
  DevBuf<uint32_t>& doff = t0_.dig;
  DevBuf<Aff>& dpts = t0_.a0;
  DevBuf<Fr>& dchal = t0_.fr;
  din.ensure(in.bytes);
  dst.ensure(6 * count);
  doff.ensure(TCK_PLANES * count);
  dpts.ensure(TCK_PLANES * count);
  dchal.ensure(count);
  // the five points of proof i are read where they lie: A, B inside the proof, k_r_G, r_G inside the tracker, k_G
  tracker_point_offsets(count, in.plane_off, in.plane_rec, TCK_PLANES, h.off);
  CPX_HIP(hipMemcpyAsync(din.p + in.trackers, trackers, 96 * count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(din.p + in.k_commitments, k_commitments, 48 * count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(din.p + in.proofs, proofs, 128 * count, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(doff.p, h.off.data(), h.off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  uint8_t* d_bad = dst.p + TCK_PLANES * count;
  tick("k_decompress", 0, 5.0 * count);
  launch_decompress(opt_, din.p, TCK_PLANES * n, dpts.p, nullptr, dst.p, 1, stream_, doff.p);
  tock();
  tick("k_tracker_challenge", 288.0 * count, (double)count);
  launch_tracker_challenge_verify(din.p, dst.p, n, dchal.p, d_bad, stream_);
  tock();
  return TrackerFront{din.p + in.proofs, d_bad, dpts.p, dchal.p};
}

// whisk.rs:183-226 is_valid_whisk_tracker_proof for every (tracker, k_commitment, proof) triple
void Engine::whisk_verify_tracker_proofs(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, int* verdict) {
  for (size_t i = 0; i < count; i++) verdict[i] = CPX_ERR_INTERNAL;   // an entry the device never wrote is never read as accepted
  if (!count) return;
  if (count > kTrackerBatchMax) throw ArgError("tracker proofs: at most 2^23 per call");
  const Aff G = generator();   // (before the scope: the first call decodes the generator, a tier-0 call of its own, and scopes do not nest)
  TrackerFrontHost host;
  CallScope call(this);
  DevBuf<int>& dver = t0_.flag;
  dver.ensure(count);
  CPX_HIP(hipMemsetAsync(dver.p, 0xff, count * sizeof(int), stream_));   // (-1: not CPX_OK)
  const TrackerFront f = tracker_front(count, trackers, k_commitments, proofs, host);
  tick("k_tracker_relations", 0, 2.0 * count);
  launch_tracker_relations(f.pts, f.d_prf, f.chal, f.d_bad, G, (int)count, dver.p, stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(verdict, dver.p, count * sizeof(int), hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// whisk.rs:228-263 generate_whisk_tracker_proof for every (tracker, k, blinder) triple
void Engine::whisk_generate_tracker_proofs(size_t count, const uint8_t* trackers, const uint8_t* k, const uint8_t* blinders, uint8_t* proofs_out, int* status) {
  for (size_t i = 0; i < count; i++) status[i] = CPX_ERR_INTERNAL;
  if (!count) return;
  if (count > kTrackerBatchMax) throw ArgError("tracker proofs: at most 2^23 per call");
  const Aff G = generator();   // (before the scope, as above)
  std::vector<uint8_t> canon;
  std::vector<Aff> g;
  std::vector<uint32_t> off;
  SmulTask tasks[3];
  CallScope call(this);
  const int n = (int)count;
  DevBuf<uint8_t>&db = t0_.bytes, &dst = t0_.status;   // trackers | k_G, A, B compressed | proofs
  DevBuf<uint32_t>& doff = t0_.dig;
  DevBuf<Aff>&dtr = t0_.a0, &dout = t0_.a1, &dgen = t0_.gen;   // r_G | k_r_G; k G | blinder G | blinder r_G
  DevBuf<Fr>& dsc = t0_.fr;                                    // k | blinder
  DevBuf<SmulTask>& dtask = t0_.stask;
  DevBuf<int>& dver = t0_.flag;
  db.ensure(368 * count);
  dst.ensure(2 * count);
  doff.ensure(2 * count);
  dtr.ensure(2 * count);
  dout.ensure(3 * count);
  dsc.ensure(2 * count);
  dtask.ensure(3);
  dver.ensure(count);
  if (t0_.gen_n < count) {   // grows with the largest call; filled once
    dgen.ensure(count);
    g.assign(count, G);
    CPX_HIP(hipMemcpyAsync(dgen.p, g.data(), count * sizeof(Aff), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipStreamSynchronize(stream_));   // (gen_n counts copies that have arrived; only when the buffer grows)
    t0_.gen_n = count;
  }
  uint8_t *d_trk = db.p, *d_comp = db.p + 96 * count, *d_prf = db.p + 240 * count;
  const uint32_t fl = smul_flag();
  tasks[0] = SmulTask{nullptr, dgen.p, dout.p, dsc.p, 1, fl};                              // k_G = k G
  tasks[1] = SmulTask{nullptr, dgen.p, dout.p + count, dsc.p + count, 1, fl};              // A = blinder G
  tasks[2] = SmulTask{nullptr, dtr.p, dout.p + 2 * count, dsc.p + count, 1, fl};           // B = blinder r_G
  CPX_HIP(hipMemcpyAsync(dsc.p, k, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dsc.p + count, blinders, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(dtask.p, tasks, sizeof tasks, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemsetAsync(dver.p, 0xff, count * sizeof(int), stream_));
  CPX_HIP(hipMemsetAsync(d_prf, 0, 128 * count, stream_));
  decode_tracker_planes(count, trackers, canon, off, d_trk, doff.p, dtr.p, dst.p);
  smul_tasks(dtask.p, 3, count, 3.0 * count);
  tick("k_compress", 0, 3.0 * count);
  launch_compress(dout.p, 3 * n, 3 * n, 1, d_comp, stream_);
  tock();
  tick("k_tracker_challenge", 288.0 * count, (double)count);
  launch_tracker_challenge_prove(d_trk, d_comp, dst.p, dsc.p, dsc.p + count, n, d_prf, dver.p, stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(proofs_out, d_prf, 128 * count, hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(status, dver.p, count * sizeof(int), hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// ---------------------------------------------------------------- tracker proofs, grouped and fused: one MSM (tracker_check_plan.hpp)
// The verifier's two relations weighted by the caller's a_i, b_i and summed per group of items: after the decoding and the transcripts of
// the per-item call, k_tracker_check_scalars writes every group's task (the generator, then five points per item) and the device half of
// the tier-0 bucket MSM (msm_chain) leaves one sum per group.  Grouped: the sums come down with the flags — ONE synchronisation when every
// group sums to the identity; otherwise k_tracker_gather compacts the unflagged items of the failing groups and the per-item relations
// (launch_tracker_relations, unchanged) run on them: a second synchronisation.  Fused: k_sum_jac adds the sums and one point comes down.
// The number of launches never depends on the count.  Scratch is the tier-0 set.
void Engine::whisk_verify_tracker_proofs_grouped(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand,
                                                 int* verdict, size_t* n_rechecked) {
  if (!count) {
    if (n_rechecked) *n_rechecked = 0;
    return;
  }
  tracker_check(count, trackers, k_commitments, proofs, rand, verdict, n_rechecked, nullptr, nullptr);
}
void Engine::whisk_verify_tracker_proofs_fused(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand,
                                               uint8_t* partial_jac, int* n_invalid) {
  if (!count) {
    const Jac id = Jac::identity();
    memcpy(partial_jac, &id, sizeof id);
    *n_invalid = 0;
    return;
  }
  tracker_check(count, trackers, k_commitments, proofs, rand, nullptr, nullptr, partial_jac, n_invalid);
}
void Engine::tracker_check(size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                           size_t* n_rechecked, uint8_t* partial_jac, int* n_invalid) {
  if (!tracker_check_fits(count)) throw ArgError("tracker proofs, grouped / fused: at most 2^21 per call");
  for (size_t i = 0; i < 2 * count; i++)
    if (!host::is_valid_factor(rand + 32 * i)) throw ArgError("tracker check weights must be non-zero reduced field elements");
  const bool grouped = verdict != nullptr;
  if (grouped) {
    for (size_t i = 0; i < count; i++) verdict[i] = CPX_ERR_INTERNAL;   // an entry the device never wrote is never read as accepted
    if (n_rechecked) *n_rechecked = 0;
  }
  const Aff G = generator();   // (before the scope, as above)
  // the fused sum keeps the grouping of cpx_batch_verify_fused; the groups only shape the MSM there
  const TrackerCheckPlan tp = tracker_check_plan(count, grouped ? opt_.locate_groups_max : kLocateGroupsMax);
  const LocatePlan& lp = tp.lp;
  const size_t NT = tp.tasks();
  Tier0MsmPlan pl;
  pl.count = NT;
  pl.points = tp.points();
  pl.max_n = (uint32_t)tp.max_n();
  pl.conv_off.resize(NT);
  std::vector<uint32_t> lens(NT), list, flags;
  TrackerFrontHost host;
  for (size_t g = 0; g < NT; g++) {
    pl.conv_off[g] = (uint32_t)tp.task_off(g);
    lens[g] = (uint32_t)tp.task_n(g);
  }
  std::vector<MsmTask> tasks;
  std::vector<uint8_t> bad, group_ok, recheck_ok;
  std::vector<Jac> sums;
  std::vector<int> ver2;
  Jac total;
  int total_is_identity = 0;
  CallScope call(this);
  pl.slices = msm_tblw_slices(opt_, (int)NT, 2, (int)pl.max_n);
  const int n = (int)count;
  DevBuf<uint8_t>& dst = t0_.status;      // (the front's; stage 2 reuses it)
  DevBuf<uint32_t>& doff = t0_.dig;       // the decoder's offsets, then the chain's digits, then stage 2's list
  DevBuf<Aff>& dbase = t0_.tbase;
  DevBuf<Fr>&dscal = t0_.tscal, &dw = t0_.tw;
  DevBuf<Jac>&dsum = t0_.tres, &dtot = t0_.res;
  DevBuf<int>& dver = t0_.flag;
  msm_chain_reserve(pl);   // (first: ensure() may free a buffer, and the digits outgrow the front's 5 count offsets)
  dver.ensure(count);
  dbase.ensure(tp.points());
  dscal.ensure(tp.points());
  dw.ensure(tp.weight_scalars());
  dsum.ensure(tp.result_points());
  dtot.ensure(1);
  CPX_HIP(hipMemcpyAsync(dw.p, rand, 2 * count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  const TrackerFront f = tracker_front(count, trackers, k_commitments, proofs, host);
  const uint8_t *d_prf = f.d_prf, *d_bad = f.d_bad;
  tick("k_tracker_check_scalars", (double)(tp.points() * (sizeof(Aff) + sizeof(Fr))), (double)count);
  launch_tracker_check_scalars(f.pts, d_prf, f.chal, d_bad, dw.p, G, n, (int)lp.G, (int)NT, dbase.p, dscal.p, stream_);
  tock();
  msm_chain(pl, lens.data(), dbase.p, dscal.p, dsum.p, tasks);
  bad.resize(count);
  CPX_HIP(hipMemcpyAsync(bad.data(), d_bad, count, hipMemcpyDeviceToHost, stream_));
  if (!grouped) {
    launch_sum_jac(dsum.p, (int)NT, dtot.p, dver.p, stream_);
    CPX_HIP(hipMemcpyAsync(&total, dtot.p, sizeof(Jac), hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(&total_is_identity, dver.p, sizeof(int), hipMemcpyDeviceToHost, stream_));
    call.finish();
    int inv = 0;
    for (size_t i = 0; i < count; i++) inv += bad[i] ? 1 : 0;
    if (total_is_identity) total = Jac::identity();   // (one encoding of the identity whatever the chain left in X and Y)
    memcpy(partial_jac, &total, sizeof(Jac));
    *n_invalid = inv;
    return;
  }
  sums.resize(NT);
  CPX_HIP(hipMemcpyAsync(sums.data(), dsum.p, NT * sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  call.finish();   // the one synchronisation of a batch whose groups all pass
  group_ok.resize(NT);
  flags.resize(count);
  for (size_t g = 0; g < NT; g++) group_ok[g] = sums[g].is_identity() ? 1 : 0;
  for (size_t i = 0; i < count; i++) flags[i] = bad[i] ? kLocateFlagDecode : 0u;
  locate_stage2(lp, group_ok.data(), flags.data(), list);   // empty with one item per group: stage 1 was the per-item check
  const size_t S = list.size();
  if (S) {
    // the buffers of stage 1 that are dead by now take the dense arrays (the stream is idle: ensure() may free)
    DevBuf<Aff>& dpts2 = t0_.a1;
    dpts2.ensure(TrackerCheckPlan::s2_points(S));
    dst.ensure(TrackerCheckPlan::s2_proof_bytes(S) + S);
    uint32_t* d_list = doff.p;                                    // (9 points() words: S fits)
    uint8_t *d_prf2 = dst.p, *d_bad2 = dst.p + TrackerCheckPlan::s2_proof_bytes(S);
    Fr* d_chal2 = dw.p;                                           // (2 count scalars: S fit)
    CPX_HIP(hipMemcpyAsync(d_list, list.data(), S * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemsetAsync(dver.p, 0xff, S * sizeof(int), stream_));   // (-1: not CPX_OK)
    tick("k_tracker_gather", (double)(S * (5 * sizeof(Aff) + 128 + sizeof(Fr))), (double)S);
    launch_tracker_gather(d_list, (int)S, n, f.pts, d_prf, f.chal, dpts2.p, d_prf2, d_chal2, d_bad2, stream_);
    tock();
    tick("k_tracker_relations", 0, 2.0 * S);
    launch_tracker_relations(dpts2.p, d_prf2, d_chal2, d_bad2, G, (int)S, dver.p, stream_);
    tock();
    ver2.resize(S);
    CPX_HIP(hipMemcpyAsync(ver2.data(), dver.p, S * sizeof(int), hipMemcpyDeviceToHost, stream_));
    call.finish();
    recheck_ok.resize(S);
    for (size_t s = 0; s < S; s++) recheck_ok[s] = ver2[s] == CPX_OK ? 1 : 0;
  }
  locate_verdicts(lp, group_ok.data(), flags.data(), list, recheck_ok.data(), verdict);
  if (n_rechecked) *n_rechecked = S;
}

// ---------------------------------------------------------------- which trackers a set of keys opens (find.hip, find_plan.hpp)
// k_j * r_G_i == k_r_G_i (whisk.rs:36-55, the multiplication of whisk.rs:323) for every (tracker, key) pair: the trackers and the keys go up once,
// every point is decoded once, and either ONE k_smul + ONE k_find_compare run (few keys), or per chunk of trackers k_table_build + k_fix_build +
// k_find_scan (many keys) — the number of launches never depends on n_keys.  The owners and the decoding verdicts come down and the stream is
// synchronised once.  Scratch is the tier-0 set; the table and its build scratch live for the call only.
void Engine::whisk_find_trackers(size_t n_trackers, const uint8_t* trackers, size_t n_keys, const uint8_t* k, uint32_t* owner, int* status) {
  for (size_t i = 0; i < n_trackers; i++) {   // an entry the device never wrote is never read as an owner
    status[i] = CPX_ERR_INTERNAL;
    owner[i] = CPX_NO_OWNER;
  }
  if (!n_trackers) return;
  if (!find_fits(n_trackers, n_keys)) throw ArgError("find trackers: at most 2^23 trackers, 2^20 keys and 2^32 pairs per call");
  std::vector<uint32_t> off;
  std::vector<SmulTask> tasks;
  std::vector<uint8_t> st, canon;
  CallScope call(this);
  const FindPlan pl = find_plan(n_trackers, n_keys, opt_.find_table_min_keys, opt_.find_table_mb);
  const size_t n = n_trackers;
  DevBuf<uint8_t>&din = t0_.bytes, &dst = t0_.status;   // the trackers; decoding verdicts r_G plane | k_r_G plane
  DevBuf<uint32_t>& dwords = t0_.dig;                   // 2 n byte offsets of the encodings | n owners
  DevBuf<Aff>&dpts = t0_.a0, &dprod = t0_.a1;           // r_G | k_r_G decoded; ladder path: k_j r_G_i, key-major
  DevBuf<Fr>& dkeys = t0_.fr;
  DevBuf<SmulTask>& dtask = t0_.stask;
  din.ensure(96 * n);
  dst.ensure(2 * n);
  dwords.ensure(3 * n);
  dpts.ensure(2 * n);
  dkeys.ensure(std::max<size_t>(n_keys, 1));
  uint32_t* d_owner = dwords.p + 2 * n;
  const Aff *d_r = dpts.p, *d_claimed = dpts.p + n;
  if (n_keys) CPX_HIP(hipMemcpyAsync(dkeys.p, k, n_keys * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemsetAsync(d_owner, 0xff, n * sizeof(uint32_t), stream_));   // CPX_NO_OWNER
  decode_tracker_planes(n, trackers, canon, off, din.p, dwords.p, dpts.p, dst.p);
  DevBuf<TFix> tab;   // table path: one chunk's table, its shifted copies and the build scratch; released when the call ends
  DevBuf<TAff> shift;
  DevBuf<TblTmp> tmp;
  if (pl.table) {
    tab.ensure(FindPlan::table_entries(pl.chunk_cols));
    shift.ensure(FindPlan::shift_entries(pl.chunk_cols));
    tmp.ensure(FindPlan::tmp_entries(pl.chunk_cols, pl.fix_chunk));
    for (size_t c = 0; c < pl.n_chunks; c++) {
      const size_t first = pl.chunk_first(c), nc = pl.chunk_size(c);
      // copy w = 256^w r_G for the nc trackers of the chunk, then the multiples m 256^w r_G: the CRS table at fix_bits = 8, a tracker per column
      tick("k_table_build", 0, (double)nc);
      launch_table_build(opt_, d_r + first, 0, shift.p, 1, 0, (int)nc, (int)nc, FIND_WINDOWS, false, tmp.p, stream_, 8);
      tock();
      tick("k_fix_build", (double)(FindPlan::table_entries(nc) * sizeof(TFix)), (double)FindPlan::table_entries(nc));
      launch_fix_build(shift.p, (int)nc, 8, tab.p, tmp.p, pl.fix_chunk, stream_);
      tock();
      tick("k_find_scan", 32.0 * sizeof(TFix) * nc * n_keys, (double)nc * n_keys);
      launch_find_scan(pl, tab.p, nc, first, dkeys.p, d_claimed, dst.p, d_owner, stream_);
      tock();
    }
  } else if (n_keys) {
    dprod.ensure(n * n_keys);
    dtask.ensure(n_keys);
    // one task per key, the key shared by its n elements; the subgroup-checked decoding is what makes k_smul's endomorphism split valid
    const uint32_t fl = smul_flag();
    tasks.resize(n_keys);
    for (size_t j = 0; j < n_keys; j++) tasks[j] = SmulTask{nullptr, d_r, dprod.p + j * n, dkeys.p + j, 0, fl};
    CPX_HIP(hipMemcpyAsync(dtask.p, tasks.data(), tasks.size() * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
    smul_tasks(dtask.p, n_keys, n, (double)n * n_keys);
    tick("k_find_compare", (double)sizeof(Aff) * n * n_keys, (double)n * n_keys);
    launch_find_compare(dprod.p, d_claimed, dst.p, n, n_keys, d_owner, stream_);
    tock();
  }
  st.resize(2 * n);
  CPX_HIP(hipMemcpyAsync(owner, d_owner, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(st.data(), dst.p, 2 * n, hipMemcpyDeviceToHost, stream_));
  call.finish();
  for (size_t i = 0; i < n; i++) {
    const bool bad = st[i] != 0 || st[n + i] != 0;
    status[i] = bad ? CPX_ERR_DESERIALIZE : CPX_OK;
    if (bad) owner[i] = CPX_NO_OWNER;   // (the kernels mask by the verdicts; an identity left by a failed decode never matches)
  }
}

// ---------------------------------------------------------------- trackers and k commitments, `count` per call (genmul.hip)
// The objects the batched tracker calls consume: every one of them is a multiple of the generator — r G, k G and k (r G) = (k r mod r_order) G —
// so they come from the fixed-base table of G (gen_table.hpp): the scalars go up once, ONE k_gen_mul (the Fr product k r included) and ONE
// k_compress run whatever the count, the results come down and the stream is synchronised once.  The context's first call also decodes the
// generator and builds the table (one launch, once per context).  Scratch is the tier-0 set.
const TAff* Engine::generator_table() {
  if (!have_gen_tab_) {
    const Aff G = generator();
    CallScope call(this);   // (selects the device; the launch stays enqueued for the caller's own scope to wait for)
    gen_tab_.ensure(gen_table_entries());
    tick("k_gen_table", (double)(gen_table_entries() * sizeof(TAff)), (double)gen_table_entries());
    launch_gen_table(G, gen_tab_.p, stream_);
    tock();
    have_gen_tab_ = true;
  }
  return gen_tab_.p;
}

// out[i] = scalars[i] G (whisk.rs:318, :323 with g1 = the generator)
void Engine::generator_mul(size_t count, const uint8_t* scalars, uint8_t* out_affine, uint8_t* out_compressed) {
  if (!count || (!out_affine && !out_compressed)) return;
  if (count > kTrackerBatchMax) throw ArgError("generator multiples: at most 2^23 per call");
  const TAff* tab = generator_table();   // (before the scope and the buffers below: the first call decodes the generator in the same scratch)
  CallScope call(this);
  DevBuf<Fr>& dsc = t0_.fr;
  DevBuf<Aff>& dout = t0_.a0;
  DevBuf<uint8_t>& dcomp = t0_.bytes;
  dsc.ensure(count);
  dout.ensure(count);
  if (out_compressed) dcomp.ensure(48 * count);
  const int n = (int)count;
  CPX_HIP(hipMemcpyAsync(dsc.p, scalars, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  tick("k_gen_mul", 128.0 * count, (double)count);
  launch_gen_mul(dsc.p, nullptr, n, GEN_MUL_PLAIN, tab, dout.p, stream_);
  tock();
  if (out_compressed) {
    tick("k_compress", 0, (double)count);
    launch_compress(dout.p, n, n, 1, dcomp.p, stream_);
    tock();
    CPX_HIP(hipMemcpyAsync(out_compressed, dcomp.p, 48 * count, hipMemcpyDeviceToHost, stream_));
  }
  if (out_affine) CPX_HIP(hipMemcpyAsync(out_affine, dout.p, count * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// whisk.rs:45-55 WhiskTracker::from_k_r and whisk.rs:370 get_k_commitment for every (k, r) pair
void Engine::whisk_trackers_from_k_r(size_t count, const uint8_t* k, const uint8_t* r, uint8_t* trackers_out, uint8_t* k_commitments_out) {
  if (!count || (!trackers_out && !k_commitments_out)) return;
  if (count > kTrackerBatchMax) throw ArgError("trackers: at most 2^23 per call");
  const TAff* tab = generator_table();
  CallScope call(this);
  // points: r_0 G, k_0 r_0 G, r_1 G, ... (the trackers as they are serialised), then k_0 G, k_1 G, ...; without trackers only the latter
  const int mode = !trackers_out ? GEN_MUL_PLAIN : k_commitments_out ? GEN_MUL_BOTH : GEN_MUL_TRACKERS;
  const size_t points = count * (mode == GEN_MUL_PLAIN ? 1 : mode == GEN_MUL_TRACKERS ? 2 : 3);
  DevBuf<Fr>& dsc = t0_.fr;   // k | r
  DevBuf<Aff>& dout = t0_.a0;
  DevBuf<uint8_t>& dcomp = t0_.bytes;
  dsc.ensure(2 * count);
  dout.ensure(points);
  dcomp.ensure(48 * points);
  const int n = (int)count, np = (int)points;
  CPX_HIP(hipMemcpyAsync(dsc.p, k, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  if (trackers_out) CPX_HIP(hipMemcpyAsync(dsc.p + count, r, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  tick("k_gen_mul", 128.0 * points, (double)points);
  launch_gen_mul(dsc.p, dsc.p + count, n, mode, tab, dout.p, stream_);
  tock();
  tick("k_compress", 0, (double)points);
  launch_compress(dout.p, np, np, 1, dcomp.p, stream_);
  tock();
  if (trackers_out) CPX_HIP(hipMemcpyAsync(trackers_out, dcomp.p, 96 * count, hipMemcpyDeviceToHost, stream_));
  if (k_commitments_out) CPX_HIP(hipMemcpyAsync(k_commitments_out, dcomp.p + (trackers_out ? 96 * count : 0), 48 * count, hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// ---------------------------------------------------------------- shuffle step and shuffle proofs, `count` per call (shuffle.hip)
// All three calls: the inputs go up once; decoding, the placeholder rule, k R / k S, the gather, M and the compression are a constant number
// of launches whatever the count, on device-resident data; the count instances become the loaded batch through load_rows (device to device)
// and the batch prover / verifier runs on them unchanged.  The host touches bytes (offset table, task descriptors, the proof records'
// 48-byte prefix), never points.
namespace {
// every row must be a permutation of 0..ell (the reference shuffles (0..ELL)): the check of the single call (capi.cpp), before anything is launched
void check_permutations(size_t count, size_t ell, const uint32_t* permutation) {
  std::vector<uint8_t> seen(ell);
  for (size_t i = 0; i < count; i++) {
    std::fill(seen.begin(), seen.end(), 0);
    for (size_t j = 0; j < ell; j++) {
      const uint32_t p = permutation[i * ell + j];
      if (p >= ell || seen[p]) throw ArgError("permutation: every row must be a permutation of 0..ell");
      seen[p] = 1;
    }
  }
}
void shuffle_point_offsets(const ShufflePlan& pl, std::vector<uint32_t>& off) {
  off.resize(pl.points());
  for (size_t j = 0; j < off.size(); j++) off[j] = (uint32_t)pl.src_offset(j);
}
}  // namespace

// util.rs:94-104 on the device.  In: sh_.pts = vec_R | vec_S (dense planes), sh_.perm, sh_.fr = k [count] | blinders [count][4] | the scalars
// of M [count][n] (k_shuffle_status).  Out: sh_.tu = vec_T | vec_U, sh_.zip = (T_j, U_j) interleaved, the loaded batch (R, S, T, U, M) and the
// compressed M of every item in d_comp_.  Ends synchronised: the staging buffers and the task list (`tasks`: the caller's, declared above
// its scope) are free again.
void Engine::shuffle_device(const ShufflePlan& pl, std::vector<SmulTask>& tasks) {
  const size_t count = pl.count, ell = ell_, n = n_, pp = pl.plane_points();
  sh_.kpts.ensure(2 * pp);
  sh_.tu.ensure(2 * pp);
  sh_.zip.ensure(2 * pp);
  sh_.stask.ensure(2 * count);
  sh_.mjac.ensure(count);
  const Aff *d_r = sh_.pts.p + pl.point_index(SHP_R, 0, 0), *d_s = sh_.pts.p + pl.point_index(SHP_S, 0, 0);
  // k R, k S: one task per (item, family), the item's k shared by its ell elements
  const uint32_t fl = smul_flag();
  tasks.resize(2 * count);
  for (size_t i = 0; i < count; i++) {
    tasks[2 * i] = SmulTask{nullptr, d_r + i * ell, sh_.kpts.p + i * ell, sh_.fr.p + i, 0, fl};
    tasks[2 * i + 1] = SmulTask{nullptr, d_s + i * ell, sh_.kpts.p + pp + i * ell, sh_.fr.p + i, 0, fl};
  }
  CPX_HIP(hipMemcpyAsync(sh_.stask.p, tasks.data(), tasks.size() * sizeof(SmulTask), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemsetAsync(sh_.mjac.p, 0, count * sizeof(Jac), stream_));   // (Z = 0: the identity, until M is known)
  smul_tasks(sh_.stask.p, 2 * count, ell, 2.0 * pp);
  tick("k_shuffle_gather", 6.0 * sizeof(Aff) * pp, (double)pp);
  launch_shuffle_gather(pl, sh_.perm.p, sh_.kpts.p, sh_.kpts.p + pp, sh_.tu.p, sh_.tu.p + pp, sh_.zip.p, stream_);
  tock();
  load_rows(count, reinterpret_cast<const uint8_t*>(d_r), reinterpret_cast<const uint8_t*>(d_s), reinterpret_cast<const uint8_t*>(sh_.tu.p),
            reinterpret_cast<const uint8_t*>(sh_.tu.p + pp), reinterpret_cast<const uint8_t*>(sh_.mjac.p), true);
  // M = msm(vec_G, sigma) + msm(vec_H, blinders): vec_G | vec_H are the first n columns of the CRS tables — one fixed-base task per item
  const TblSeg none{nullptr, nullptr, 0, 0};
  const Fr* d_msc = sh_.fr.p + 5 * count;
  std::vector<TblReq> reqs(count);
  for (size_t i = 0; i < count; i++) reqs[i] = TblReq{cseg(0, (uint32_t)n), nullptr, none, nullptr, slot_index(i, SL_M), d_msc + i * n};
  enqueue_tbl_phase(reqs, slot_index(0, SlotMap(L_).TMP(7)), h_stage_, d_blob_, d_comp_, stream_, main_, true);
  tick("k_shuffle_commit", 0, (double)count);
  launch_shuffle_commit(d_pp_.p, pp_stride_, (uint32_t)(4 * ell + SL_M), (uint32_t)count, d_Mjac_.p, stream_);
  tock();
  CPX_HIP(hipStreamSynchronize(stream_));
}

// util.rs:83-106 shuffle_permute_and_commit_input for every instance
void Engine::shuffle_batch(size_t count, const uint8_t* vec_R, const uint8_t* vec_S, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                           uint8_t* vec_T_out, uint8_t* vec_U_out, uint8_t* M_out) {
  if (!count) return;
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_, n = n_;
  const ShufflePlan pl(count, ell, false);
  if (!pl.fits()) throw ArgError("shuffle batch: count * ell exceeds the 32-bit index range of one call");
  check_permutations(count, ell, permutation);
  std::vector<SmulTask> tasks;
  CallScope call(this);
  const size_t pp = pl.plane_points();
  sh_.pts.ensure(2 * pp);
  sh_.perm.ensure(pp);
  sh_.fr.ensure(5 * count + count * n);
  sh_.bad.ensure(count);
  CPX_HIP(hipMemcpyAsync(sh_.pts.p, vec_R, pp * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(sh_.pts.p + pp, vec_S, pp * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(sh_.perm.p, permutation, pp * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(sh_.fr.p, k, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(sh_.fr.p + count, vec_m_blinders, 4 * count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  tick("k_shuffle_status", 0, (double)count);
  launch_shuffle_status(pl, nullptr, sh_.pts.p, Aff::identity(), sh_.perm.p, sh_.fr.p + count, sh_.fr.p + 5 * count, nullptr, sh_.bad.p, stream_);
  tock();
  shuffle_device(pl, tasks);
  if (vec_T_out) CPX_HIP(hipMemcpyAsync(vec_T_out, sh_.tu.p, pp * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  if (vec_U_out) CPX_HIP(hipMemcpyAsync(vec_U_out, sh_.tu.p + pp, pp * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  if (M_out) CPX_HIP(hipMemcpyAsync(M_out, d_Mjac_.p, count * sizeof(Jac), hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// whisk.rs:144-179 generate_whisk_shuffle_proof for every (pre_trackers, permutation, k, blinders, draws) item
void Engine::whisk_generate_shuffle_proofs(size_t count, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                                           const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status) {
  whisk_generate_shuffle_proofs_with(count, pre_trackers, permutation, k, vec_m_blinders, rand, nullptr, post_trackers_out, proofs_out, status);
}
// The body.  states == null: the caller's draws are uploaded.  states != null (a batch the device-resident prover takes): k_rng_draw makes
// the permutation, k and the blinders where the shuffle step reads them, the prover that follows draws its 3n + 9 the same way, and only the
// 40-byte states cross the bus; an undecodable item gets its state as it stood after the shuffle and k (whisk.rs:150-157).
void Engine::whisk_generate_shuffle_proofs_with(size_t count, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders,
                                                const uint8_t* rand, uint8_t* states, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status) {
  for (size_t i = 0; i < count; i++) status[i] = CPX_ERR_INTERNAL;   // an entry the device never wrote is never read as a proof
  if (!count) return;
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_, n = n_, psz = proof_size(), rec = 48 + psz;
  const ShufflePlan pl(count, ell, false);
  if (!pl.fits()) throw ArgError("shuffle proofs: count * ell exceeds the 32-bit index range of one call");
  if (!states) check_permutations(count, ell, permutation);   // (a row k_rng_draw shuffled from 0..ell is one)
  const Aff G = generator();   // (before the scope, as above)
  const size_t pp = pl.plane_points();
  std::vector<uint32_t> off;
  std::vector<uint8_t> bad, dense, mid, end, canon;
  pre_trackers = canonical_infinities(pre_trackers, pp * 96, pp, 96, {0, 48}, canon);
  std::vector<SmulTask> tasks;
  CallScope call(this);
  sh_.bytes.ensure(pl.upload_bytes() + 2 * pp * 48);   // pre trackers | post trackers
  sh_.status.ensure(pl.points());
  sh_.off.ensure(pl.points());
  sh_.pts.ensure(pl.points());
  sh_.perm.ensure(pp);
  sh_.fr.ensure(5 * count + count * n);
  sh_.bad.ensure(count);
  shuffle_point_offsets(pl, off);
  CPX_HIP(hipMemcpyAsync(sh_.bytes.p, pre_trackers, pl.upload_bytes(), hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(sh_.off.p, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  if (states) {
    rng_.states.ensure(count * RNG_STATE_BYTES);
    rng_.mid.ensure(count * RNG_STATE_BYTES);
    rng_.perm.ensure(pp);
    rng_.kb.ensure(5 * count);
    mid.resize(count * RNG_STATE_BYTES);
    CPX_HIP(hipMemcpyAsync(rng_.states.p, states, count * RNG_STATE_BYTES, hipMemcpyHostToDevice, stream_));
    tick("k_rng_draw", (double)(pp * sizeof(uint32_t) + 5 * count * sizeof(Fr)), (double)(5 * count));
    launch_rng_draw(rng_draw_args(rng_.states.p, rng_.mid.p, count, ell, sh_.perm.p, {{1, sh_.fr.p}, {4, sh_.fr.p + count}}), stream_);
    tock();
    // the prover behind this scope reads them again: out of the scratch set, which the scope's end may trim
    CPX_HIP(hipMemcpyAsync(rng_.perm.p, sh_.perm.p, pp * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(rng_.kb.p, sh_.fr.p, 5 * count * sizeof(Fr), hipMemcpyDeviceToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(mid.data(), rng_.mid.p, mid.size(), hipMemcpyDeviceToHost, stream_));
  } else {
    CPX_HIP(hipMemcpyAsync(sh_.perm.p, permutation, pp * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(sh_.fr.p, k, count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(sh_.fr.p + count, vec_m_blinders, 4 * count * sizeof(Fr), hipMemcpyHostToDevice, stream_));
  }
  tick("k_decompress", 0, (double)pl.points());
  launch_decompress(opt_, sh_.bytes.p, (int)pl.points(), sh_.pts.p, nullptr, sh_.status.p, 1, stream_, sh_.off.p);
  tock();
  tick("k_shuffle_status", 0, (double)count);
  launch_shuffle_status(pl, sh_.status.p, sh_.pts.p, G, sh_.perm.p, sh_.fr.p + count, sh_.fr.p + 5 * count, nullptr, sh_.bad.p, stream_);
  tock();
  shuffle_device(pl, tasks);
  uint8_t* d_post = sh_.bytes.p + pl.upload_bytes();
  tick("k_compress", 0, 2.0 * pp);
  launch_compress(sh_.zip.p, (int)(2 * pp), (int)(2 * pp), 1, d_post, stream_);   // zip_trackers (whisk.rs:279-293)
  tock();
  bad.resize(count);
  CPX_HIP(hipMemcpyAsync(post_trackers_out, d_post, 2 * pp * 48, hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpy2DAsync(proofs_out, rec, d_comp_.p, 48, 48, count, hipMemcpyDeviceToHost, stream_));   // WhiskShuffleProof::serialize: M first (whisk.rs:87-91)
  CPX_HIP(hipMemcpyAsync(bad.data(), sh_.bad.p, count, hipMemcpyDeviceToHost, stream_));
  call.finish();
  // CurdleproofsProof::new on the loaded instances; the proofs come back dense and go behind their M
  dense.resize(count * psz);
  if (states) {
    end.resize(count * RNG_STATE_BYTES);
    batch_prove_device(ProveDraws{rng_.perm.p, reinterpret_cast<const uint8_t*>(rng_.kb.p), reinterpret_cast<const uint8_t*>(rng_.kb.p + count), hipMemcpyDeviceToDevice,
                                  nullptr, nullptr, end.data()},
                       dense.data());
    for (size_t i = 0; i < count; i++) memcpy(states + i * RNG_STATE_BYTES, (bad[i] ? mid.data() : end.data()) + i * RNG_STATE_BYTES, RNG_STATE_BYTES);
  } else {
    batch_prove(permutation, k, vec_m_blinders, rand, dense.data());
  }
  for (size_t i = 0; i < count; i++) {
    if (bad[i]) {   // Err(SerializationError): the placeholder's proof is dropped
      memset(post_trackers_out + i * ell * 96, 0, ell * 96);
      memset(proofs_out + i * rec, 0, rec);
      status[i] = CPX_ERR_DESERIALIZE;
    } else {
      memcpy(proofs_out + i * rec + 48, dense.data() + i * psz, psz);
      status[i] = CPX_OK;
    }
  }
}

// ---------------------------------------------------------------- draws from ChaCha12 states (rng.hip, rng.hpp)
// The reference hands every prover `rng: &mut T`; here a stream's state goes up (40 bytes), k_rng_draw makes the draws where their consumer
// reads them, and the advanced state comes back.  A caller's states are written only when the call has succeeded.
namespace {
constexpr size_t kRngFrEachMax = (size_t)1 << 20, kRngFrTotalMax = (size_t)1 << 26;
void check_rng_states(size_t count, const uint8_t* states) {
  for (size_t i = 0; i < count; i++) {
    uint64_t pos;
    memcpy(&pos, states + i * RNG_STATE_BYTES + 32, 8);
    if (!rng_pos_valid(pos)) throw ArgError("rng state: word_pos within 2^32 words of 2^64");
  }
}
}  // namespace
void Engine::trim_rng() {
  const auto trim = [](auto& b) {
    if (b.bytes() > kTier0Keep) b.release();
  };
  each_buf(trim, rng_.states, rng_.mid, rng_.perm, rng_.kb);
}

// Fr::rand n_each times per stream
void Engine::rng_fr(size_t count, uint8_t* states, size_t n_each, uint8_t* out) {
  if (count > kTrackerBatchMax || n_each > kRngFrEachMax) throw ArgError("rng draws: at most 2^23 streams and 2^20 draws each per call");
  if (!count || !n_each) return;
  if (count * n_each > kRngFrTotalMax) throw ArgError("rng draws: at most 2^26 draws per call");
  check_rng_states(count, states);
  std::vector<uint8_t> st;
  CallScope call(this);
  DevBuf<uint8_t>& dst = t0_.bytes;
  DevBuf<Fr>& dfr = t0_.fr;
  dst.ensure(count * RNG_STATE_BYTES);
  dfr.ensure(count * n_each);
  st.resize(count * RNG_STATE_BYTES);
  CPX_HIP(hipMemcpyAsync(dst.p, states, st.size(), hipMemcpyHostToDevice, stream_));
  tick("k_rng_draw", (double)(count * n_each * sizeof(Fr)), (double)(count * n_each));
  launch_rng_draw(rng_draw_args(dst.p, nullptr, count, 0, nullptr, {{n_each, dfr.p}}), stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(out, dfr.p, count * n_each * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(st.data(), dst.p, st.size(), hipMemcpyDeviceToHost, stream_));
  call.finish();
  memcpy(states, st.data(), st.size());
}

// G1Projective::rand(rng).into_affine() n_each times per stream (rng_g1.hip; the rounds in rng_g1_plan.hpp).  Rounds run per chunk of
// streams until no stream of the chunk owes a point; between two rounds the host reads the chunk's shortfall counts and nothing else.
// The scratch is one carved block of the tier-0 set: the call's scope gives back what grew beyond kTier0Keep.
void Engine::rng_g1(size_t count, uint8_t* states, size_t n_each, uint8_t* out_affine, uint8_t* out_compressed) {
  if (!RngG1Plan::fits(count, n_each)) throw ArgError("rng G1 draws: at most 2^20 streams, 2^16 points each and 2^22 points per call");
  if (!count || !n_each) return;
  check_rng_states(count, states);
  const RngG1Plan pl(count, n_each, opt_.rng_g1_round_cap);
  const size_t total = count * n_each;
  std::vector<RngG1Stream> hs(count);
  std::vector<uint32_t> owed(pl.chunk);
  for (size_t i = 0; i < count; i++) {
    uint64_t pos;
    memcpy(&pos, states + i * RNG_STATE_BYTES + 32, 8);
    hs[i] = RngG1Stream{pos, pos, 0, (uint32_t)n_each, 0, 0};
  }
  CallScope call(this);
  DevBuf<Aff>& dout = t0_.a0;
  DevBuf<uint8_t>&dcomp = sh_.bytes, &blob = t0_.bytes;
  const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_states = 0, o_streams = o_states + up(pl.chunk * RNG_STATE_BYTES), o_owed = o_streams + up(pl.chunk * sizeof(RngG1Stream)),
               o_sel = o_owed + up(pl.chunk * sizeof(uint32_t)), o_cand = o_sel + up(pl.chunk * n_each * sizeof(uint32_t)),
               o_pts = o_cand + up(pl.chunk * pl.cap * sizeof(RngG1Cand)), o_end = o_pts + up(pl.chunk * pl.cap * sizeof(Aff28));
  dout.ensure(total);
  if (out_compressed) dcomp.ensure(total * 48);
  blob.ensure(o_end);
  RngG1Args a{};
  a.states = blob.p + o_states;
  a.streams = reinterpret_cast<RngG1Stream*>(blob.p + o_streams);
  a.shortfall = reinterpret_cast<uint32_t*>(blob.p + o_owed);
  a.sel = reinterpret_cast<uint32_t*>(blob.p + o_sel);
  a.cand = reinterpret_cast<RngG1Cand*>(blob.p + o_cand);
  a.pts = reinterpret_cast<Aff28*>(blob.p + o_pts);
  a.cap = (uint32_t)pl.cap;
  a.n_each = (uint32_t)n_each;
  a.round_cap = (uint32_t)opt_.rng_g1_round_cap;
  const size_t round_limit = 4096 + 64 * n_each;   // (a candidate has a root with probability 1/2: a stream that gets nowhere in this many rounds is a bug, not bad luck)
  rng_g1_rounds_ = 0;
  for (size_t c = 0; c < pl.chunks(); c++) {
    const size_t first = c * pl.chunk, n = pl.chunk_streams(c);
    a.nstreams = (uint32_t)n;
    CPX_HIP(hipMemcpyAsync(blob.p + o_states, states + first * RNG_STATE_BYTES, n * RNG_STATE_BYTES, hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(a.streams, hs.data() + first, n * sizeof(RngG1Stream), hipMemcpyHostToDevice, stream_));
    for (size_t round = 1;; round++) {
      if (round > round_limit) throw std::runtime_error("rng G1 draws: a stream made no progress");
      tick("k_rng_g1_scan", 0, (double)n);
      launch_rng_g1_scan(a, stream_);
      tock();
      tick("k_rng_g1_sqrt", 0, (double)(n * pl.cap));
      launch_rng_g1_sqrt(a, stream_);
      tock();
      tick("k_rng_g1_select", 0, (double)n);
      launch_rng_g1_select(a, stream_);
      tock();
      tick("k_clear_cofactor", 192.0 * (n * n_each), (double)(n * n_each));
      launch_clear_cofactor(a.sel, a.pts, nullptr, n * n_each, dout.p + first * n_each, stream_);
      tock();
      CPX_HIP(hipMemcpyAsync(owed.data(), a.shortfall, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
      CPX_HIP(hipStreamSynchronize(stream_));
      rng_g1_rounds_ = std::max(rng_g1_rounds_, round);
      bool more = false;
      for (size_t i = 0; i < n; i++) more = more || owed[i] != 0;
      if (!more) break;
    }
    CPX_HIP(hipMemcpyAsync(hs.data() + first, a.streams, n * sizeof(RngG1Stream), hipMemcpyDeviceToHost, stream_));   // the positions (the next chunk reuses the block)
  }
  if (out_compressed) {
    tick("k_compress", 144.0 * total, (double)total);
    launch_compress(dout.p, (int)total, (int)total, 1, dcomp.p, stream_);
    tock();
    CPX_HIP(hipMemcpyAsync(out_compressed, dcomp.p, total * 48, hipMemcpyDeviceToHost, stream_));
  }
  if (out_affine) CPX_HIP(hipMemcpyAsync(out_affine, dout.p, total * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  call.finish();
  for (size_t i = 0; i < count; i++) memcpy(states + i * RNG_STATE_BYTES + 32, &hs[i].pos, 8);
}

// [h] P for n points of E(Fp), whatever option scale_any_point says
void Engine::clear_cofactor(const uint8_t* points, size_t n, uint8_t* out_affine) {
  if (n > ((size_t)1 << 24)) throw ArgError("cpx_g1_clear_cofactor: at most 2^24 points per call");
  if (!n) return;
  CallScope call(this);
  DevBuf<Aff>&din = t0_.a0, &dout = t0_.a1;
  din.ensure(n);
  dout.ensure(n);
  CPX_HIP(hipMemcpyAsync(din.p, points, n * sizeof(Aff), hipMemcpyHostToDevice, stream_));
  tick("k_clear_cofactor", 192.0 * n, (double)n);
  launch_clear_cofactor(nullptr, nullptr, din.p, n, dout.p, stream_);
  tock();
  CPX_HIP(hipMemcpyAsync(out_affine, dout.p, n * sizeof(Aff), hipMemcpyDeviceToHost, stream_));
  call.finish();
}

// crs.rs:61-69 generate_crs on the caller's stream: ell + 7 draws, then from_points.  Refusals of set_crs come before the first word
void Engine::crs_generate(size_t ell, uint8_t* state, uint8_t* points_out) {
  const size_t n = ell + 4;   // (Engine::set_crs: ell + N_BLINDERS)
  if (ell == 0 || (n & (n - 1))) throw std::invalid_argument("ell + 4 must be a power of two");
  if (ell + 7 > kRngG1EachMax) throw ArgError("cpx_crs_generate: ell + 7 exceeds the points one stream draws per call");
  std::vector<uint8_t> st(state, state + RNG_STATE_BYTES), pts((ell + 7) * sizeof(Aff));
  rng_g1(1, st.data(), ell + 7, pts.data(), nullptr);
  set_crs(ell, pts.data());
  memcpy(state, st.data(), st.size());
  if (points_out) memcpy(points_out, pts.data(), pts.size());
}

// README.md:85-95 per stream at the context's ell: the shuffle of 0..ell, k, vec_R, vec_S — one k_rng_draw program, then 2 ell G1 draws
void Engine::rng_instance_draws(size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* vec_R_out, uint8_t* vec_S_out) {
  if (!count) return;
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_;
  if (!RngG1Plan::fits(count, 2 * ell) || !ShufflePlan(count, ell, false).fits()) throw ArgError("rng instance draws: too many streams for one call");
  if (ell > rng_draw_max_shuffle()) throw ArgError("rng shuffle draws: ell exceeds the permutation a wave holds");
  check_rng_states(count, states);
  std::vector<uint8_t> st(states, states + count * RNG_STATE_BYTES), k(count * sizeof(Fr)), pts(count * 2 * ell * sizeof(Aff));
  std::vector<uint32_t> perm(count * ell);
  {
    CallScope call(this);
    DevBuf<uint8_t>& dst = t0_.bytes;
    DevBuf<Fr>& dfr = t0_.fr;
    dst.ensure(count * RNG_STATE_BYTES);
    dfr.ensure(count);
    sh_.perm.ensure(count * ell);
    CPX_HIP(hipMemcpyAsync(dst.p, st.data(), st.size(), hipMemcpyHostToDevice, stream_));
    tick("k_rng_draw", (double)(count * (ell * sizeof(uint32_t) + sizeof(Fr))), (double)count);
    launch_rng_draw(rng_draw_args(dst.p, nullptr, count, ell, sh_.perm.p, {{1, dfr.p}}), stream_);
    tock();
    CPX_HIP(hipMemcpyAsync(perm.data(), sh_.perm.p, perm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(k.data(), dfr.p, k.size(), hipMemcpyDeviceToHost, stream_));
    CPX_HIP(hipMemcpyAsync(st.data(), dst.p, st.size(), hipMemcpyDeviceToHost, stream_));
    call.finish();
  }
  rng_g1(count, st.data(), 2 * ell, pts.data(), nullptr);
  const size_t row = ell * sizeof(Aff);
  if (permutation_out) memcpy(permutation_out, perm.data(), perm.size() * sizeof(uint32_t));
  if (k_out) memcpy(k_out, k.data(), k.size());
  for (size_t i = 0; i < count; i++) {
    if (vec_R_out) memcpy(vec_R_out + i * row, pts.data() + 2 * i * row, row);
    if (vec_S_out) memcpy(vec_S_out + i * row, pts.data() + (2 * i + 1) * row, row);
  }
  memcpy(states, st.data(), st.size());
}

// whisk.rs:144-179: the draws of one generate_whisk_shuffle_proof per stream — shuffle, k, 4 blinders, 3n + 9 — downloaded
void Engine::rng_shuffle_draws(size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* blinders_out, uint8_t* rand_out, uint8_t* states_after_k) {
  if (!count) return;
  if (!ell_) throw std::logic_error("set_crs first");
  const size_t ell = ell_, nrand = 3 * n_ + 9;
  if (count > kTrackerBatchMax || !ShufflePlan(count, ell, false).fits() || count * nrand > kRngFrTotalMax) throw ArgError("rng shuffle draws: too many streams for one call");
  if (ell > rng_draw_max_shuffle()) throw ArgError("rng shuffle draws: ell exceeds the permutation a wave holds");
  check_rng_states(count, states);
  std::vector<uint8_t> st, mid;
  CallScope call(this);
  DevBuf<uint8_t>& dst = t0_.bytes;   // states | states after k
  DevBuf<Fr>& dfr = t0_.fr;           // k | blinders | rand
  dst.ensure(2 * count * RNG_STATE_BYTES);
  dfr.ensure(count * (5 + nrand));
  sh_.perm.ensure(count * ell);
  st.resize(count * RNG_STATE_BYTES);
  mid.resize(count * RNG_STATE_BYTES);
  CPX_HIP(hipMemcpyAsync(dst.p, states, st.size(), hipMemcpyHostToDevice, stream_));
  tick("k_rng_draw", (double)(count * (ell * sizeof(uint32_t) + (5 + nrand) * sizeof(Fr))), (double)(count * (5 + nrand)));
  launch_rng_draw(rng_draw_args(dst.p, dst.p + st.size(), count, ell, sh_.perm.p, {{1, dfr.p}, {4, dfr.p + count}, {nrand, dfr.p + 5 * count}}), stream_);
  tock();
  if (permutation_out) CPX_HIP(hipMemcpyAsync(permutation_out, sh_.perm.p, count * ell * sizeof(uint32_t), hipMemcpyDeviceToHost, stream_));
  if (k_out) CPX_HIP(hipMemcpyAsync(k_out, dfr.p, count * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  if (blinders_out) CPX_HIP(hipMemcpyAsync(blinders_out, dfr.p + count, 4 * count * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  if (rand_out) CPX_HIP(hipMemcpyAsync(rand_out, dfr.p + 5 * count, count * nrand * sizeof(Fr), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(st.data(), dst.p, st.size(), hipMemcpyDeviceToHost, stream_));
  CPX_HIP(hipMemcpyAsync(mid.data(), dst.p + st.size(), mid.size(), hipMemcpyDeviceToHost, stream_));
  call.finish();
  memcpy(states, st.data(), st.size());
  if (states_after_k) memcpy(states_after_k, mid.data(), mid.size());
}

// whisk.rs:144-179 for every (pre_trackers, stream) item with the draws made on the device
void Engine::whisk_generate_shuffle_proofs_rng(size_t count, const uint8_t* pre_trackers, uint8_t* states, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status) {
  if (!count) return;
  if (!ell_) throw std::logic_error("set_crs first");
  if (ell_ > rng_draw_max_shuffle()) throw ArgError("rng shuffle draws: ell exceeds the permutation a wave holds");
  check_rng_states(count, states);
  if (device_prefix(count)) {   // nothing but the states crosses the bus
    struct Trim {
      Engine* e;
      ~Trim() { e->trim_rng(); }
    } trim{this};
    whisk_generate_shuffle_proofs_with(count, pre_trackers, nullptr, nullptr, nullptr, nullptr, states, post_trackers_out, proofs_out, status);
    return;
  }
  // a few proofs, driven from the host: the draws come down and go through the explicit-draw call
  const size_t nrand = 3 * n_ + 9;
  std::vector<uint8_t> end(states, states + count * RNG_STATE_BYTES), mid(count * RNG_STATE_BYTES), k(count * 32), mbl(count * 4 * 32), rnd(count * nrand * 32);
  std::vector<uint32_t> perm(count * ell_);
  rng_shuffle_draws(count, end.data(), perm.data(), k.data(), mbl.data(), rnd.data(), mid.data());
  whisk_generate_shuffle_proofs(count, pre_trackers, perm.data(), k.data(), mbl.data(), rnd.data(), post_trackers_out, proofs_out, status);
  for (size_t i = 0; i < count; i++)
    memcpy(states + i * RNG_STATE_BYTES, (status[i] == CPX_ERR_DESERIALIZE ? mid.data() : end.data()) + i * RNG_STATE_BYTES, RNG_STATE_BYTES);
}

// CurdleproofsProof::new on the loaded instances, the 3n + 9 draws of each taken from its stream
void Engine::batch_prove_rng(const uint32_t* permutation, const uint8_t* k, const uint8_t* m_blinders, uint8_t* states, uint8_t* proofs_out) {
  if (!B_) throw std::logic_error("batch_load first");
  check_rng_states(B_, states);
  if (device_prefix(B_)) {
    batch_prove_device(ProveDraws{permutation, k, m_blinders, hipMemcpyHostToDevice, nullptr, states, states}, proofs_out);
    return;
  }
  const size_t nrand = 3 * n_ + 9;
  std::vector<uint8_t> st(states, states + B_ * RNG_STATE_BYTES), rnd(B_ * nrand * 32);
  rng_fr(B_, st.data(), nrand, rnd.data());
  batch_prove_tables(permutation, k, m_blinders, rnd.data(), proofs_out);
  memcpy(states, st.data(), st.size());
}

// whisk.rs:106-130 is_valid_whisk_shuffle_proof for every (pre_trackers, post_trackers, proof) triple
void Engine::whisk_verify_shuffle_proofs(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand,
                                         int* verdict) {
  whisk_verify_shuffle_proofs_with(count, pre_trackers, post_trackers, proofs, verdict, [&](const uint8_t* dense, int* v) { batch_verify(dense, rand, v); });
}
// ... with 12 factors per item, through the grouped form of the accumulated check (locate_plan.hpp)
void Engine::whisk_verify_shuffle_proofs_grouped(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand,
                                                 int* verdict, size_t* n_rechecked) {
  if (n_rechecked) *n_rechecked = 0;
  whisk_verify_shuffle_proofs_with(count, pre_trackers, post_trackers, proofs, verdict,
                                   [&](const uint8_t* dense, int* v) { batch_verify_grouped(dense, rand, v, n_rechecked); });
}
// The explicit pre side: its bytes are uploaded and decoded with the rest
void Engine::whisk_verify_shuffle_proofs_with(size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs, int* verdict,
                                              const ShuffleVerifyFn& verify) {
  if (!shuffle_verify_begin(count, verdict)) return;
  const ShufflePlan pl(count, ell_, true);
  if (!pl.fits()) throw ArgError("shuffle proofs: count * ell exceeds the 32-bit index range of one call");
  const Aff G = generator();   // (before the scope, as above)
  ShuffleVerifyHost host;
  CallScope call(this);
  shuffle_verify_body(call, host, pl, G, pre_trackers, nullptr, post_trackers, proofs, verdict, verify);
}
// What both bodies begin with: the verdict preset and the refusal that needs nothing but the context; false: nothing to verify
bool Engine::shuffle_verify_begin(size_t count, int* verdict) {
  for (size_t i = 0; i < count; i++) verdict[i] = CPX_ERR_INTERNAL;   // an entry the device never wrote is never read as accepted
  if (count && !ell_) throw std::logic_error("set_crs first");
  return count != 0;
}
// The shared body, inside the caller's scope (`h`: the caller's, declared above it): decode the trackers and M, load the count instances,
// hand the dense proofs to `verify`, override the undecodable items.  The pre side is either pre_trackers (src == null), uploaded and
// decoded in front of post | M into the planes R | S, or the run's source list `src` (pre_trackers == null): then only post | M go up, at
// offsets that are tracker_bytes() lower, into the planes T | U and the M slots, and k_run_gather fills R | S from the candidate planes
// and from T | U.  Ends synchronised, the planes still in sh_.pts.
void Engine::shuffle_verify_body(CallScope& call, ShuffleVerifyHost& h, const ShufflePlan& pl, const Aff& G, const uint8_t* pre_trackers, const uint32_t* src,
                                 const uint8_t* post_trackers, const uint8_t* proofs, int* verdict, const ShuffleVerifyFn& verify) {
  const size_t count = pl.count, psz = proof_size(), rec = 48 + psz, pp = pl.plane_points(), tb = pl.tracker_bytes();
  const size_t first = src ? 2 * pp : 0, skip = src ? tb : 0, npts = pl.points() - first;   // the encodings decoded here, the bytes in front of them that are not uploaded
  // strict_infinity = 0: non-canonical infinity encodings are rewritten in COPIES of the inputs (canonical_infinities)
  if (!src) pre_trackers = canonical_infinities(pre_trackers, tb, pp, 96, {0, 48}, h.canon[0]);
  post_trackers = canonical_infinities(post_trackers, tb, pp, 96, {0, 48}, h.canon[1]);
  proofs = canonical_infinities(proofs, count * rec, count, rec, {0}, h.canon[2]);   // M; the proof points behind it are batch_verify's
  h.dense.resize(count * psz);                                                      // CurdleproofsProof::deserialize reads the bytes behind M (whisk.rs:122)
  for (size_t i = 0; i < count; i++) memcpy(h.dense.data() + i * psz, proofs + i * rec + 48, psz);
  h.off.resize(npts);
  for (size_t j = 0; j < npts; j++) h.off[j] = (uint32_t)(pl.src_offset(first + j) - skip);
  sh_.bytes.ensure(pl.upload_bytes() - skip);
  sh_.status.ensure(pl.points());
  sh_.off.ensure(npts);
  if (src) sh_.perm.ensure(3 * pp);   // the source list | the commit list's destinations | its positions
  sh_.pts.ensure(pl.points());
  sh_.bad.ensure(count);
  sh_.mjac.ensure(count);
  uint8_t* d_post = sh_.bytes.p + (tb - skip);
  if (!src) CPX_HIP(hipMemcpyAsync(sh_.bytes.p, pre_trackers, tb, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpyAsync(d_post, post_trackers, tb, hipMemcpyHostToDevice, stream_));
  CPX_HIP(hipMemcpy2DAsync(d_post + tb, 48, proofs, rec, 48, count, hipMemcpyHostToDevice, stream_));   // the M prefixes only
  CPX_HIP(hipMemcpyAsync(sh_.off.p, h.off.data(), npts * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  if (src) CPX_HIP(hipMemcpyAsync(sh_.perm.p, src, pp * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
  tick("k_decompress", 0, (double)npts);
  launch_decompress(opt_, sh_.bytes.p, (int)npts, sh_.pts.p + first, nullptr, sh_.status.p + first, 1, stream_, sh_.off.p);
  tock();
  if (src) {
    tick("k_run_gather", (double)pp * (4 * sizeof(Aff) + 4 + sizeof(uint32_t)), (double)pp);   // two points and two status bytes read and written, one list entry
    launch_run_gather((uint32_t)pp, (uint32_t)cand_.n, sh_.perm.p, cand_.pts.p, cand_.status.p, sh_.pts.p, sh_.status.p, stream_);
    tock();
  }
  tick("k_shuffle_status", 0, (double)count);
  launch_shuffle_status(pl, sh_.status.p, sh_.pts.p, G, nullptr, nullptr, nullptr, sh_.mjac.p, sh_.bad.p, stream_);
  tock();
  const Aff* d = sh_.pts.p;
  load_rows(count, reinterpret_cast<const uint8_t*>(d), reinterpret_cast<const uint8_t*>(d + pp), reinterpret_cast<const uint8_t*>(d + 2 * pp),
            reinterpret_cast<const uint8_t*>(d + 3 * pp), reinterpret_cast<const uint8_t*>(sh_.mjac.p), true);
  h.bad.resize(count);
  CPX_HIP(hipMemcpyAsync(h.bad.data(), sh_.bad.p, count, hipMemcpyDeviceToHost, stream_));
  call.finish();
  verify(h.dense.data(), verdict);
  for (size_t i = 0; i < count; i++)
    if (h.bad[i]) verdict[i] = CPX_ERR_DESERIALIZE;   // an undecodable tracker or M: Err(SerializationError), whatever the placeholder's verdict
}

// ---------------------------------------------------------------- a run of shuffles against the resident candidate list (run.hip, run_plan.hpp)
// The list: decoded once, kept as two planes cand_R | cand_S with the decoder's status per point and the bytes as given.  An undecodable
// candidate is no error here: whisk.rs fails in unzip_trackers only, so it fails the items that read it.
void Engine::whisk_candidates_load(size_t n, const uint8_t* trackers, uint8_t* status) {
  if (n > RUN_MAX_CANDIDATES) throw ArgError("candidate list: more than 2^24 trackers");
  if (!n) {
    cand_.pts.release();
    cand_.status.release();
    cand_.bytes.clear();
    cand_.n = 0;
    return;
  }
  std::vector<uint8_t> st, canon;
  std::vector<uint8_t> mirror(trackers, trackers + n * 96);   // (as given)
  std::vector<uint32_t> off;
  DevBuf<Aff> pts;   // the new list replaces the old one only once it is complete
  DevBuf<uint8_t> dst;
  {
    CallScope call(this);
    pts.ensure(2 * n);
    dst.ensure(2 * n);
    sh_.bytes.ensure(n * 96);
    sh_.off.ensure(2 * n);
    decode_tracker_planes(n, trackers, canon, off, sh_.bytes.p, sh_.off.p, pts.p, dst.p);   // plane-major, as the run's own planes
    st.resize(2 * n);
    CPX_HIP(hipMemcpyAsync(st.data(), dst.p, 2 * n, hipMemcpyDeviceToHost, stream_));
    call.finish();
  }
  std::swap(cand_.pts.p, pts.p);
  std::swap(cand_.pts.cap, pts.cap);
  std::swap(cand_.status.p, dst.p);
  std::swap(cand_.status.cap, dst.cap);
  cand_.bytes.swap(mirror);
  cand_.n = n;
  cand_.strict = opt_.strict_infinity;
  if (status)
    for (size_t i = 0; i < n; i++) status[i] = st[i] ? st[i] : st[n + i];
}

void Engine::whisk_candidates_read(size_t first, size_t count, uint8_t* trackers_out) const {
  if (first > cand_.n || count > cand_.n - first) throw ArgError("candidate list: the range is outside the list");
  if (count) memcpy(trackers_out, cand_.bytes.data() + first * 96, count * 96);
}

// whisk.rs:106-130 is_valid_whisk_shuffle_proof for a run of items over the resident list
void Engine::whisk_verify_shuffle_run(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand, int* verdict,
                                      size_t* n_applied) {
  whisk_verify_shuffle_run_with(count, indices, post_trackers, proofs, verdict, n_applied, [&](const uint8_t* dense, int* v) { batch_verify(dense, rand, v); });
}
// ... with 12 factors per item, through the grouped form of the accumulated check (locate_plan.hpp)
void Engine::whisk_verify_shuffle_run_grouped(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand,
                                              int* verdict, size_t* n_applied, size_t* n_rechecked) {
  if (n_rechecked) *n_rechecked = 0;
  whisk_verify_shuffle_run_with(count, indices, post_trackers, proofs, verdict, n_applied,
                                [&](const uint8_t* dense, int* v) { batch_verify_grouped(dense, rand, v, n_rechecked); });
}
// The pre side comes from the resident list: the planes R | S are gathered from the candidate planes and from T | U through the source
// list, and the accepted prefix is written back through the commit list as the last step.
void Engine::whisk_verify_shuffle_run_with(size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, int* verdict, size_t* n_applied,
                                           const ShuffleVerifyFn& verify) {
  if (n_applied) *n_applied = 0;
  if (!shuffle_verify_begin(count, verdict)) return;
  if (!cand_.n) throw std::logic_error("cpx_whisk_candidates_load first");
  if (cand_.strict != opt_.strict_infinity) throw std::logic_error("option strict_infinity changed since the candidate list was loaded");
  const size_t ell = ell_, n = cand_.n;
  const ShufflePlan pl(count, ell, true);
  if (!pl.fits()) throw ArgError("shuffle run: count * ell exceeds the 32-bit index range of one call");
  const RunPlan rp(count, ell, n);
  if (!rp.indices_valid(indices)) throw ArgError("shuffle run: an index is outside the candidate list");
  const Aff G = generator();   // (before the scope, as above)
  const size_t pp = pl.plane_points();
  std::vector<uint32_t> lists(3 * pp), last(n);
  rp.resolve(indices, lists.data(), last.data());
  ShuffleVerifyHost host;
  CallScope call(this);
  shuffle_verify_body(call, host, pl, G, nullptr, lists.data(), post_trackers, proofs, verdict, verify);
  if (!n_applied) return;   // a dry run
  size_t lead = 0;
  while (lead < count && verdict[lead] == CPX_OK) lead++;
  // The write-back, last: the planes T | U of the scratch still hold the decoded post trackers of every accepted item (k_shuffle_status
  // rewrites the rows of undecodable items only, and none of those is in the prefix)
  uint32_t *dst = lists.data() + pp, *pos = lists.data() + 2 * pp;
  const size_t len = rp.commit_list(indices, (uint32_t)lead, dst, pos, last.data());
  if (len) {
    CPX_HIP(hipMemcpyAsync(sh_.perm.p + pp, dst, len * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    CPX_HIP(hipMemcpyAsync(sh_.perm.p + 2 * pp, pos, len * sizeof(uint32_t), hipMemcpyHostToDevice, stream_));
    tick("k_run_commit", (double)len * (4 * sizeof(Aff) + 4 + 2 * sizeof(uint32_t)), (double)len);
    launch_run_commit((uint32_t)len, (uint32_t)pp, (uint32_t)n, sh_.perm.p + pp, sh_.perm.p + 2 * pp, sh_.pts.p, sh_.status.p, cand_.pts.p, cand_.status.p, stream_);
    tock();
    call.finish();
    for (size_t t = 0; t < len; t++) memcpy(cand_.bytes.data() + (size_t)dst[t] * 96, post_trackers + (size_t)pos[t] * 96, 96);   // the list keeps the bytes as the items spelt them
  }
  *n_applied = lead;
}

}  // namespace cpx
