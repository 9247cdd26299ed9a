// extern "C" boundary (include/cpx.h) over the engine.  Nothing unwinds across it.
#include "../../include/cpx.h"
#include <cstring>
#include <map>
#include <new>
#include <string>
#include <vector>
#include <cstdlib>
#include "engine.hpp"
#include "find_plan.hpp"
#include "transcript_state.hpp"

using namespace cpx;

struct cpx_ctx {
  Engine* eng = nullptr;
  std::string err;
};

// msm_accumulator.rs:22-68.  The per-base scalar merge (Fr additions keyed by the base's bytes) is host
// bookkeeping; the group work (a*C and the final MSM) runs on the device.
struct cpx_accum {
  cpx_ctx* ctx;
  struct Key {
    uint8_t b[96];
    bool operator<(const Key& o) const { return memcmp(b, o.b, 96) < 0; }
  };
  std::map<Key, host::S> base_scalar;
  std::vector<uint8_t> lhs_points;   // Jacobian C_i (144 B each)
  std::vector<host::S> lhs_scalars;  // a_i
};

namespace {
// The host side of this library is compiled for x86-64-v3 + ADX (build.py: the Keccak permutation of the host transcripts and the 64-bit-limb Fr
// products use BMI2 / ADX forms).  A host without them would die of SIGILL somewhere inside a prove; cpx_ctx_create refuses it instead.
const char* missing_cpu_feature() {
#if defined(__x86_64__) && !defined(__HIP_DEVICE_COMPILE__)   // (this file is compiled as HIP: the device pass has no CPU to ask)
  __builtin_cpu_init();
  if (!__builtin_cpu_supports("avx2")) return "AVX2";
  if (!__builtin_cpu_supports("bmi2")) return "BMI2";
  if (!__builtin_cpu_supports("fma")) return "FMA";
  unsigned a = 0, b = 0, c = 0, d = 0;
  __asm__ volatile("cpuid" : "=a"(a), "=b"(b), "=c"(c), "=d"(d) : "a"(7u), "c"(0u));
  if (!(b & (1u << 19))) return "ADX";   // CPUID.(EAX=7, ECX=0):EBX bit 19
#endif
  return nullptr;
}
thread_local std::string g_create_error;   // why the calling thread's last cpx_ctx_create failed (there is no context to ask)
}  // namespace

namespace {
template <class F> int guarded(cpx_ctx* ctx, F&& f) {
  if (!ctx || !ctx->eng) return CPX_ERR_ARG;
  try {
    return f();
  } catch (const HipError& e) {
    ctx->err = e.what();
    return CPX_ERR_HIP;
  } catch (const ArgError& e) {
    ctx->err = e.what();
    return CPX_ERR_ARG;
  } catch (const std::invalid_argument& e) {
    ctx->err = e.what();
    return CPX_ERR_NOT_POW2;
  } catch (const std::logic_error& e) {
    ctx->err = e.what();
    return CPX_ERR_STATE;
  } catch (const std::bad_alloc&) {
    ctx->err = "out of host memory";
    return CPX_ERR_INTERNAL;
  } catch (const std::exception& e) {
    ctx->err = e.what();
    return CPX_ERR_INTERNAL;
  } catch (...) {
    ctx->err = "unknown failure";
    return CPX_ERR_INTERNAL;
  }
}
}  // namespace

// the transcript as a 216-byte value (transcript_state.hpp; cpx_transcript_* below)
namespace {
// one operation on a copy of the state, written back when it succeeds: an error leaves the caller's state as it was
template <class F> int on_transcript(uint8_t* state, const uint8_t* label, size_t label_len, size_t len, F&& f) {
  Strobe s;
  if (!state || (label_len && !label) || len > 0xffffffffu) return CPX_ERR_ARG;   // (merlin encodes a length as LE32)
  if (!transcript_state_load(state, s)) return CPX_ERR_ARG;
  f(s, reinterpret_cast<const char*>(label ? label : state));   // (an empty label is never read)
  transcript_state_store(s, state);
  return CPX_OK;
}
}  // namespace

extern "C" {

int cpx_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void* cpx_host_alloc(size_t bytes) {
  void* p = nullptr;
  if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
  CPX_HOST_MEMORY_ACQUIRE();
  return p;
}
void cpx_host_free(void* p) {
  CPX_HOST_MEMORY_RELEASE();
  if (p) (void)hipHostFree(p);
}

int cpx_ctx_create(int device_id, cpx_ctx** out) {
  if (!out) return CPX_ERR_ARG;
  *out = nullptr;
  g_create_error.clear();
  if (const char* f = missing_cpu_feature()) {
    g_create_error = std::string("cpx_ctx_create: this host CPU lacks ") + f + " (libcpx.so's host code is built for x86-64-v3 + ADX)";
    return CPX_ERR_STATE;
  }
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || device_id < 0 || device_id >= n) {
    g_create_error = "cpx_ctx_create: no HIP device with this index";
    return CPX_ERR_HIP;
  }
  cpx_ctx* c = new (std::nothrow) cpx_ctx();
  if (!c) return CPX_ERR_INTERNAL;
  try {
    c->eng = new Engine(device_id);
  } catch (const std::exception& e) {
    g_create_error = std::string("cpx_ctx_create: ") + e.what();
    delete c;
    return CPX_ERR_HIP;
  } catch (...) {
    delete c;
    return CPX_ERR_HIP;
  }
  *out = c;
  return CPX_OK;
}
void cpx_ctx_destroy(cpx_ctx* ctx) {
  if (!ctx) return;
  delete ctx->eng;
  delete ctx;
}
int cpx_ctx_set_option(cpx_ctx* ctx, const char* key, long long value) {
  if (!ctx || !ctx->eng || !key) return CPX_ERR_ARG;
  if (!ctx->eng->set_option(key, (long)value)) {
    ctx->err = std::string("cpx_ctx_set_option: unknown key or value out of range: ") + key;
    return CPX_ERR_ARG;
  }
  return CPX_OK;
}
int cpx_ctx_get_option(const cpx_ctx* ctx, const char* key, long long* value) {
  if (!ctx || !ctx->eng || !key || !value) return CPX_ERR_ARG;
  long v = 0;
  if (!ctx->eng->get_option(key, &v)) return CPX_ERR_ARG;
  *value = v;
  return CPX_OK;
}
const char* cpx_last_error(const cpx_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }   // NULL: why this thread's last cpx_ctx_create failed

int cpx_ctx_set_crs(cpx_ctx* ctx, size_t ell, const uint8_t* points, size_t n_points) {
  if (!points) return CPX_ERR_ARG;
  if (n_points < ell + 7) {   // crs.rs:40-42 "not enough points"
    if (ctx) ctx->err = "CurdleproofsCrs::from_points: not enough points (need ell + 7)";
    return CPX_ERR_ARG;
  }
  return guarded(ctx, [&] {
    ctx->eng->set_crs(ell, points);
    return CPX_OK;
  });
}
int cpx_crs_sums(const cpx_ctx* ctx, uint8_t g_sum[96], uint8_t h_sum[96]) {
  if (!ctx || !ctx->eng || !ctx->eng->ell()) return CPX_ERR_STATE;
  ctx->eng->crs_sums(g_sum, h_sum);
  return CPX_OK;
}
size_t cpx_batch_size(const cpx_ctx* ctx) { return (ctx && ctx->eng) ? ctx->eng->batch() : 0; }
size_t cpx_proof_size(const cpx_ctx* ctx) { return (ctx && ctx->eng && ctx->eng->ell()) ? ctx->eng->proof_size() : 0; }

int cpx_g1_msm(cpx_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[144]) {
  if (!out || (n && (!bases || !scalars))) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->msm(bases, scalars, n, out);
    return CPX_OK;
  });
}
int cpx_g1_msm_jac(cpx_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[144]) {
  if (!out || (n && (!bases || !scalars))) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->msm_jac(bases, scalars, n, out);
    return CPX_OK;
  });
}
int cpx_g1_fold(cpx_ctx* ctx, uint8_t* PL, const uint8_t* PR, const uint8_t gamma[32], size_t half) {
  if (half && (!PL || !PR || !gamma)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->fold(PL, PR, gamma, half);
    return CPX_OK;
  });
}
int cpx_g1_scale(cpx_ctx* ctx, const uint8_t* P, const uint8_t* scalars, size_t scalar_stride, size_t n, uint8_t* out) {
  if (n && (!P || !scalars || !out)) return CPX_ERR_ARG;
  if (scalar_stride != 0 && scalar_stride != 32) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->scale(P, scalars, scalar_stride, n, out);
    return CPX_OK;
  });
}
int cpx_g1_msm_many(cpx_ctx* ctx, size_t count, const uint32_t* lens, const uint8_t* bases, const uint8_t* scalars, uint8_t* out_jac, uint8_t* out_compressed) {
  if (count && (!lens || !bases || !scalars)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->msm_many(count, lens, bases, scalars, out_jac, out_compressed);
    return (int)CPX_OK;
  });
}
int cpx_g1_fold_many(cpx_ctx* ctx, size_t families, size_t half, uint8_t* PL, const uint8_t* PR, const uint8_t* gammas) {
  if (families && half && (!PL || !PR || !gammas)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->fold_many(families, half, PL, PR, gammas);
    return (int)CPX_OK;
  });
}
int cpx_g1_normalize(cpx_ctx* ctx, const uint8_t* jac, size_t n, uint8_t* out_affine, uint8_t* out_compressed) {
  if (n && !jac) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->normalize(jac, n, out_affine, out_compressed);
    return CPX_OK;
  });
}
int cpx_g1_decompress(cpx_ctx* ctx, const uint8_t* compressed, size_t n, uint8_t* out_affine, int check_subgroup) {
  if (n && (!compressed || !out_affine)) return CPX_ERR_ARG;
  return guarded(ctx, [&] { return ctx->eng->decompress(compressed, n, out_affine, check_subgroup); });
}

int cpx_g1_decompress_status(cpx_ctx* ctx, const uint8_t* compressed, size_t n, uint8_t* out_affine, int check_subgroup, uint8_t* status) {
  if (n && (!compressed || !out_affine || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] { return ctx->eng->decompress(compressed, n, out_affine, check_subgroup, status); });
}

int cpx_accum_new(cpx_ctx* ctx, cpx_accum** out) {
  if (!ctx || !ctx->eng || !out) return CPX_ERR_ARG;
  cpx_accum* a = new (std::nothrow) cpx_accum();
  if (!a) return CPX_ERR_INTERNAL;
  a->ctx = ctx;
  *out = a;
  return CPX_OK;
}
void cpx_accum_free(cpx_accum* acc) { delete acc; }
int cpx_accum_check(cpx_accum* acc, const uint8_t C[144], const uint8_t* vec_x, const uint8_t* vec_V, size_t n, const uint8_t random_factor[32]) {
  if (!acc || !C || !random_factor || (n && (!vec_x || !vec_V))) return CPX_ERR_ARG;
  return guarded(acc->ctx, [&] {
    host::S a;
    memcpy(a.f.v, random_factor, 32);
    if (!host::is_valid_factor(random_factor)) throw ArgError("random_factor must be a non-zero reduced field element (msm_accumulator.rs:44 draws Fr::rand)");
    acc->lhs_points.insert(acc->lhs_points.end(), C, C + 144);
    acc->lhs_scalars.push_back(a);
    for (size_t i = 0; i < n; i++) {
      cpx_accum::Key k;
      memcpy(k.b, vec_V + 96 * i, 96);
      host::S x;
      memcpy(x.f.v, vec_x + 32 * i, 32);
      auto it = acc->base_scalar.emplace(k, host::S::zero()).first;
      it->second += a * x;
    }
    return CPX_OK;
  });
}
int cpx_accum_verify(cpx_accum* acc) {
  if (!acc) return CPX_ERR_ARG;
  return guarded(acc->ctx, [&] {
    Engine* e = acc->ctx->eng;
    // msm(bases, scalars) - A_c == O, with A_c = sum a_i C_i folded into the same MSM (negated scalars)
    const size_t nl = acc->lhs_scalars.size(), nb = acc->base_scalar.size();
    std::vector<uint8_t> bases((nl + nb) * 96), scalars((nl + nb) * 32);
    if (nl) e->normalize(acc->lhs_points.data(), nl, bases.data(), nullptr);
    for (size_t i = 0; i < nl; i++) {
      host::S m = -acc->lhs_scalars[i];
      memcpy(&scalars[32 * i], m.f.v, 32);
    }
    size_t j = nl;
    for (auto& kv : acc->base_scalar) {
      memcpy(&bases[96 * j], kv.first.b, 96);
      memcpy(&scalars[32 * j], kv.second.f.v, 32);
      j++;
    }
    uint8_t res[144], comp[48];
    e->msm(bases.data(), scalars.data(), nl + nb, res);
    e->normalize(res, 1, nullptr, comp);
    return comp[0] == 0xc0 ? CPX_OK : CPX_ERR_VERIFY;
  });
}

int cpx_batch_load(cpx_ctx* ctx, size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M) {
  if (!batch || !vec_R || !vec_S || !vec_T || !vec_U || !M) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->batch_load(batch, vec_R, vec_S, vec_T, vec_U, M);
    return CPX_OK;
  });
}
int cpx_batch_load_begin(cpx_ctx* ctx, size_t batch, const uint8_t* vec_R, const uint8_t* vec_S, const uint8_t* vec_T, const uint8_t* vec_U, const uint8_t* M) {
  if (!batch || !vec_R || !vec_S || !vec_T || !vec_U || !M) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->batch_load_begin(batch, vec_R, vec_S, vec_T, vec_U, M);
    return CPX_OK;
  });
}
int cpx_batch_load_end(cpx_ctx* ctx) {
  return guarded(ctx, [&] {
    ctx->eng->batch_load_end();
    return CPX_OK;
  });
}
int cpx_batch_prove(cpx_ctx* ctx, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders, const uint8_t* rand, uint8_t* proofs_out) {
  if (!permutation || !k || !vec_m_blinders || !rand || !proofs_out) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    const size_t B = ctx->eng->batch(), ell = ctx->eng->ell();
    for (size_t i = 0; i < B * ell; i++)
      if (permutation[i] >= ell) return (int)CPX_ERR_ARG;
    ctx->eng->batch_prove(permutation, k, vec_m_blinders, rand, proofs_out);
    return (int)CPX_OK;
  });
}
int cpx_batch_verify(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand, int* verdict) {
  if (!proofs || !rand || !verdict) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->batch_verify(proofs, rand, verdict);
    return CPX_OK;
  });
}

int cpx_batch_verify_fused(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand, uint8_t* partial_jac, int* n_invalid) {
  if (!proofs || !rand || !partial_jac || !n_invalid) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->batch_verify_fused(proofs, rand, partial_jac, n_invalid);
    return CPX_OK;
  });
}
int cpx_batch_verify_grouped(cpx_ctx* ctx, const uint8_t* proofs, const uint8_t* rand, int* verdict, size_t* n_rechecked) {
  if (!proofs || !rand || !verdict) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->batch_verify_grouped(proofs, rand, verdict, n_rechecked);
    return CPX_OK;
  });
}
int cpx_g1_sum_jac(cpx_ctx* ctx, const uint8_t* points_jac, size_t n, uint8_t* out_jac, int* is_identity) {
  if ((n && !points_jac) || !out_jac || !is_identity) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    *is_identity = ctx->eng->sum_jac(points_jac, n, out_jac) ? 1 : 0;
    return CPX_OK;
  });
}

// ---- Whisk byte-level API (whisk.rs) ----
int cpx_whisk_generate_shuffle_proof(cpx_ctx* ctx, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t k[32], const uint8_t* vec_m_blinders,
                                     const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proof_out) {
  if (!pre_trackers || !permutation || !k || !vec_m_blinders || !rand || !post_trackers_out || !proof_out) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    const size_t ell = ctx->eng->ell();
    std::vector<uint8_t> seen(ell, 0);
    for (size_t i = 0; i < ell; i++) {   // must be a permutation of 0..ell (the reference shuffles (0..ELL))
      if (permutation[i] >= ell || seen[permutation[i]]) return (int)CPX_ERR_ARG;
      seen[permutation[i]] = 1;
    }
    return ctx->eng->whisk_generate_shuffle_proof(pre_trackers, permutation, k, vec_m_blinders, rand, post_trackers_out, proof_out);
  });
}
int cpx_whisk_is_valid_shuffle_proof(cpx_ctx* ctx, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proof, const uint8_t* rand, int* valid) {
  if (!pre_trackers || !post_trackers || !proof || !rand || !valid) return CPX_ERR_ARG;
  return guarded(ctx, [&] { return ctx->eng->whisk_is_valid_shuffle_proof(pre_trackers, post_trackers, proof, rand, valid); });
}
int cpx_whisk_generate_tracker_proof(cpx_ctx* ctx, const uint8_t tracker[96], const uint8_t k[32], const uint8_t blinder[32], uint8_t proof_out[128]) {
  if (!tracker || !k || !blinder || !proof_out) return CPX_ERR_ARG;
  return guarded(ctx, [&] { return ctx->eng->whisk_generate_tracker_proof(tracker, k, blinder, proof_out); });
}
int cpx_whisk_is_valid_tracker_proof(cpx_ctx* ctx, const uint8_t tracker[96], const uint8_t k_commitment[48], const uint8_t proof[128], int* valid) {
  if (!tracker || !k_commitment || !proof || !valid) return CPX_ERR_ARG;
  return guarded(ctx, [&] { return ctx->eng->whisk_is_valid_tracker_proof(tracker, k_commitment, proof, valid); });
}
int cpx_whisk_generate_tracker_proofs(cpx_ctx* ctx, size_t count, const uint8_t* trackers, const uint8_t* k, const uint8_t* blinders, uint8_t* proofs_out, int* status) {
  if (count && (!trackers || !k || !blinders || !proofs_out || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_generate_tracker_proofs(count, trackers, k, blinders, proofs_out, status);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_tracker_proofs(cpx_ctx* ctx, size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, int* verdict) {
  if (count && (!trackers || !k_commitments || !proofs || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_tracker_proofs(count, trackers, k_commitments, proofs, verdict);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_tracker_proofs_fused(cpx_ctx* ctx, size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand,
                                          uint8_t* partial_jac, int* n_invalid) {
  if (!tracker_check_fits(count)) return CPX_ERR_ARG;   // before anything is read
  if (!partial_jac || !n_invalid || (count && (!trackers || !k_commitments || !proofs || !rand))) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_tracker_proofs_fused(count, trackers, k_commitments, proofs, rand, partial_jac, n_invalid);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_tracker_proofs_grouped(cpx_ctx* ctx, size_t count, const uint8_t* trackers, const uint8_t* k_commitments, const uint8_t* proofs, const uint8_t* rand,
                                            int* verdict, size_t* n_rechecked) {
  if (!tracker_check_fits(count)) return CPX_ERR_ARG;   // before anything is read
  if (count && (!trackers || !k_commitments || !proofs || !rand || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_tracker_proofs_grouped(count, trackers, k_commitments, proofs, rand, verdict, n_rechecked);
    return (int)CPX_OK;
  });
}
int cpx_g1_generator_mul(cpx_ctx* ctx, size_t count, const uint8_t* scalars, uint8_t* out_affine, uint8_t* out_compressed) {
  if (count && !scalars) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->generator_mul(count, scalars, out_affine, out_compressed);
    return (int)CPX_OK;
  });
}
int cpx_whisk_trackers_from_k_r(cpx_ctx* ctx, size_t count, const uint8_t* k, const uint8_t* r, uint8_t* trackers_out, uint8_t* k_commitments_out) {
  if (count && (!k || !r)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_trackers_from_k_r(count, k, r, trackers_out, k_commitments_out);
    return (int)CPX_OK;
  });
}
int cpx_whisk_find_trackers(cpx_ctx* ctx, size_t n_trackers, const uint8_t* trackers, size_t n_keys, const uint8_t* k, uint32_t* owner, int* status) {
  if (!find_fits(n_trackers, n_keys)) return CPX_ERR_ARG;   // before anything is read
  if (n_trackers && (!trackers || !owner || !status || (n_keys && !k))) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_find_trackers(n_trackers, trackers, n_keys, k, owner, status);
    return (int)CPX_OK;
  });
}

int cpx_batch_shuffle(cpx_ctx* ctx, size_t count, const uint8_t* vec_R, const uint8_t* vec_S, const uint32_t* permutation, const uint8_t* k,
                      const uint8_t* vec_m_blinders, uint8_t* vec_T_out, uint8_t* vec_U_out, uint8_t* M_out) {
  if (count && (!vec_R || !vec_S || !permutation || !k || !vec_m_blinders)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->shuffle_batch(count, vec_R, vec_S, permutation, k, vec_m_blinders, vec_T_out, vec_U_out, M_out);
    return (int)CPX_OK;
  });
}
int cpx_whisk_generate_shuffle_proofs(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, const uint32_t* permutation, const uint8_t* k,
                                      const uint8_t* vec_m_blinders, const uint8_t* rand, uint8_t* post_trackers_out, uint8_t* proofs_out, int* status) {
  if (count && (!pre_trackers || !permutation || !k || !vec_m_blinders || !rand || !post_trackers_out || !proofs_out || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_generate_shuffle_proofs(count, pre_trackers, permutation, k, vec_m_blinders, rand, post_trackers_out, proofs_out, status);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_shuffle_proofs(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs,
                                    const uint8_t* rand, int* verdict) {
  if (count && (!pre_trackers || !post_trackers || !proofs || !rand || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_shuffle_proofs(count, pre_trackers, post_trackers, proofs, rand, verdict);
    return (int)CPX_OK;
  });
}

int cpx_whisk_verify_shuffle_proofs_grouped(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, const uint8_t* post_trackers, const uint8_t* proofs,
                                            const uint8_t* rand, int* verdict, size_t* n_rechecked) {
  if (count && (!pre_trackers || !post_trackers || !proofs || !rand || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_shuffle_proofs_grouped(count, pre_trackers, post_trackers, proofs, rand, verdict, n_rechecked);
    return (int)CPX_OK;
  });
}

// ---- the resident candidate tracker list and a run of shuffles against it (run_plan.hpp, run.hip) ----
int cpx_whisk_candidates_load(cpx_ctx* ctx, size_t n, const uint8_t* trackers, uint8_t* status) {
  if (n && !trackers) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_candidates_load(n, trackers, status);
    return (int)CPX_OK;
  });
}
size_t cpx_whisk_candidates_size(cpx_ctx* ctx) { return ctx && ctx->eng ? ctx->eng->whisk_candidates_size() : 0; }
int cpx_whisk_candidates_read(cpx_ctx* ctx, size_t first, size_t count, uint8_t* trackers_out) {
  if (count && !trackers_out) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_candidates_read(first, count, trackers_out);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_shuffle_run(cpx_ctx* ctx, size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand,
                                 int* verdict, size_t* n_applied) {
  if (count && (!indices || !post_trackers || !proofs || !rand || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_shuffle_run(count, indices, post_trackers, proofs, rand, verdict, n_applied);
    return (int)CPX_OK;
  });
}
int cpx_whisk_verify_shuffle_run_grouped(cpx_ctx* ctx, size_t count, const uint32_t* indices, const uint8_t* post_trackers, const uint8_t* proofs, const uint8_t* rand,
                                         int* verdict, size_t* n_applied, size_t* n_rechecked) {
  if (count && (!indices || !post_trackers || !proofs || !rand || !verdict)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_verify_shuffle_run_grouped(count, indices, post_trackers, proofs, rand, verdict, n_applied, n_rechecked);
    return (int)CPX_OK;
  });
}

// ---- the reference's `rng: &mut T` as ChaCha12 states (rng.hpp) ----
namespace {
RngState rng_state_from_bytes(const uint8_t b[40]) {
  uint32_t w[10];
  memcpy(w, b, sizeof w);
  return rng_state_from_words(w);
}
void rng_state_to_bytes(const RngState& s, uint8_t b[40]) {
  uint32_t w[10];
  rng_state_to_words(s, w);
  memcpy(b, w, sizeof w);
}
}  // namespace
int cpx_rng_from_u64(uint64_t seed, uint8_t state_out[40]) {
  if (!state_out) return CPX_ERR_ARG;
  rng_state_to_bytes(rng_seed_from_u64(seed), state_out);
  return CPX_OK;
}
int cpx_rng_split(uint8_t parent[40], size_t count, uint8_t* states_out) {
  if (!count) return CPX_OK;
  if (!parent || !states_out) return CPX_ERR_ARG;
  RngStream p(rng_state_from_bytes(parent));
  // (8 words per child: the position stays valid iff it does with every child drawn)
  if (!rng_pos_valid(p.st.word_pos) || count > ((size_t)1 << 28) || !rng_pos_valid(p.st.word_pos + 8 * (uint64_t)count)) return CPX_ERR_ARG;
  for (size_t i = 0; i < count; i++) rng_state_to_bytes(rng_split(p), states_out + i * RNG_STATE_BYTES);
  rng_state_to_bytes(p.st, parent);
  return CPX_OK;
}
int cpx_rng_fr(cpx_ctx* ctx, size_t count, uint8_t* states, size_t n_each, uint8_t* out) {
  if (count && n_each && (!states || !out)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->rng_fr(count, states, n_each, out);
    return (int)CPX_OK;
  });
}
int cpx_rng_g1(cpx_ctx* ctx, size_t count, uint8_t* states, size_t n_each, uint8_t* out_affine, uint8_t* out_compressed) {
  if (count && n_each && (!states || !out_affine)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->rng_g1(count, states, n_each, out_affine, out_compressed);
    return (int)CPX_OK;
  });
}
int cpx_rng_instance_draws(cpx_ctx* ctx, size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* vec_R_out, uint8_t* vec_S_out) {
  if (count && !states) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->rng_instance_draws(count, states, permutation_out, k_out, vec_R_out, vec_S_out);
    return (int)CPX_OK;
  });
}
int cpx_crs_generate(cpx_ctx* ctx, size_t ell, uint8_t state[40], uint8_t* points_out) {
  if (!state) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->crs_generate(ell, state, points_out);
    return (int)CPX_OK;
  });
}
int cpx_g1_clear_cofactor(cpx_ctx* ctx, const uint8_t* points, size_t n, uint8_t* out_affine) {
  if (n && (!points || !out_affine)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->clear_cofactor(points, n, out_affine);
    return (int)CPX_OK;
  });
}
int cpx_rng_shuffle_draws(cpx_ctx* ctx, size_t count, uint8_t* states, uint32_t* permutation_out, uint8_t* k_out, uint8_t* blinders_out, uint8_t* rand_out) {
  if (count && !states) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->rng_shuffle_draws(count, states, permutation_out, k_out, blinders_out, rand_out);
    return (int)CPX_OK;
  });
}
int cpx_whisk_generate_shuffle_proofs_rng(cpx_ctx* ctx, size_t count, const uint8_t* pre_trackers, uint8_t* states, uint8_t* post_trackers_out, uint8_t* proofs_out,
                                          int* status) {
  if (count && (!pre_trackers || !states || !post_trackers_out || !proofs_out || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->whisk_generate_shuffle_proofs_rng(count, pre_trackers, states, post_trackers_out, proofs_out, status);
    return (int)CPX_OK;
  });
}
int cpx_batch_prove_rng(cpx_ctx* ctx, const uint32_t* permutation, const uint8_t* k, const uint8_t* vec_m_blinders, uint8_t* states, uint8_t* proofs_out) {
  if (!permutation || !k || !vec_m_blinders || !states || !proofs_out) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    const size_t B = ctx->eng->batch(), ell = ctx->eng->ell();
    for (size_t i = 0; i < B * ell; i++)
      if (permutation[i] >= ell) return (int)CPX_ERR_ARG;
    ctx->eng->batch_prove_rng(permutation, k, vec_m_blinders, states, proofs_out);
    return (int)CPX_OK;
  });
}

// ---- the reference's `transcript: &mut merlin::Transcript` as a 216-byte value (transcript_state.hpp; the operations are strobe.hpp's) ----
int cpx_transcript_new(const uint8_t* label, size_t label_len, uint8_t state_out[CPX_TRANSCRIPT_BYTES]) {
  if (!state_out || (label_len && !label) || label_len > 0xffffffffu) return CPX_ERR_ARG;
  Strobe s;
  s.init(reinterpret_cast<const char*>(label_len ? label : state_out), label_len);   // (an empty label is never read)
  transcript_state_store(s, state_out);
  return CPX_OK;
}
int cpx_transcript_append_message(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, const uint8_t* msg, size_t len) {
  if (len && !msg) return CPX_ERR_ARG;
  return on_transcript(state, label, label_len, len, [&](Strobe& s, const char* l) { s.append_message(l, label_len, msg, len); });
}
int cpx_transcript_append_scalar(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, const uint8_t scalar_mont[32]) {
  if (!scalar_mont || !fr_wire_reduced(scalar_mont)) return CPX_ERR_ARG;
  uint8_t b[32];
  host::S_from_wire(scalar_mont).to_le_bytes(b);
  return on_transcript(state, label, label_len, 32, [&](Strobe& s, const char* l) { s.append_message(l, label_len, b, 32); });
}
int cpx_transcript_challenge_bytes(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, uint8_t* out, size_t len) {
  if (len && !out) return CPX_ERR_ARG;
  return on_transcript(state, label, label_len, len, [&](Strobe& s, const char* l) { s.challenge_bytes(l, label_len, out, len); });
}
int cpx_transcript_challenge_scalar(uint8_t state[CPX_TRANSCRIPT_BYTES], const uint8_t* label, size_t label_len, uint8_t out_mont[32]) {
  if (!out_mont) return CPX_ERR_ARG;
  return on_transcript(state, label, label_len, 64, [&](Strobe& s, const char* l) {
    Fr e;
    while (!s.challenge_attempt_canonical(l, label_len, e.v)) {
    }
    e = fe_to_mont(e);
    memcpy(out_mont, e.v, 32);
  });
}
int cpx_ipa_rounds(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* H, const uint8_t* vec_c, const uint8_t* vec_d,
                   uint8_t* transcripts, uint8_t* rounds_compressed, uint8_t* rounds_affine, uint8_t* finals, uint8_t* gammas) {
  if (count && n && (!G || !G_prime || !H || !vec_c || !vec_d || !transcripts || !finals)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->ipa_rounds(count, n, G, G_prime, H, vec_c, vec_d, transcripts, rounds_compressed, rounds_affine, finals, gammas);
    return (int)CPX_OK;
  });
}
int cpx_same_msm_rounds(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* vec_x, uint8_t* transcripts,
                        uint8_t* rounds_compressed, uint8_t* rounds_affine, uint8_t* finals, uint8_t* gammas) {
  if (count && n && (!G || !T || !U || !vec_x || !transcripts || !finals)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_msm_rounds(count, n, G, T, U, vec_x, transcripts, rounds_compressed, rounds_affine, finals, gammas);
    return (int)CPX_OK;
  });
}

int cpx_ipa_verify(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D, const uint8_t* z, const uint8_t* vec_u,
                   const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  if (count && n && (!G || !crs_H || !C || !D || !z || !vec_u || !proofs || !rand || !transcripts || !verdicts)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->ipa_verify(count, n, G, crs_H, C, D, z, vec_u, proofs, rand, transcripts, challenges, verdicts);
    return (int)CPX_OK;
  });
}
int cpx_same_msm_verify(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t, const uint8_t* Z_u,
                        const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  if (count && n && (!G || !T || !U || !A || !Z_t || !Z_u || !proofs || !rand || !transcripts || !verdicts)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_msm_verify(count, n, G, T, U, A, Z_t, Z_u, proofs, rand, transcripts, challenges, verdicts);
    return (int)CPX_OK;
  });
}

int cpx_ipa_prove(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D,
                  const uint8_t* z, const uint8_t* vec_c, const uint8_t* vec_d, const uint8_t* rand, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges,
                  int* status) {
  if (count && n && (!G || !G_prime || !crs_H || !C || !D || !z || !vec_c || !vec_d || !rand || !transcripts || !proofs || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->ipa_prove(count, n, G, G_prime, crs_H, C, D, z, vec_c, vec_d, rand, nullptr, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_ipa_prove_rng(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* G_prime, const uint8_t* crs_H, const uint8_t* C, const uint8_t* D,
                      const uint8_t* z, const uint8_t* vec_c, const uint8_t* vec_d, uint8_t* states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges,
                      int* status) {
  if (count && n && (!G || !G_prime || !crs_H || !C || !D || !z || !vec_c || !vec_d || !states || !transcripts || !proofs || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->ipa_prove(count, n, G, G_prime, crs_H, C, D, z, vec_c, vec_d, nullptr, states, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_same_msm_prove(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t,
                       const uint8_t* Z_u, const uint8_t* vec_x, const uint8_t* rand, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  if (count && n && (!G || !T || !U || !A || !Z_t || !Z_u || !vec_x || !rand || !transcripts || !proofs || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_msm_prove(count, n, G, T, U, A, Z_t, Z_u, vec_x, rand, nullptr, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_same_msm_prove_rng(cpx_ctx* ctx, size_t count, size_t n, const uint8_t* G, const uint8_t* T, const uint8_t* U, const uint8_t* A, const uint8_t* Z_t,
                           const uint8_t* Z_u, const uint8_t* vec_x, uint8_t* states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  if (count && n && (!G || !T || !U || !A || !Z_t || !Z_u || !vec_x || !states || !transcripts || !proofs || !status)) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_msm_prove(count, n, G, T, U, A, Z_t, Z_u, vec_x, nullptr, states, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_gprod_prove(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
                    const uint8_t* gprod_result, const uint8_t* vec_b, const uint8_t* vec_b_blinders, const uint8_t* rand, uint8_t* transcripts, uint8_t* proofs,
                    uint8_t* challenges, int* status) {
  if (count && ell &&
      (!G || (n_blinders && (!H || !vec_b_blinders)) || !crs_U || !B || !gprod_result || !vec_b || !rand || !transcripts || !proofs || !status))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->gprod_prove(count, ell, n_blinders, G, H, crs_U, B, gprod_result, vec_b, vec_b_blinders, rand, nullptr, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_gprod_prove_rng(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* B,
                        const uint8_t* gprod_result, const uint8_t* vec_b, const uint8_t* vec_b_blinders, uint8_t* states, uint8_t* transcripts, uint8_t* proofs,
                        uint8_t* challenges, int* status) {
  if (count && ell &&
      (!G || (n_blinders && (!H || !vec_b_blinders)) || !crs_U || !B || !gprod_result || !vec_b || !states || !transcripts || !proofs || !status))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->gprod_prove(count, ell, n_blinders, G, H, crs_U, B, gprod_result, vec_b, vec_b_blinders, nullptr, states, transcripts, proofs, challenges, status);
    return (int)CPX_OK;
  });
}
int cpx_gprod_verify(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                     const uint8_t* crs_H_sum, const uint8_t* B, const uint8_t* gprod_result, const uint8_t* proofs, const uint8_t* rand, uint8_t* transcripts,
                     uint8_t* challenges, int* verdicts) {
  if (count && ell && (!G || (n_blinders && !H) || !crs_U || !crs_G_sum || !crs_H_sum || !B || !gprod_result || !proofs || !rand || !transcripts || !verdicts))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->gprod_verify(count, ell, n_blinders, G, H, crs_U, crs_G_sum, crs_H_sum, B, gprod_result, proofs, rand, transcripts, challenges, verdicts);
    return (int)CPX_OK;
  });
}
int cpx_same_perm_prove(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A,
                        const uint8_t* M, const uint8_t* vec_a, const uint32_t* permutation, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders,
                        const uint8_t* rand, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  if (count && ell &&
      (!G || (n_blinders && (!H || !vec_a_blinders || !vec_m_blinders)) || !crs_U || !A || !M || !vec_a || !permutation || !rand || !transcripts || !proofs || !status))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_perm_prove(count, ell, n_blinders, G, H, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders, rand, nullptr, transcripts, proofs, challenges,
                              status);
    return (int)CPX_OK;
  });
}
int cpx_same_perm_prove_rng(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* A,
                            const uint8_t* M, const uint8_t* vec_a, const uint32_t* permutation, const uint8_t* vec_a_blinders, const uint8_t* vec_m_blinders,
                            uint8_t* states, uint8_t* transcripts, uint8_t* proofs, uint8_t* challenges, int* status) {
  if (count && ell &&
      (!G || (n_blinders && (!H || !vec_a_blinders || !vec_m_blinders)) || !crs_U || !A || !M || !vec_a || !permutation || !states || !transcripts || !proofs || !status))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_perm_prove(count, ell, n_blinders, G, H, crs_U, A, M, vec_a, permutation, vec_a_blinders, vec_m_blinders, nullptr, states, transcripts, proofs, challenges,
                              status);
    return (int)CPX_OK;
  });
}
int cpx_same_perm_verify(cpx_ctx* ctx, size_t count, size_t ell, size_t n_blinders, const uint8_t* G, const uint8_t* H, const uint8_t* crs_U, const uint8_t* crs_G_sum,
                         const uint8_t* crs_H_sum, const uint8_t* A, const uint8_t* M, const uint8_t* vec_a, const uint8_t* proofs, const uint8_t* rand,
                         uint8_t* transcripts, uint8_t* challenges, int* verdicts) {
  if (count && ell && (!G || (n_blinders && !H) || !crs_U || !crs_G_sum || !crs_H_sum || !A || !M || !vec_a || !proofs || !rand || !transcripts || !verdicts))
    return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    ctx->eng->same_perm_verify(count, ell, n_blinders, G, H, crs_U, crs_G_sum, crs_H_sum, A, M, vec_a, proofs, rand, transcripts, challenges, verdicts);
    return (int)CPX_OK;
  });
}

int cpx_set_profiling(cpx_ctx* ctx, int on) {
  if (!ctx || !ctx->eng) return CPX_ERR_ARG;
  ctx->eng->set_profiling(on != 0);
  return CPX_OK;
}
int cpx_reset_stats(cpx_ctx* ctx) {
  if (!ctx || !ctx->eng) return CPX_ERR_ARG;
  ctx->eng->reset_stats();
  return CPX_OK;
}
int cpx_get_stat(const cpx_ctx* ctx, const char* name, uint64_t* launches, double* total_ms, double* algorithmic_bytes, double* units) {
  if (!ctx || !ctx->eng || !name) return CPX_ERR_ARG;
  auto& m = ctx->eng->stats();
  auto it = m.find(name);
  KernelStat st;
  if (it != m.end()) st = it->second;
  if (launches) *launches = st.launches;
  if (total_ms) *total_ms = st.ms;
  if (algorithmic_bytes) *algorithmic_bytes = st.alg_bytes;
  if (units) *units = st.units;
  return CPX_OK;
}
int cpx_set_host_threads(cpx_ctx* ctx, int threads) {
  if (!ctx || !ctx->eng) return CPX_ERR_ARG;
  ctx->eng->set_host_threads(threads);
  return CPX_OK;
}
int cpx_bench_fpmul(cpx_ctx* ctx, int blocks, int iters, int reps, double* products_per_second) {
  if (!products_per_second || blocks <= 0 || iters <= 0 || reps <= 0) return CPX_ERR_ARG;
  return guarded(ctx, [&] {
    *products_per_second = ctx->eng->bench_fpmul(blocks, iters, reps);
    return CPX_OK;
  });
}

}  // extern "C"
