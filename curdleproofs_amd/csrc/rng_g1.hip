// gfx950 kernels of the G1::rand draws (ark-ec `G1Projective::rand` from a ChaCha12 state: crs.rs:61-69 generate_crs, the README's vec_R /
// vec_S) and of the cofactor multiplication.  The token format is in rng.hpp, the point arithmetic in g1_28.hpp, the shape of a round and
// the scratch records in rng_g1_plan.hpp.
//
//  k_rng_g1_scan     one wave per stream.  The wave keeps a window of RNG_G1_WINDOW_BLOCKS blocks of the word stream in LDS, one ChaCha12
//                    block per lane (the window and `fill` of k_rng_draw).  Lane 0 walks the tokens — twelve words, the compare with p, one
//                    more word behind an accepted candidate: about 31 stream words per point — and notes where the accepted ones lie; all
//                    lanes copy them out.  A token that does not lie wholly inside the window (its twelve words, or its bool word) is not
//                    consumed: the next window starts at the block of that token's first word.
//  k_rng_g1_sqrt     one lane per emitted candidate of all streams of the chunk: g1_28_point_from_x, the square root out of line as in
//                    k_decompress.
//  k_rng_g1_select   one wave per stream: ballot + popcount prefix over the hit flags, 64 candidates a trip.
//  k_clear_cofactor  one lane per output slot: g1_28_clear_cofactor, then one inversion per work-group (block_inverse.hpp).  Also the
//                    kernel of cpx_g1_clear_cofactor, which feeds it standard-form points instead of the selection's list.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "kernels.h"
#include "block_inverse.hpp"
#include "rng_g1_plan.hpp"

namespace cpx {

constexpr int RNG_G1_THREADS = 64;   // one wave
static_assert(RNG_G1_WINDOW_BLOCKS == RNG_G1_THREADS, "the window holds one block per lane");

__global__ __launch_bounds__(RNG_G1_THREADS) void k_rng_g1_scan(RngG1Args a) {
  __shared__ __attribute__((aligned(16))) uint32_t win[RNG_G1_WINDOW_WORDS];
  __shared__ uint16_t tok[RNG_G1_WINDOW_TOKENS];   // first word of every accepted token of the window
  __shared__ uint64_t sh_pos;
  __shared__ uint32_t sh_n;
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  RngG1Stream& st = a.streams[s];
  uint64_t pos = st.pos;
  const uint32_t owed = st.shortfall;
  if (!owed) {   // (uniform over the wave)
    if (lane == 0) {
      st.emitted = 0;
      st.stop = pos;
    }
    return;
  }
  uint32_t want = rng_g1_cap(owed, a.round_cap);
  if (want > a.cap) want = a.cap;   // (the row holds cap(n_each) >= cap(owed) candidates: never taken)
  const uint32_t* const key_words = reinterpret_cast<const uint32_t*>(a.states + (size_t)s * RNG_STATE_BYTES);
  uint32_t key[8];
  for (int i = 0; i < 8; i++) key[i] = key_words[i];
  RngG1Cand* const row = a.cand + (size_t)s * a.cap;
  uint32_t emitted = 0;
  while (emitted < want) {
    const uint64_t base = (pos >> 4) << 4;
    {   // blocks pos >> 4 .. + 63 of the stream into win (the previous window is no longer read: the trip ends with a barrier)
      uint32_t o[RNG_BLOCK_WORDS];
      chacha12_block(key, (pos >> 4) + lane, o);
      uint4* dst = reinterpret_cast<uint4*>(win + lane * RNG_BLOCK_WORDS);
      for (int q = 0; q < 4; q++) dst[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
    __syncthreads();
    if (lane == 0) {
      uint32_t n = 0;
      while (emitted + n < want) {
        const uint32_t off = (uint32_t)(pos - base);
        if (off + RNG_FP_WORDS > (uint32_t)RNG_G1_WINDOW_WORDS) break;
        uint32_t c[RNG_FP_WORDS];
        for (int i = 0; i < RNG_FP_WORDS; i++) c[i] = win[off + i];
        if (!rng_fp_accept(c)) {
          pos += RNG_FP_WORDS;
          continue;
        }
        if (off + RNG_G1_TOKEN_WORDS > (uint32_t)RNG_G1_WINDOW_WORDS) break;   // its bool word is the next window's
        tok[n++] = (uint16_t)off;
        pos += RNG_G1_TOKEN_WORDS;
      }
      sh_n = n;
      sh_pos = pos;
    }
    __syncthreads();
    const uint32_t n = sh_n;
    pos = sh_pos;
    for (uint32_t idx = lane; idx < n * RNG_FP_WORDS; idx += RNG_G1_THREADS) {
      const uint32_t t = idx / RNG_FP_WORDS, i = idx % RNG_FP_WORDS;
      const uint32_t w = win[tok[t] + i];
      row[emitted + t].x[i] = i == RNG_FP_WORDS - 1 ? (w & 0x1fffffffu) : w;
    }
    for (uint32_t t = lane; t < n; t += RNG_G1_THREADS) {
      row[emitted + t].greatest = win[tok[t] + RNG_FP_WORDS] >> 31;
      row[emitted + t].after = base + tok[t] + RNG_G1_TOKEN_WORDS;
    }
    emitted += n;
    __syncthreads();
  }
  if (lane == 0) {
    st.emitted = emitted;
    st.stop = pos;
  }
}

static __device__ __noinline__ F28 f28_sqrt_out_of_line(const F28& a) { return f28_sqrt_candidate(a); }

__global__ __launch_bounds__(RNG_G1_THREADS, 2) void k_rng_g1_sqrt(RngG1Args a) {
  const size_t g = (size_t)blockIdx.x * RNG_G1_THREADS + threadIdx.x;
  const size_t s = g / a.cap;
  if (s >= a.nstreams || (uint32_t)(g % a.cap) >= a.streams[s].emitted) return;
  RngG1Cand& c = a.cand[g];
  Fp x;
  for (int i = 0; i < RNG_FP_WORDS; i++) x.v[i] = c.x[i];
  Aff28 p;
  const bool greatest = c.greatest & 1u;
  const bool hit = g1_28_point_from_x_with(f28_from_std(x), greatest, &p, [](const F28& v) { return f28_sqrt_out_of_line(v); });
  if (hit) a.pts[g] = p;
  c.greatest = (greatest ? 1u : 0u) | (hit ? RNG_G1_HIT : 0u);
}

__global__ __launch_bounds__(RNG_G1_THREADS) void k_rng_g1_select(RngG1Args a) {
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  RngG1Stream& st = a.streams[s];
  uint32_t* const sel = a.sel + (size_t)s * a.n_each;
  for (uint32_t j = lane; j < a.n_each; j += RNG_G1_THREADS) sel[j] = RNG_G1_NONE;
  const uint32_t owed = st.shortfall, done = st.done, emitted = st.emitted;
  if (!owed) {
    if (lane == 0) a.shortfall[s] = 0;
    return;
  }
  __syncthreads();
  const size_t row = (size_t)s * a.cap;
  uint32_t hits = 0;
  for (uint32_t j0 = 0; j0 < emitted && hits < owed; j0 += RNG_G1_THREADS) {
    const uint32_t j = j0 + lane;
    const bool hit = j < emitted && (a.cand[row + j].greatest & RNG_G1_HIT);
    const unsigned long long votes = __ballot(hit);
    const uint32_t h = hits + (uint32_t)__popcll(votes & ((1ull << lane) - 1ull));
    if (hit && h < owed) {
      sel[done + h] = (uint32_t)(row + j);
      if (h == owed - 1) st.pos = a.cand[row + j].after;   // the stream ends behind the candidate that supplied its last point
    }
    hits += (uint32_t)__popcll(votes);
  }
  if (lane == 0) {
    if (hits >= owed) {
      st.done = done + owed;
      st.shortfall = 0;
      a.shortfall[s] = 0;
    } else {
      st.pos = st.stop;
      st.done = done + hits;
      st.shortfall = owed - hits;
      a.shortfall[s] = owed - hits;
    }
  }
}

static __device__ __noinline__ Jac28 g1_clear_cofactor_device(const Aff28& p) { return g1_28_clear_cofactor(p); }

// slot g: sel != null: the candidate sel[g] of pts (RNG_G1_NONE: nothing to do this round); sel == null: std_in[g]
__global__ __launch_bounds__(RNG_G1_THREADS, 2) void k_clear_cofactor(const uint32_t* __restrict__ sel, const Aff28* __restrict__ pts, const Aff* __restrict__ std_in,
                                                                  size_t n, Aff* __restrict__ out) {
  __shared__ TF inv_buf[2 * RNG_G1_THREADS];
  const size_t g = (size_t)blockIdx.x * RNG_G1_THREADS + threadIdx.x;
  uint32_t src = RNG_G1_NONE;
  if (g < n) src = sel ? sel[g] : (uint32_t)g;
  const bool live = g < n && (!sel || src != RNG_G1_NONE);
  Aff28 p = Aff28::identity();
  if (live) p = sel ? pts[src] : t_from_std(std_in[g]);
  const Jac28 q = g1_clear_cofactor_device(p);
  const bool inf = q.is_identity();
  const TF zinv = t_block_batch_inverse(q.z, inv_buf);
  if (live) out[g] = inf ? Aff::identity() : t_to_std(t_to_affine(q, zinv));
}

template <class K, class... A> static void launch_timed(K k, dim3 grid, size_t lds, hipStream_t s, A... args) {
  hipEvent_t ea = nullptr, eb = nullptr;
  take_launch_events(&ea, &eb);
  if (ea || eb) hipExtLaunchKernelGGL(k, grid, dim3(RNG_G1_THREADS), lds, s, ea, eb, 0, args...);
  else hipLaunchKernelGGL(k, grid, dim3(RNG_G1_THREADS), lds, s, args...);
}

void launch_rng_g1_scan(const RngG1Args& a, hipStream_t s) {
  if (a.nstreams) launch_timed(k_rng_g1_scan, dim3(a.nstreams), 0, s, a);
}
void launch_rng_g1_sqrt(const RngG1Args& a, hipStream_t s) {
  const size_t n = (size_t)a.nstreams * a.cap;
  if (n) launch_timed(k_rng_g1_sqrt, dim3((unsigned)((n + RNG_G1_THREADS - 1) / RNG_G1_THREADS)), 0, s, a);
}
void launch_rng_g1_select(const RngG1Args& a, hipStream_t s) {
  if (a.nstreams) launch_timed(k_rng_g1_select, dim3(a.nstreams), 0, s, a);
}
void launch_clear_cofactor(const uint32_t* d_sel, const Aff28* d_pts, const Aff* d_std_in, size_t n, Aff* d_out, hipStream_t s) {
  if (n) launch_timed(k_clear_cofactor, dim3((unsigned)((n + RNG_G1_THREADS - 1) / RNG_G1_THREADS)), 0, s, d_sel, d_pts, d_std_in, n, d_out);
}

}  // namespace cpx
