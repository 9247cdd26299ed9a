// gfx950 kernel of the prover's random draws (rng.hpp: the reference's StdRng and its samplers; whisk.rs:144-179 draws the permutation, k,
// the blinders and the 3n + 9 scalars of CurdleproofsProof::new in this order).
//
//  k_rng_draw    one wave per stream runs a short program: an optional `shuffle` of 0..len, then up to RNG_MAX_FR_PHASES phases of Fr::rand.
//                The wave keeps a window of the word stream in LDS, one ChaCha12 block per lane.
//                Shuffle: lane 0 walks the window word by word, one gen_range trial per word, and swaps on a permutation held in LDS; how
//                many words that takes depends on the zone rejections, so the window is refilled from wherever the walk stopped until the
//                permutation is done.
//                Fr: candidate j of a window is the eight words at position + 8 j — any residue mod 16, so candidates straddle block
//                boundaries.  Lane j masks and compares candidate j; the 64-bit ballot and a popcount prefix give every accepted candidate its
//                output index; the phase ends just behind the candidate that supplied its last draw, the next window starts behind the 64th.
//                The draws go straight to the arrays of the caller (the prover's perm / k / mbl / rnd, the shuffle step's perm / fr).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include "kernels.h"
#include "rng.hpp"

namespace cpx {

constexpr int RNG_THREADS = 64;                                  // one wave
constexpr int RNG_WINDOW_BLOCKS = 64;                            // the shuffle's window: one block per lane
constexpr int RNG_WINDOW_WORDS = RNG_WINDOW_BLOCKS * RNG_BLOCK_WORDS;
constexpr int RNG_FR_BLOCKS = (15 + 64 * RNG_FR_WORDS + 15) / 16;   // 64 candidates from any word offset: 34 blocks
static_assert(RNG_FR_BLOCKS <= RNG_WINDOW_BLOCKS, "the Fr window fits the LDS window");

__global__ __launch_bounds__(RNG_THREADS) void k_rng_draw(RngDrawArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t win[RNG_WINDOW_WORDS];
  __shared__ uint64_t sh_pos;
  __shared__ uint32_t sh_i;
  extern __shared__ __attribute__((aligned(16))) uint32_t perm[];   // shuffle_len entries
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  uint32_t* const st_words = reinterpret_cast<uint32_t*>(a.states + (size_t)s * RNG_STATE_BYTES);
  uint32_t w10[10];
  for (int i = 0; i < 10; i++) w10[i] = st_words[i];
  RngState st = rng_state_from_words(w10);
  uint64_t pos = st.word_pos;

  // blocks first .. first + nblocks - 1 of the stream into win (the previous window is no longer read: every user ends with a barrier)
  const auto fill = [&](uint64_t first, uint32_t nblocks) {
    if (lane < nblocks) {
      uint32_t o[RNG_BLOCK_WORDS];
      chacha12_block(st.key, first + lane, o);
      uint4* dst = reinterpret_cast<uint4*>(win + lane * RNG_BLOCK_WORDS);
      for (int q = 0; q < 4; q++) dst[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
    }
    __syncthreads();
  };

  if (a.shuffle_len) {
    const uint32_t len = a.shuffle_len;
    for (uint32_t j = lane; j < len; j += RNG_THREADS) perm[j] = j;
    uint32_t i = len - 1;   // the element the next accepted trial places; 0: done
    while (i >= 1) {
      const uint64_t base = (pos >> 4) << 4;
      fill(pos >> 4, RNG_WINDOW_BLOCKS);   // (its barrier also publishes the identity permutation)
      if (lane == 0) {
        uint32_t zone = rng_range_zone(i + 1);
        while (i >= 1 && pos - base < (uint64_t)RNG_WINDOW_WORDS) {
          uint32_t hi;
          if (rng_range_accept(win[pos - base], i + 1, zone, hi)) {
            const uint32_t t = perm[i];
            perm[i] = perm[hi];
            perm[hi] = t;
            i--;
            zone = rng_range_zone(i + 1);
          }
          pos++;
        }
        sh_pos = pos;
        sh_i = i;
      }
      __syncthreads();
      pos = sh_pos;
      i = sh_i;
      __syncthreads();
    }
    __syncthreads();   // (len <= 1: no trip above)
    uint32_t* out = a.perm + (size_t)s * len;
    for (uint32_t j = lane; j < len; j += RNG_THREADS) out[j] = perm[j];
  }

  for (int ph = 0; ph < a.nfr; ph++) {
    uint32_t need = a.fr_cnt[ph], done = 0;
    uint32_t* out = reinterpret_cast<uint32_t*>(a.fr_out[ph]) + (size_t)s * a.fr_cnt[ph] * RNG_FR_WORDS;
    while (need) {
      const uint32_t off = (uint32_t)(pos & 15);
      fill(pos >> 4, RNG_FR_BLOCKS);
      uint32_t c[RNG_FR_WORDS];
      for (int i = 0; i < RNG_FR_WORDS; i++) c[i] = win[off + RNG_FR_WORDS * lane + i];
      const bool acc = rng_fr_accept(c);
      const unsigned long long votes = __ballot(acc);
      const uint32_t before = (uint32_t)__popcll(votes & ((1ull << lane) - 1ull)), total = (uint32_t)__popcll(votes);
      if (acc && before < need) {
        uint4* o = reinterpret_cast<uint4*>(out + (size_t)(done + before) * RNG_FR_WORDS);   // (an Fr array: 32-byte aligned)
        o[0] = make_uint4(c[0], c[1], c[2], c[3]);
        o[1] = make_uint4(c[4], c[5], c[6], c[7]);
      }
      if (total >= need) {   // the phase ends behind the candidate that supplied its last draw
        const unsigned long long last = __ballot(acc && before == need - 1);
        pos += (uint64_t)RNG_FR_WORDS * (uint32_t)__ffsll((long long)last);
        need = 0;
      } else {
        pos += (uint64_t)RNG_FR_WORDS * RNG_THREADS;
        done += total;
        need -= total;
      }
      __syncthreads();
    }
    if (ph == a.mid_phase && a.states_mid && lane == 0) {
      st.word_pos = pos;
      rng_state_to_words(st, w10);
      uint32_t* m = reinterpret_cast<uint32_t*>(a.states_mid + (size_t)s * RNG_STATE_BYTES);
      for (int i = 0; i < 10; i++) m[i] = w10[i];
    }
  }
  if (lane == 0) {
    st_words[8] = (uint32_t)pos;
    st_words[9] = (uint32_t)(pos >> 32);
  }
}

size_t rng_draw_max_shuffle() { return (size_t)12288; }   // 48 KiB of permutation beside the 4 KiB window: within the 64 KiB a work-group gets without opting in

void launch_rng_draw(const RngDrawArgs& a, hipStream_t s) {
  if (!a.count) return;
  hipEvent_t ea = nullptr, eb = nullptr;
  take_launch_events(&ea, &eb);
  const size_t lds = (size_t)a.shuffle_len * sizeof(uint32_t);
  if (ea || eb) hipExtLaunchKernelGGL(k_rng_draw, dim3(a.count), dim3(RNG_THREADS), lds, s, ea, eb, 0, a);
  else hipLaunchKernelGGL(k_rng_draw, dim3(a.count), dim3(RNG_THREADS), lds, s, a);
}

}  // namespace cpx
