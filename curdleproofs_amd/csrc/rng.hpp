// The randomness source of the reference's provers, word for word: rand 0.8 `StdRng` = `ChaCha12Rng` and the samplers the reference draws
// from it (whisk.rs:144-179: `SliceRandom::shuffle`, `Fr::rand`) — product code, host and device.
//
//   block      constants "expand 32-byte k", the key in words 4..11, a 64-bit block counter in words 12 / 13, words 14 / 15 (the stream
//              id) zero, 12 rounds, the input added to the result
//   stream     the u32 words of block 0, block 1, ... back to back, addressed by word_pos: block = word_pos >> 4, index = word_pos & 15.
//              `BlockRng` consumes whole words: next_u32 takes one, next_u64 two (low word first, across a block boundary as anywhere
//              else), fill_bytes of 4 k bytes k of them
//   Fr::rand   four u64 least significant limb first, the top bit of the last limb cleared (255-bit modulus), drawn again while the
//              value is >= r; the limbs ARE the Montgomery form (ark-ff `UniformRand` for `Fp<MontBackend>`)
//   gen_range  rand 0.8 `UniformInt<u32>::sample_single(0, range)`: widening multiply of one u32 by the range, accepted when the low
//              half is <= zone = (range << clz(range)) - 1
//   shuffle    rand 0.8 `SliceRandom::shuffle`: i from len - 1 down to 1, j = gen_range(0..i + 1), swap(i, j)
//   G1::rand   ark-ec 0.4 `Projective::rand` (recalled; the reference's known-answer test pins it through the oracle): a loop over TOKENS.
//              A candidate is six u64 least significant limb first, the top three bits cleared (381-bit modulus); a value >= p is
//              rejected and nothing else is drawn for it.  An accepted candidate — its limbs ARE the Montgomery form of x — is followed
//              by ONE word whose top bit is `greatest` (rand's `Standard` for bool), whether or not x^3 + 4 is a square; where it is, the
//              draw is [h](x, y) with y the larger of (y, p - y) iff `greatest` and h the full cofactor (g1_28.hpp).  Where a token ends
//              depends on the compare with p alone: rng_g1_candidate walks tokens, the square roots are somebody else's work
//   seed       rand_core 0.6 `SeedableRng::seed_from_u64`: eight PCG32 outputs are the key, word_pos = 0
//   split      `ChaCha12Rng::from_rng(&mut parent)`: the child's key is the next eight words of the parent, its word_pos is 0
//
// A state is (key, word_pos): `ChaCha12Rng::get_seed()` and the low 64 bits of `get_word_pos()`, 40 bytes on the wire (key bytes, then
// word_pos little-endian).  States whose word_pos is within 2^32 words of 2^64 are refused at the boundary (rng_pos_valid): no draw
// sequence of one call wraps the position.
//
// The samplers are templates over a word source (anything with next_u32()); RngStream is the plain one, a block at a time.  k_rng_draw
// (rng.hip) fills a window of blocks per wave and runs the same acceptance tests (rng_fr_accept, rng_range_accept) on it.
#pragma once
#include <stdint.h>
#include "mont32.hpp"

namespace cpx {

constexpr int RNG_STATE_BYTES = 40;
constexpr int RNG_BLOCK_WORDS = 16;
constexpr int RNG_FR_WORDS = 8;   // u32 words of one Fr::rand candidate
constexpr int RNG_FP_WORDS = 12;  // u32 words of one Fp::rand candidate (the x of a G1::rand token)

CPX_HD bool rng_pos_valid(uint64_t word_pos) { return word_pos < 0xffffffff00000000ull; }

CPX_HD uint32_t rng_rotl(uint32_t x, int n) {   // n in 1..31
#if defined(__HIPCC__) || defined(__clang__)
  return __builtin_rotateleft32(x, (uint32_t)n);
#else
  return (x << n) | (x >> (32 - n));
#endif
}

#define CPX_RNG_QR(a, b, c, d)        \
  a += b; d = rng_rotl(d ^ a, 16);    \
  c += d; b = rng_rotl(b ^ c, 12);    \
  a += b; d = rng_rotl(d ^ a, 8);     \
  c += d; b = rng_rotl(b ^ c, 7);

// one block of the ChaCha12 key stream
CPX_HD void chacha12_block(const uint32_t key[8], uint64_t counter, uint32_t out[RNG_BLOCK_WORDS]) {
  const uint32_t c0 = 0x61707865u, c1 = 0x3320646eu, c2 = 0x79622d32u, c3 = 0x6b206574u;   // "expand 32-byte k"
  const uint32_t n0 = (uint32_t)counter, n1 = (uint32_t)(counter >> 32);
  uint32_t x0 = c0, x1 = c1, x2 = c2, x3 = c3, x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7],
           x12 = n0, x13 = n1, x14 = 0, x15 = 0;
  for (int r = 0; r < 6; r++) {   // 6 double rounds
    CPX_RNG_QR(x0, x4, x8, x12) CPX_RNG_QR(x1, x5, x9, x13) CPX_RNG_QR(x2, x6, x10, x14) CPX_RNG_QR(x3, x7, x11, x15)
    CPX_RNG_QR(x0, x5, x10, x15) CPX_RNG_QR(x1, x6, x11, x12) CPX_RNG_QR(x2, x7, x8, x13) CPX_RNG_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + c0;
  out[1] = x1 + c1;
  out[2] = x2 + c2;
  out[3] = x3 + c3;
  out[4] = x4 + key[0];
  out[5] = x5 + key[1];
  out[6] = x6 + key[2];
  out[7] = x7 + key[3];
  out[8] = x8 + key[4];
  out[9] = x9 + key[5];
  out[10] = x10 + key[6];
  out[11] = x11 + key[7];
  out[12] = x12 + n0;
  out[13] = x13 + n1;
  out[14] = x14;
  out[15] = x15;
}
#undef CPX_RNG_QR

struct RngState {
  uint32_t key[8];
  uint64_t word_pos;
};
// the 40 wire bytes as ten little-endian words (the callers' buffers are word-aligned on the device; the host copies bytes)
CPX_HD RngState rng_state_from_words(const uint32_t w[10]) {
  RngState s;
  for (int i = 0; i < 8; i++) s.key[i] = w[i];
  s.word_pos = (uint64_t)w[8] | ((uint64_t)w[9] << 32);
  return s;
}
CPX_HD void rng_state_to_words(const RngState& s, uint32_t w[10]) {
  for (int i = 0; i < 8; i++) w[i] = s.key[i];
  w[8] = (uint32_t)s.word_pos;
  w[9] = (uint32_t)(s.word_pos >> 32);
}

// The word stream read in order, one block cached.
struct RngStream {
  RngState st;
  uint64_t cached;   // block held in buf; ~0: none
  uint32_t buf[RNG_BLOCK_WORDS];
  CPX_HD explicit RngStream(const RngState& s) : st(s), cached(~(uint64_t)0) {}
  CPX_HD uint32_t next_u32() {
    const uint64_t blk = st.word_pos >> 4;
    if (blk != cached) {
      chacha12_block(st.key, blk, buf);
      cached = blk;
    }
    return buf[st.word_pos++ & 15];
  }
};

template <class W> CPX_HD uint64_t rng_next_u64(W& w) {
  const uint64_t lo = w.next_u32();
  const uint64_t hi = w.next_u32();
  return lo | (hi << 32);
}

// One Fr::rand candidate: the eight words as they come off the stream.  Clears the top bit in place; true iff the value is below r.
CPX_HD bool rng_fr_accept(uint32_t limbs[RNG_FR_WORDS]) {
  limbs[7] &= 0x7fffffffu;
  bool lt = false, decided = false;
  for (int i = 7; i >= 0; i--) {
    const uint32_t p = FrCfg::P[i];
    const bool ne = limbs[i] != p;
    if (!decided && ne) lt = limbs[i] < p;
    decided = decided || ne;
  }
  return lt;   // equal to r: rejected
}
template <class W> CPX_HD void rng_fr(W& w, uint32_t out[RNG_FR_WORDS]) {
  for (;;) {
    for (int i = 0; i < RNG_FR_WORDS; i++) out[i] = w.next_u32();   // four next_u64, low word first
    if (rng_fr_accept(out)) return;
  }
}

// One Fp::rand candidate: the twelve words as they come off the stream.  Clears the top three bits in place; true iff the value is below p.
CPX_HD bool rng_fp_accept(uint32_t limbs[RNG_FP_WORDS]) {
  limbs[11] &= 0x1fffffffu;
  bool lt = false, decided = false;
  for (int i = 11; i >= 0; i--) {
    const uint32_t p = FpCfg::P[i];
    const bool ne = limbs[i] != p;
    if (!decided && ne) lt = limbs[i] < p;
    decided = decided || ne;
  }
  return lt;   // equal to p: rejected
}
// One accepted token of G1::rand: x (Montgomery limbs) and the bool drawn behind it; rejected candidates are walked over
template <class W> CPX_HD void rng_g1_candidate(W& w, uint32_t x[RNG_FP_WORDS], bool& greatest) {
  for (;;) {
    for (int i = 0; i < RNG_FP_WORDS; i++) x[i] = w.next_u32();   // six next_u64, low word first
    if (rng_fp_accept(x)) break;
  }
  greatest = (w.next_u32() >> 31) != 0;   // rand 0.8 Standard for bool: the most significant bit of one u32
}

// sample_single(0, range), range >= 1
CPX_HD uint32_t rng_range_zone(uint32_t range) { return (range << __builtin_clz(range)) - 1u; }
CPX_HD bool rng_range_accept(uint32_t v, uint32_t range, uint32_t zone, uint32_t& hi) {
  const uint64_t m = (uint64_t)v * range;
  hi = (uint32_t)(m >> 32);
  return (uint32_t)m <= zone;
}
template <class W> CPX_HD uint32_t rng_gen_range(W& w, uint32_t range) {
  const uint32_t zone = rng_range_zone(range);
  for (;;) {
    uint32_t hi;
    if (rng_range_accept(w.next_u32(), range, zone, hi)) return hi;
  }
}
template <class W, class T> CPX_HD void rng_shuffle(W& w, T* v, uint32_t len) {
  for (uint32_t i = len; i-- > 1;) {
    const uint32_t j = rng_gen_range(w, i + 1);
    const T t = v[i];
    v[i] = v[j];
    v[j] = t;
  }
}

// SeedableRng::seed_from_u64: PCG32 (XSH RR) expands the u64 into the key
CPX_HD RngState rng_seed_from_u64(uint64_t seed) {
  const uint64_t MUL = 6364136223846793005ull, INC = 11634580027462260723ull;
  RngState s;
  uint64_t state = seed;
  for (int i = 0; i < 8; i++) {
    state = state * MUL + INC;
    const uint32_t xorshifted = (uint32_t)(((state >> 18) ^ state) >> 27);
    const uint32_t rot = (uint32_t)(state >> 59);
    s.key[i] = (xorshifted >> rot) | (xorshifted << ((32 - rot) & 31));
  }
  s.word_pos = 0;
  return s;
}
// from_rng(&mut parent): fill_bytes of the 32-byte seed = eight words of the parent
template <class W> CPX_HD RngState rng_split(W& parent) {
  RngState c;
  for (int i = 0; i < 8; i++) c.key[i] = parent.next_u32();
  c.word_pos = 0;
  return c;
}

}  // namespace cpx
