// Launch plan of the G1::rand draws (rng_g1.hip; the token format in rng.hpp, the point arithmetic in g1_28.hpp) — plain C++, shared by the
// kernels, the host loop (Engine::rng_g1, whisk.cpp) and the tests' model of the scan window.
//
// Every stream needs `need` points.  A round is four launches over a chunk of streams:
//   k_rng_g1_scan     one wave per stream walks tokens from the stream's position and emits up to cap(shortfall) ACCEPTED candidates
//                     (x, greatest, the position behind the token) into the stream's row of the candidate scratch
//   k_rng_g1_sqrt     one lane per emitted candidate of the whole chunk: the square root, a hit flag and the affine point
//   k_rng_g1_select   one wave per stream: hit number j < shortfall takes output slot done + j; enough hits: the stream's position is the one
//                     behind the candidate that supplied its last point, later candidates are discarded unread; too few: the stream resumes
//                     at the scan's stop position with the shortfall that is left
//   k_clear_cofactor  one lane per output slot of the chunk through the slot -> candidate list the selection wrote: [h] P, one inversion
//                     per work-group, standard-form affine to the slot
// and the host reads the chunk's shortfall counts — nothing else — to learn whether another round is due.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "g1_28.hpp"
#include "rng.hpp"

namespace cpx {

constexpr size_t kRngG1CountMax = (size_t)1 << 20, kRngG1EachMax = (size_t)1 << 16, kRngG1TotalMax = (size_t)1 << 22;
constexpr size_t kRngG1ScratchMax = (size_t)512 << 20;   // candidate scratch of one chunk of streams
constexpr uint32_t RNG_G1_NONE = 0xffffffffu;            // a slot the round does not fill

// the scan's window: RNG_G1_WINDOW_BLOCKS blocks from the block that holds the first word of the next token
constexpr int RNG_G1_WINDOW_BLOCKS = 64;
constexpr int RNG_G1_WINDOW_WORDS = RNG_G1_WINDOW_BLOCKS * RNG_BLOCK_WORDS;
constexpr int RNG_G1_TOKEN_WORDS = RNG_FP_WORDS + 1;                                        // an accepted candidate and its bool
constexpr int RNG_G1_WINDOW_TOKENS = RNG_G1_WINDOW_WORDS / RNG_FP_WORDS;                     // no window holds more tokens than this

// ceil(sqrt(n))
CPX_HD uint32_t rng_g1_ceil_sqrt(uint32_t n) {
  uint32_t r = 0;
  while ((uint64_t)r * r < n) r++;
  return r;
}
// Candidates a stream emits in a round that still owes `need` points: 2 need + 8 ceil(sqrt(need)) + 16.  A candidate has a root with
// probability 1/2, so the hits are Binomial(cap, 1/2): mean cap / 2 = need + 4 ceil(sqrt(need)) + 8, standard deviation sqrt(cap) / 2.  The
// surplus over `need` is 4.7 deviations at need = 1 (26 candidates: 27 of 2^26 draws fall short) and more than 5 from need = 2 on — one
// round is the expected case; correctness never rests on it.  round_cap (option rng_g1_round_cap) > 0: at most that many.
CPX_HD uint32_t rng_g1_cap(uint32_t need, uint32_t round_cap) {
  const uint32_t dflt = 2 * need + 8 * rng_g1_ceil_sqrt(need) + 16;
  return round_cap && round_cap < dflt ? round_cap : dflt;
}

// one emitted candidate
struct RngG1Cand {
  uint32_t x[RNG_FP_WORDS];   // Montgomery limbs, below p
  uint32_t greatest;          // the bool behind it; k_rng_g1_sqrt adds RNG_G1_HIT where x^3 + 4 is a square
  uint32_t pad;
  uint64_t after;             // the stream's position behind the token
};
constexpr uint32_t RNG_G1_HIT = 2u;
// one stream of a chunk, between the rounds
struct RngG1Stream {
  uint64_t pos;        // where the next token starts
  uint64_t stop;       // where the round's scan stopped
  uint32_t done;       // points delivered so far
  uint32_t shortfall;  // points still owed
  uint32_t emitted;    // candidates of the round
  uint32_t pad;
};

struct RngG1Plan {
  size_t count, n_each, cap, chunk;   // chunk: streams per chunk, every chunk's candidate scratch within kRngG1ScratchMax
  static constexpr size_t cand_bytes() { return sizeof(RngG1Cand) + sizeof(Aff28); }
  RngG1Plan(size_t count_, size_t n_each_, long round_cap) : count(count_), n_each(n_each_) {
    cap = rng_g1_cap((uint32_t)n_each, round_cap > 0 ? (uint32_t)(round_cap > 0x7fffffffl ? 0x7fffffffl : round_cap) : 0u);
    chunk = kRngG1ScratchMax / (cap * cand_bytes());
    if (chunk < 1) chunk = 1;
    if (chunk > count) chunk = count;
  }
  static bool fits(size_t count, size_t n_each) {
    return count <= kRngG1CountMax && n_each <= kRngG1EachMax && (!count || !n_each || count * n_each <= kRngG1TotalMax);
  }
  size_t chunks() const { return (count + chunk - 1) / chunk; }
  size_t chunk_streams(size_t c) const { return c + 1 < chunks() ? chunk : count - c * chunk; }
};

}  // namespace cpx
