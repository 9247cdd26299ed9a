// The Merlin transcript as a value that crosses the C ABI (include/cpx.h cpx_transcript_*, cpx_ipa_rounds, cpx_same_msm_rounds) — host
// code without a HIP call.  216 bytes = 27 little-endian u64: the 25 Keccak lanes, pos, pos_begin — the layout WaveStrobe::load / store
// (wave_strobe.hpp) read and write on the device and tests/strobe_ref.py::Strobe.from_words reads in the tests.  Merlin's cur_flags is not
// part of it: between whole Merlin messages it has no effect (every operation Merlin performs begins with `more = false`).
// The operations themselves are strobe.hpp's; this header only moves the value in and out and says which values are one.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "mont32.hpp"
#include "strobe.hpp"

namespace cpx {

constexpr size_t kTranscriptWords = 27, kTranscriptBytes = 8 * kTranscriptWords;

// pos indexes the state (run_f writes bytes pos and pos + 1 of the 200), pos_begin is pos + 1 of an earlier operation: a value outside
// these ranges was not written by a transcript and is refused before anything is launched or hashed
inline bool transcript_state_valid(const uint8_t* state) {
  uint64_t w[2];
  memcpy(w, state + 8 * 25, 16);
  return w[0] < Strobe::RATE && w[1] <= Strobe::RATE;
}
inline bool transcript_state_load(const uint8_t* state, Strobe& s) {
  if (!transcript_state_valid(state)) return false;
  uint64_t w[kTranscriptWords];
  memcpy(w, state, kTranscriptBytes);
  for (int i = 0; i < 25; i++) s.st[i] = w[i];
  s.pos = (uint32_t)w[25];
  s.pos_begin = (uint32_t)w[26];
  return true;
}
inline void transcript_state_store(const Strobe& s, uint8_t* state) {
  uint64_t w[kTranscriptWords];
  for (int i = 0; i < 25; i++) w[i] = s.st[i];
  w[25] = s.pos;
  w[26] = s.pos_begin;
  memcpy(state, w, kTranscriptBytes);
}

// a scalar as the ABI carries it (Montgomery residue, 4 x u64 little-endian) is a reduced one
inline bool fr_wire_reduced(const uint8_t wire[32]) {
  uint32_t w[8];
  memcpy(w, wire, 32);
  for (int i = 7; i >= 0; i--)
    if (w[i] != FrCfg::P[i]) return w[i] < FrCfg::P[i];
  return false;   // == r
}

}  // namespace cpx
