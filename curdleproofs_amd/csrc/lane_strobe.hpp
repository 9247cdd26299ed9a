// One-lane STROBE-128 for the device side of the transcripts — product code (device only).
//
// ONE lane per transcript running the plain 64-bit Keccak of strobe.hpp (k_transcript_step1_lane: large batches, where the prefix hides
// behind the table build / the decompression and instructions count, not latency).  The sponge state lives in LDS, word-interleaved by
// lane (word i of lane l at [i * 64 + l]: dynamic word indices without scratch memory, no bank conflicts).  Same semantics as strobe.hpp
// (the host's code) and wave_strobe.hpp; tests/device/transcript_check.hip runs all three at every position of the rate.
#pragma once
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "strobe.hpp"

namespace cpx {

struct LaneStrobe {
  uint64_t* st;   // &lds[lane]; word i at st[64 * i]
  uint32_t pos, pos_begin;
  __device__ __forceinline__ uint64_t& w(uint32_t i) { return st[64 * i]; }
  __device__ __forceinline__ void xor_byte(uint32_t i, uint8_t b) { w(i >> 3) ^= (uint64_t)b << (8 * (i & 7)); }
  __device__ void run_f() {
    xor_byte(pos, (uint8_t)pos_begin);
    xor_byte(pos + 1, 0x04);
    xor_byte(Strobe::RATE + 1, 0x80);
    uint64_t a[25];
    CPX_UNROLL for (int i = 0; i < 25; i++) a[i] = st[64 * i];
    keccak_f1600(a);
    CPX_UNROLL for (int i = 0; i < 25; i++) st[64 * i] = a[i];
    pos = pos_begin = 0;
  }
  __device__ void absorb(const uint8_t* d, size_t n) {
    size_t i = 0;
    while (i < n) {
      if ((pos & 7) == 0 && n - i >= 8 && pos + 8 <= Strobe::RATE) {
        uint64_t v;
        if ((reinterpret_cast<uintptr_t>(d + i) & 7) == 0) v = *reinterpret_cast<const uint64_t*>(d + i);
        else {
          v = 0;
          for (int j = 0; j < 8; j++) v |= (uint64_t)d[i + j] << (8 * j);
        }
        w(pos >> 3) ^= v;
        pos += 8;
        i += 8;
        continue;
      }
      xor_byte(pos, d[i++]);
      if (++pos == Strobe::RATE) run_f();
    }
  }
  __device__ void begin_op(uint32_t flags, bool more) {
    if (more) return;
    const uint8_t hdr[2] = {(uint8_t)pos_begin, (uint8_t)flags};
    pos_begin = pos + 1;
    absorb(hdr, 2);
    if ((flags & (Strobe::FLAG_C | Strobe::FLAG_K)) && pos != 0) run_f();
  }
  __device__ void meta_ad(const void* d, size_t n, bool more) {
    begin_op(Strobe::FLAG_M | Strobe::FLAG_A, more);
    absorb(static_cast<const uint8_t*>(d), n);
  }
  __device__ void append_begin(const char* label, size_t label_len, size_t len) {
    const uint8_t l4[4] = {(uint8_t)len, (uint8_t)(len >> 8), (uint8_t)(len >> 16), (uint8_t)(len >> 24)};
    meta_ad(label, label_len, false);
    meta_ad(l4, 4, true);
    begin_op(Strobe::FLAG_A, false);
  }
  __device__ void init(const char* label, size_t label_len) {
    for (int i = 0; i < 25; i++) st[64 * i] = 0;
    const uint8_t ini[18] = {1, 168, 1, 0, 1, 96, 'S', 'T', 'R', 'O', 'B', 'E', 'v', '1', '.', '0', '.', '2'};
    for (int i = 0; i < 18; i++) xor_byte(i, ini[i]);
    pos = pos_begin = 0;
    {
      uint64_t a[25];
      CPX_UNROLL for (int i = 0; i < 25; i++) a[i] = st[64 * i];
      keccak_f1600(a);
      CPX_UNROLL for (int i = 0; i < 25; i++) st[64 * i] = a[i];
    }
    meta_ad("Merlin v1.0", 11, false);
    append_begin("dom-sep", 7, label_len);
    absorb(reinterpret_cast<const uint8_t*>(label), label_len);
  }
  // One attempt of get_and_append_challenge (transcript.rs:40-60), as WaveStrobe::challenge_attempt: 64 PRF bytes, the first 32 with the
  // top bit cleared; when canonical and non-zero the scalar is appended back under the same label and returned in canonical form,
  // otherwise the caller retries.
  __device__ bool challenge_attempt(const char* label, size_t label_len, Fr& c) {
    const uint8_t l4[4] = {64, 0, 0, 0};
    meta_ad(label, label_len, false);
    meta_ad(l4, 4, true);
    begin_op(Strobe::FLAG_I | Strobe::FLAG_A | Strobe::FLAG_C, false);   // forces a permutation: pos = 0 afterwards
    uint64_t sq[4];
    CPX_UNROLL for (int j = 0; j < 4; j++) sq[j] = w(j);
    CPX_UNROLL for (int j = 0; j < 8; j++) w(j) = 0;   // the PRF operation overwrites the 64 squeezed bytes with zero
    pos = 64;
    sq[3] &= 0x7fffffffffffffffULL;
    CPX_UNROLL for (int j = 0; j < 4; j++) {
      c.v[2 * j] = (uint32_t)sq[j];
      c.v[2 * j + 1] = (uint32_t)(sq[j] >> 32);
    }
    bool nz = false, lt = false;
    for (int j = 0; j < 8; j++) nz |= c.v[j] != 0;
    for (int j = 7; j >= 0; j--) {
      if (c.v[j] != FrCfg::P[j]) {
        lt = c.v[j] < FrCfg::P[j];
        break;
      }
    }
    if (!(lt && nz)) return false;
    append_begin(label, label_len, 32);
    uint8_t b32[32];
    CPX_UNROLL for (int j = 0; j < 32; j++) b32[j] = (uint8_t)(sq[j >> 3] >> (8 * (j & 7)));
    absorb(b32, 32);
    return true;
  }
};

}  // namespace cpx
