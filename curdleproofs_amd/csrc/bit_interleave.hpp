// Even / odd bit interleaving of 32- and 64-bit words — product code shared by host and device: the form wave_strobe.hpp keeps the
// Keccak state in (the even bits of a 64-bit word in one lane, its odd bits in another).  Plain C++, no HIP dependency:
// tests/device/transcript_check.hip runs these through g++ and on the device.
#pragma once
#include <cstdint>
#include "mont32.hpp"

namespace cpx {

// perfect outer un-shuffle of 32 bits: even bits -> low 16, odd bits -> high 16 (Hacker's Delight 7-2), and its inverse
CPX_HD uint32_t bits_unshuffle32(uint32_t x) {
  uint32_t t;
  t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
  t = (x ^ (x >> 2)) & 0x0c0c0c0cu; x ^= t ^ (t << 2);
  t = (x ^ (x >> 4)) & 0x00f000f0u; x ^= t ^ (t << 4);
  t = (x ^ (x >> 8)) & 0x0000ff00u; x ^= t ^ (t << 8);
  return x;
}
CPX_HD uint32_t bits_shuffle32(uint32_t x) {
  uint32_t t;
  t = (x ^ (x >> 8)) & 0x0000ff00u; x ^= t ^ (t << 8);
  t = (x ^ (x >> 4)) & 0x00f000f0u; x ^= t ^ (t << 4);
  t = (x ^ (x >> 2)) & 0x0c0c0c0cu; x ^= t ^ (t << 2);
  t = (x ^ (x >> 1)) & 0x22222222u; x ^= t ^ (t << 1);
  return x;
}
// 64-bit word <-> (even bits, odd bits)
CPX_HD void bits_split64(uint64_t v, uint32_t& even, uint32_t& odd) {
  const uint32_t lo = bits_unshuffle32((uint32_t)v), hi = bits_unshuffle32((uint32_t)(v >> 32));
  even = (lo & 0xffffu) | (hi << 16);
  odd = (lo >> 16) | (hi & 0xffff0000u);
}
CPX_HD uint64_t bits_join64(uint32_t even, uint32_t odd) {
  const uint32_t lo = bits_shuffle32((even & 0xffffu) | (odd << 16)), hi = bits_shuffle32((even >> 16) | (odd & 0xffff0000u));
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace cpx
