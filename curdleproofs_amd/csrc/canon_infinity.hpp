// Encodings with the infinity flag set (include/cpx.h, option strict_infinity) — host code without a HIP call and without an Engine; one
// definition for Engine::canonical_infinities (engine.cpp) and tests/host_emul/canon_infinity_emul.cpp, which compiles it for the CPU
// (tests/test_canon_infinity_cpu.py).
//
// ark-bls12-381 ^0.4's `read_g1_compressed` — the deserialiser behind `G1Affine::deserialize_compressed`, whisk.rs:313-320 — returns the
// identity as soon as the compression and the infinity flag are set, without looking at the sort flag or the other bits (recalled from the
// 0.4.0 source; 0.5 added both checks), and the verifier then hashes the point's CANONICAL serialisation (transcript.rs:28-36 append the
// deserialised points).  The device kernels accept exactly the canonical form, so with strict_infinity = 0 the host rewrites a non-canonical
// infinity encoding to 0xc0 || 0^47 in a copy of the input before anything reads it; with strict_infinity = 1 the bytes go through
// untouched and such an encoding is a deserialisation error.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace cpx {

inline bool infinity_is_noncanonical(const uint8_t* enc) {
  if ((enc[0] & 0xc0) != 0xc0) return false;
  if (enc[0] != 0xc0) return true;
  for (int i = 1; i < 48; i++)
    if (enc[i]) return true;
  return false;
}

// `bytes` (nbytes of them: nrec records of `stride` bytes) with every non-canonical infinity encoding at `offsets` of each record rewritten
// to the canonical one.  Nothing to rewrite: returns `bytes` itself and leaves `store` alone.  Otherwise `store` becomes the rewritten copy
// and its data() is returned: the caller owns it, so it lives as long as the caller needs the result (above its CallScope, engine.hpp).
inline const uint8_t* canonical_infinities(const uint8_t* bytes, size_t nbytes, size_t nrec, size_t stride, const std::vector<size_t>& offsets,
                                           std::vector<uint8_t>& store) {
  bool copied = false;
  for (size_t r = 0; r < nrec; r++)
    for (size_t off : offsets) {
      const size_t at = r * stride + off;
      if (!(bytes[at] & 0x40) || !infinity_is_noncanonical(bytes + at)) continue;   // (one byte per encoding on the common path)
      if (!copied) {
        store.assign(bytes, bytes + nbytes);
        bytes = store.data();
        copied = true;
      }
      store[at] = 0xc0;
      memset(&store[at + 1], 0, 47);
    }
  return bytes;
}

}  // namespace cpx
