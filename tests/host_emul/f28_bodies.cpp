// TEST-ONLY: the two bodies of the 28-bit-limb Montgomery product (fp28.hpp: schoolbook and Karatsuba) on raw limbs, so that
// tests/test_f28_karatsuba_cpu.py can drive operands the wire form cannot express (lazy differences, limbs at +-(2^28 - 1)).
// Nothing in curdleproofs_amd/ links or loads it.
#include <cstring>
#include "../../curdleproofs_amd/csrc/fp28.hpp"

using namespace cpx;

static F28 load(const int32_t* p) {
  F28 r;
  memcpy(r.v, p, sizeof r.v);
  return r;
}

extern "C" {

// in: n x 2 x 14 limbs (a, b); out: n x 14 limbs of a b / 2^392
void f28b_mul(int kara, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 a = load(in + 28 * i), b = load(in + 28 * i + 14);
    const F28 t = kara ? f28_mul_body<true>(a, b) : f28_mul_body<false>(a, b);
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
// the out-of-line entry the kernels call (f28_mul -> f28_mul_regs<KARA>)
void f28b_mul_regs(int kara, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 a = load(in + 28 * i), b = load(in + 28 * i + 14);
    const F28 t = kara ? f28_mul<true>(a, b) : f28_mul<false>(a, b);
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
// in: n x 4 x 14 limbs (a, b, c, d); out: n x 14 limbs of (a b - c d) / 2^392
void f28b_mulsub(int kara, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 a = load(in + 56 * i), b = load(in + 56 * i + 14), c = load(in + 56 * i + 28), d = load(in + 56 * i + 42);
    const F28 t = kara ? f28_mulsub_body<true>(a, b, c, d) : f28_mulsub_body<false>(a, b, c, d);
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
}
