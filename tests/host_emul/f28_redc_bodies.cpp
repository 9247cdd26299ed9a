// TEST-ONLY: every body of the 28-bit-limb Montgomery product and square (fp28.hpp) on raw limbs, so that
// tests/test_f28_redc_karatsuba_cpu.py can compare them bit for bit on operands the wire form cannot express.
// Body numbers: 0 = schoolbook, 1 = Karatsuba a b columns with the schoolbook reduction, 2 = Karatsuba a b columns and
// Karatsuba reduction; -1 = the build's default (f28_mul_body<>, f28_sqr_body<>, ...: CPX_F28_KARATSUBA, CPX_F28_REDC_KARATSUBA).
// Nothing in curdleproofs_amd/ links or loads it.
#include <cstring>
#include "../../curdleproofs_amd/csrc/fp28.hpp"

using namespace cpx;

static F28 load(const int32_t* p) {
  F28 r;
  memcpy(r.v, p, sizeof r.v);
  return r;
}
static F28 mul(int body, bool regs, const F28& a, const F28& b) {
  if (regs) {
    switch (body) {
      case 0: return f28_mul<false, false>(a, b);
      case 1: return f28_mul<true, false>(a, b);
      case 2: return f28_mul<true, true>(a, b);
      default: return f28_mul<>(a, b);
    }
  }
  switch (body) {
    case 0: return f28_mul_body<false, false>(a, b);
    case 1: return f28_mul_body<true, false>(a, b);
    case 2: return f28_mul_body<true, true>(a, b);
    default: return f28_mul_body<>(a, b);
  }
}
static F28 mulsub(int body, const F28& a, const F28& b, const F28& c, const F28& d) {
  switch (body) {
    case 0: return f28_mulsub_body<false, false>(a, b, c, d);
    case 1: return f28_mulsub_body<true, false>(a, b, c, d);
    case 2: return f28_mulsub_body<true, true>(a, b, c, d);
    default: return f28_mulsub_body<>(a, b, c, d);
  }
}
// squares: 0 = schoolbook square, 2 = Karatsuba square (symmetric blocks + Karatsuba reduction)
static F28 sqr(int body, bool regs, const F28& a) {
  if (regs) {
    switch (body) {
      case 0: return f28_sqr<false>(a);
      case 2: return f28_sqr<true>(a);
      default: return f28_sqr<>(a);
    }
  }
  switch (body) {
    case 0: return f28_sqr_body<false>(a);
    case 2: return f28_sqr_body<true>(a);
    default: return f28_sqr_body<>(a);
  }
}

extern "C" {

// the defaults this library was built with: bit 0 = F28_KARA, bit 1 = F28_REDC_KARA, bit 2 = F28_SQR_KARA
int f28r_defaults() { return (F28_KARA ? 1 : 0) | (F28_REDC_KARA ? 2 : 0) | (F28_SQR_KARA ? 4 : 0); }
// in: n x 2 x 14 limbs (a, b); out: n x 14 limbs of a b / 2^392 (regs != 0: the out-of-line entry the kernels call)
void f28r_mul(int body, int regs, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 t = mul(body, regs != 0, load(in + 28 * i), load(in + 28 * i + 14));
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
// in: n x 4 x 14 limbs (a, b, c, d); out: n x 14 limbs of (a b - c d) / 2^392
void f28r_mulsub(int body, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 t = mulsub(body, load(in + 56 * i), load(in + 56 * i + 14), load(in + 56 * i + 28), load(in + 56 * i + 42));
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
// in: n x 14 limbs; out: n x 14 limbs of a^2 / 2^392
void f28r_sqr(int body, int regs, const int32_t* in, int32_t* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    const F28 t = sqr(body, regs != 0, load(in + 14 * i));
    memcpy(out + 14 * i, t.v, sizeof t.v);
  }
}
}
