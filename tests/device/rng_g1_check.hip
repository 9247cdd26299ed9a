// TEST-ONLY: the pieces of G1::rand (curdleproofs_amd/csrc/rng.hpp: rng_fp_accept, rng_g1_candidate; g1_28.hpp: g1_28_point_from_x,
// g1_28_clear_cofactor) on raw words, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row, 64-thread blocks
// tests/test_rng_g1_check_cpu.py and tests/test_gpu_rng_g1.py feed both the same rows (tests/rng_g1_cases.py) and compare the results with
// each other and with the Python model (tests/stdrng_g1_ref.py).  Nothing in curdleproofs_amd/ links it.
//
//   rng_g1_check IN OUT      runs every record of IN and writes one record per input record to OUT
//   rng_g1_check --list      prints the operation table: name, input words per row, output words per row
//
// Record format, exit codes and the runner are those of rng_check.hip.  A state travels as ten words (key[8], word_pos low, high), a field
// element as its twelve standard-form limbs (Montgomery, R = 2^384, least significant first), the identity as x = y = 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/rng.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"

using namespace cpx;

#define OP(NAME, NI_, NO_, ...)                                       \
  struct NAME {                                                       \
    static constexpr int NI = NI_, NO = NO_;                          \
    static CPX_HD void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__ } \
  };

CPX_HD Fp fp_of(const uint32_t* w) {
  Fp a;
  for (int i = 0; i < 12; i++) a.v[i] = w[i];
  return a;
}
CPX_HD void fp_to(const Fp& a, uint32_t* w) {
  for (int i = 0; i < 12; i++) w[i] = a.v[i];
}

OP(FpAccept, 12, 13, uint32_t l[12]; for (int i = 0; i < 12; i++) l[i] = in[i]; out[12] = rng_fp_accept(l) ? 1u : 0u; for (int i = 0; i < 12; i++) out[i] = l[i];)
// state in; x, greatest, the position behind the token out
OP(G1Candidate, 10, 15, RngStream s(rng_state_from_words(in)); bool g; rng_g1_candidate(s, out, g); out[12] = g ? 1u : 0u; out[13] = (uint32_t)s.st.word_pos;
   out[14] = (uint32_t)(s.st.word_pos >> 32);)
// x (below p), greatest in; hit, x, y out (zero where there is no root)
OP(PointFromX, 13, 25, Aff28 p; const bool hit = g1_28_point_from_x(f28_from_std(fp_of(in)), in[12] != 0, &p); out[0] = hit ? 1u : 0u;
   for (int i = 1; i < 25; i++) out[i] = 0; if (hit) { fp_to(f28_to_std(p.x), out + 1); fp_to(f28_to_std(p.y), out + 13); })
// an affine point of E(Fp) in; affine([h] P) out
OP(ClearCofactor, 24, 24, Aff a; a.x = fp_of(in); a.y = fp_of(in + 12); const Jac28 q = g1_28_clear_cofactor(aff28_from_std(a));
   Aff r = Aff::identity(); if (!q.is_identity()) r = aff28_to_std(jac28_to_affine_with_zinv(q, f28_inv(q.z))); fp_to(r.x, out); fp_to(r.y, out + 12);)

// ---- running one operation over n rows ----
#if defined(__HIPCC__)
#define HIPCHECK(x)                                                                  \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      fprintf(stderr, "rng_g1_check: %s: %s\n", #x, hipGetErrorString(e_));          \
      return false;                                                                  \
    }                                                                                \
  } while (0)

template <class Op> __global__ __launch_bounds__(64) void k_rows(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
  const uint64_t row = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint32_t a[Op::NI], r[Op::NO];
  for (int i = 0; i < Op::NI; i++) a[i] = in[row * Op::NI + i];
  Op::run(a, r);
  for (int i = 0; i < Op::NO; i++) out[row * Op::NO + i] = r[i];
}
template <class Op> static bool run_rows(const uint32_t* in, uint32_t* out, uint64_t n) {
  if (n == 0) return true;
  uint32_t *din = nullptr, *dout = nullptr;
  HIPCHECK(hipMalloc(&din, n * Op::NI * sizeof(uint32_t)));
  HIPCHECK(hipMalloc(&dout, n * Op::NO * sizeof(uint32_t)));
  HIPCHECK(hipMemcpy(din, in, n * Op::NI * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(dout, 0xa5, n * Op::NO * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_rows<Op>, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, din, dout, n);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(out, dout, n * Op::NO * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(din));
  HIPCHECK(hipFree(dout));
  return true;
}
static const char* const BUILD = "device";
#else
template <class Op> static bool run_rows(const uint32_t* in, uint32_t* out, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) Op::run(in + i * Op::NI, out + i * Op::NO);
  return true;
}
static const char* const BUILD = "host";
#endif

struct Entry {
  const char* name;
  int ni, no;
  bool (*run)(const uint32_t*, uint32_t*, uint64_t);
};
template <class Op> static Entry entry(const char* name) { return Entry{name, Op::NI, Op::NO, run_rows<Op>}; }

static const Entry TABLE[] = {
    entry<FpAccept>("fp_accept"), entry<G1Candidate>("g1_candidate"), entry<PointFromX>("point_from_x"), entry<ClearCofactor>("clear_cofactor"),
};

struct Header {
  char name[48];
  uint32_t words, reserved;
  uint64_t rows;
};
static_assert(sizeof(Header) == 64, "record header layout");

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    for (const Entry& e : TABLE) printf("%s %d %d\n", e.name, e.ni, e.no);
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: rng_g1_check IN OUT | rng_g1_check --list\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) {
    fprintf(stderr, "rng_g1_check: cannot open %s\n", fi ? argv[2] : argv[1]);
    return 2;
  }
  Header h;
  size_t records = 0, rows = 0, got;
  while ((got = fread(&h, 1, sizeof h, fi)) == sizeof h) {
    h.name[sizeof h.name - 1] = 0;
    const Entry* op = nullptr;
    for (const Entry& e : TABLE)
      if (!strcmp(e.name, h.name)) op = &e;
    if (!op || h.words != (uint32_t)op->ni || h.rows > (1u << 24)) {
      fprintf(stderr, "rng_g1_check: bad record '%s' (%u words per row, %llu rows)\n", h.name, h.words, (unsigned long long)h.rows);
      return 3;
    }
    std::vector<uint32_t> in((size_t)h.rows * op->ni), out((size_t)h.rows * op->no);
    if (fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) {
      fprintf(stderr, "rng_g1_check: record '%s' is truncated\n", h.name);
      return 3;
    }
    if (!op->run(in.data(), out.data(), h.rows)) return 4;
    h.words = (uint32_t)op->no;
    if (fwrite(&h, 1, sizeof h, fo) != sizeof h || fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) {
      fprintf(stderr, "rng_g1_check: cannot write %s\n", argv[2]);
      return 2;
    }
    records++;
    rows += h.rows;
  }
  if (got != 0) {
    fprintf(stderr, "rng_g1_check: trailing bytes after the last record\n");
    return 3;
  }
  if (fclose(fo) != 0) return 2;
  fclose(fi);
  printf("rng_g1_check (%s): %zu records, %zu rows\n", BUILD, records, rows);
  return 0;
}
