// TEST-ONLY: every function of curdleproofs_amd/csrc/rng.hpp (the ChaCha12 block, the word stream, the samplers, the key expansion and the
// split) on raw words, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row, 64-thread blocks
// tests/test_rng_check_cpu.py and tests/test_gpu_rng.py feed both the same rows (tests/rng_cases.py) and compare the results with each other
// and with the Python model (tests/stdrng_ref.py).  Nothing in curdleproofs_amd/ links it.
//
//   rng_check IN OUT      runs every record of IN and writes one record per input record to OUT
//   rng_check --list      prints the operation table: name, input words per row, output words per row
//
// Record format, exit codes and the runner are those of scalar_check.hip.  A state travels as ten words: key[8], word_pos low, high.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/rng.hpp"

using namespace cpx;

#define OP(NAME, NI_, NO_, ...)                                       \
  struct NAME {                                                       \
    static constexpr int NI = NI_, NO = NO_;                          \
    static CPX_HD void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__ } \
  };

CPX_HD void st_pos(uint32_t* out, uint64_t pos) {
  out[0] = (uint32_t)pos;
  out[1] = (uint32_t)(pos >> 32);
}
constexpr int CHK_U32 = 40, CHK_U64 = 20, CHK_FR = 4, CHK_SHUFFLE = 40;

OP(Block, 10, 16, chacha12_block(in, (uint64_t)in[8] | ((uint64_t)in[9] << 32), out);)
OP(StreamU32, 10, CHK_U32 + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_U32; i++) out[i] = s.next_u32(); st_pos(out + CHK_U32, s.st.word_pos);)
OP(StreamU64, 10, 2 * CHK_U64 + 2, RngStream s(rng_state_from_words(in));
   for (int i = 0; i < CHK_U64; i++) { const uint64_t v = rng_next_u64(s); out[2 * i] = (uint32_t)v; out[2 * i + 1] = (uint32_t)(v >> 32); }
   st_pos(out + 2 * CHK_U64, s.st.word_pos);)
OP(FrRand, 10, 8 * CHK_FR + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_FR; i++) rng_fr(s, out + 8 * i); st_pos(out + 8 * CHK_FR, s.st.word_pos);)
OP(FrAccept, 8, 9, uint32_t l[8]; for (int i = 0; i < 8; i++) l[i] = in[i]; out[8] = rng_fr_accept(l) ? 1u : 0u; for (int i = 0; i < 8; i++) out[i] = l[i];)
OP(RangeAccept, 2, 3, uint32_t hi; out[0] = rng_range_zone(in[1]); out[2] = rng_range_accept(in[0], in[1], out[0], hi) ? 1u : 0u; out[1] = hi;)
OP(GenRange, 11, 3, RngStream s(rng_state_from_words(in)); out[0] = rng_gen_range(s, in[10]); st_pos(out + 1, s.st.word_pos);)
// a shuffle of 0..len, len <= CHK_SHUFFLE (longer: clamped); the unused tail stays the identity
OP(Shuffle, 11, CHK_SHUFFLE + 2, RngStream s(rng_state_from_words(in)); for (int i = 0; i < CHK_SHUFFLE; i++) out[i] = (uint32_t)i;
   rng_shuffle(s, out, in[10] < (uint32_t)CHK_SHUFFLE ? in[10] : (uint32_t)CHK_SHUFFLE); st_pos(out + CHK_SHUFFLE, s.st.word_pos);)
OP(SeedFromU64, 2, 10, rng_state_to_words(rng_seed_from_u64((uint64_t)in[0] | ((uint64_t)in[1] << 32)), out);)
OP(Split, 10, 12, RngStream s(rng_state_from_words(in)); rng_state_to_words(rng_split(s), out); st_pos(out + 10, s.st.word_pos);)
OP(PosValid, 2, 1, out[0] = rng_pos_valid((uint64_t)in[0] | ((uint64_t)in[1] << 32)) ? 1u : 0u;)

// ---- running one operation over n rows ----
#if defined(__HIPCC__)
#define HIPCHECK(x)                                                                  \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      fprintf(stderr, "rng_check: %s: %s\n", #x, hipGetErrorString(e_));             \
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
    entry<Block>("chacha12_block"), entry<StreamU32>("next_u32"), entry<StreamU64>("next_u64"), entry<FrRand>("fr_rand"), entry<FrAccept>("fr_accept"),
    entry<RangeAccept>("range_accept"), entry<GenRange>("gen_range"), entry<Shuffle>("shuffle"), entry<SeedFromU64>("seed_from_u64"), entry<Split>("split"),
    entry<PosValid>("pos_valid"),
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
    fprintf(stderr, "usage: rng_check IN OUT | rng_check --list\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) {
    fprintf(stderr, "rng_check: cannot open %s\n", fi ? argv[2] : argv[1]);
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
      fprintf(stderr, "rng_check: bad record '%s' (%u words per row, %llu rows)\n", h.name, h.words, (unsigned long long)h.rows);
      return 3;
    }
    std::vector<uint32_t> in((size_t)h.rows * op->ni), out((size_t)h.rows * op->no);
    if (fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) {
      fprintf(stderr, "rng_check: record '%s' is truncated\n", h.name);
      return 3;
    }
    if (!op->run(in.data(), out.data(), h.rows)) return 4;
    h.words = (uint32_t)op->no;
    if (fwrite(&h, 1, sizeof h, fo) != sizeof h || fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) {
      fprintf(stderr, "rng_check: cannot write %s\n", argv[2]);
      return 2;
    }
    records++;
    rows += h.rows;
  }
  if (got != 0) {
    fprintf(stderr, "rng_check: trailing bytes after the last record\n");
    return 3;
  }
  if (fclose(fo) != 0) return 2;
  fclose(fi);
  printf("rng_check (%s): %zu records, %zu rows\n", BUILD, records, rows);
  return 0;
}
