// TEST-ONLY: a script interpreter for the three transcript implementations (strobe.hpp, wave_strobe.hpp, lane_strobe.hpp) and row
// operations for the bit helpers of bit_interleave.hpp, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: engine strobe_host and the helpers
//   hipcc --offload-arch=gfx950 ...    -> the device program: every engine below, plain vector loads and stores
// tests/test_transcript_check_cpu.py and tests/test_gpu_transcript.py feed both the same cases and compare the results with each other
// and with tests/strobe_ref.py.  Nothing in curdleproofs_amd/ links it.
//
// The command line, the record header, the exit codes and the record loop are those of check_harness.hpp; --list prints name, input
// words per row, output words per row (0 0 for an engine).  After the header:
//   helper operation: rows x words x u32, a row operation of the harness
//   engine (words = 0): `rows` cases, each
//       u32 nops | u32 blob bytes | u32 message offset (0..15) | u32 reserved (0) | 27 x u64 start state (25 words, pos, pos_begin)
//       nops x { u32 code, a, b, c } | the blob, zero-padded to a multiple of 8 bytes
//     and in the output record, per case: u32 challenges | u32 reserved | 27 x u64 final state | challenges x { 4 x u64 scalar
//     (Montgomery form), u64 attempts }.
// Operations (offsets into the case's blob):
//   1 init            label at a, b bytes
//   2 meta_ad         data at a, b bytes, more = c
//   3 append_message  label at a, b bytes; the data follows the label, c bytes
//   4 append_begin    label at a, b bytes; total length c (the pieces follow as absorb operations)
//   5 absorb          data at a, b bytes
//   6 append_scalar   label at a, b bytes; the scalar (8 x u32, Montgomery form) at c
//   7 challenge_scalar label at a, b bytes; reports the scalar and the number of attempts
//   8 keccak          the permutation alone
//   9 round_trip      store the 27 words and load them back
// Engines:
//   wave         WaveStrobe, one 64-thread work-group per case as the product launches it, the blob read from global memory
//   wave_lds     the same with the blob copied to __shared__ memory first (protocol.hip absorbs from its scratch); wave_lds_sync() is the
//                only synchronisation
//   lane         LaneStrobe, 64 cases per work-group, the state in LDS at lds + threadIdx.x as in k_transcript_step1_lane
//   strobe_dev   cpx::Strobe compiled for the device, one thread per case
//   strobe_host  cpx::Strobe on the host (the only engine of the g++ build)
// The device engines place a case's blob at (16-byte boundary + message offset), so that LaneStrobe's aligned 8-byte read and its
// byte-wise path both run.  Exit code 0 only if every record was well formed (known name, offsets inside the blob, labels without NUL
// and shorter than 64 bytes, pos <= 165, pos_begin <= 166) and (device build) every HIP call succeeded.
#define CHECK_PROG "transcript_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/strobe.hpp"
#include "../../curdleproofs_amd/csrc/bit_interleave.hpp"
#if defined(__HIPCC__)
#include "../../curdleproofs_amd/csrc/wave_strobe.hpp"
#include "../../curdleproofs_amd/csrc/lane_strobe.hpp"
#endif

using namespace cpx;

enum : uint32_t { OP_INIT = 1, OP_META_AD, OP_APPEND_MESSAGE, OP_APPEND_BEGIN, OP_ABSORB, OP_APPEND_SCALAR, OP_CHALLENGE, OP_KECCAK, OP_ROUND_TRIP };
constexpr uint32_t MAX_LABEL = 63, MAX_BLOB = 1u << 16, MAX_OPS = 1u << 12, LDS_BLOB = 16384;

struct Op {
  uint32_t code, a, b, c;
};
struct Case {   // where one case's pieces lie in the flat arrays
  uint32_t op0, nops, blob0, chal0;
};

CPX_HD Fr ld_fr(const uint8_t* p) {
  Fr x;
  CPX_UNROLL for (int i = 0; i < 8; i++) x.v[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
  return x;
}
CPX_HD void st_chal(uint64_t* o, const Fr& canonical, uint64_t attempts) {
  const Fr m = fe_to_mont(canonical);
  CPX_UNROLL for (int j = 0; j < 4; j++) o[j] = (uint64_t)m.v[2 * j] | ((uint64_t)m.v[2 * j + 1] << 32);
  o[4] = attempts;
}

// ---- engines: the same nine operations on each implementation ----
// cpx::Strobe takes NUL-terminated labels: they are copied out of the blob
struct StrobeEngine {
  Strobe s;
  uint64_t tmp[27];
  struct Label {
    char s[MAX_LABEL + 1];
  };
  static CPX_HD Label label(const uint8_t* p, uint32_t n) {
    Label l;
    for (uint32_t i = 0; i < n; i++) l.s[i] = (char)p[i];
    l.s[n] = 0;
    return l;
  }
  CPX_HD void load(const uint64_t* st27) {
    for (int i = 0; i < 25; i++) s.st[i] = st27[i];
    s.pos = (uint32_t)st27[25];
    s.pos_begin = (uint32_t)st27[26];
  }
  CPX_HD void store(uint64_t* st27) {
    for (int i = 0; i < 25; i++) st27[i] = s.st[i];
    st27[25] = s.pos;
    st27[26] = s.pos_begin;
  }
  CPX_HD_FN void init(const uint8_t* l, uint32_t n) { s.init(label(l, n).s); }
  CPX_HD_FN void meta_ad(const uint8_t* d, uint32_t n, bool more) { s.meta_ad(d, n, more); }
  CPX_HD_FN void append_message(const uint8_t* l, uint32_t n, const uint8_t* d, uint32_t len) { s.append_message(label(l, n).s, d, len); }
  CPX_HD_FN void append_begin(const uint8_t* l, uint32_t n, uint32_t total) { s.append_begin(label(l, n).s, total); }
  CPX_HD_FN void absorb(const uint8_t* d, uint32_t n) { s.absorb(d, n); }
  CPX_HD_FN void append_scalar(const uint8_t* l, uint32_t n, const Fr& x_mont) {   // host::Transcript::append_scalar
    const Fr c = fe_from_mont(x_mont);
    uint8_t b[32];
    for (int j = 0; j < 32; j++) b[j] = (uint8_t)(c.v[j >> 2] >> (8 * (j & 3)));
    s.append_message(label(l, n).s, b, 32);
  }
  CPX_HD_FN void challenge(const uint8_t* l, uint32_t n, uint64_t* out) {
    const Label lb = label(l, n);
    Fr c;
    uint64_t attempts = 1;
    while (!s.challenge_attempt_canonical(lb.s, c.v)) attempts++;
    st_chal(out, c, attempts);
  }
  CPX_HD_FN void keccak() { keccak_f1600(s.st); }
  CPX_HD_FN void round_trip() {
    store(tmp);
    load(tmp);
  }
};

template <class E> CPX_HD void run_case(E& e, const Op* ops, uint32_t nops, const uint8_t* blob, uint64_t* chal) {
  for (uint32_t i = 0; i < nops; i++) {
    const Op o = ops[i];
    switch (o.code) {
      case OP_INIT: e.init(blob + o.a, o.b); break;
      case OP_META_AD: e.meta_ad(blob + o.a, o.b, o.c != 0); break;
      case OP_APPEND_MESSAGE: e.append_message(blob + o.a, o.b, blob + o.a + o.b, o.c); break;
      case OP_APPEND_BEGIN: e.append_begin(blob + o.a, o.b, o.c); break;
      case OP_ABSORB: e.absorb(blob + o.a, o.b); break;
      case OP_APPEND_SCALAR: e.append_scalar(blob + o.a, o.b, ld_fr(blob + o.c)); break;
      case OP_CHALLENGE:
        e.challenge(blob + o.a, o.b, chal);
        chal += 5;
        break;
      case OP_KECCAK: e.keccak(); break;
      case OP_ROUND_TRIP: e.round_trip(); break;
      default: break;   // (refused on the host before anything runs)
    }
  }
}

struct Batch {   // one engine record, flattened
  std::vector<Case> cases;
  std::vector<Op> ops;
  std::vector<uint8_t> blob;
  std::vector<uint64_t> st_in, st_out, chal;
};

static bool run_strobe_host(Batch& b) {
  for (size_t i = 0; i < b.cases.size(); i++) {
    const Case& c = b.cases[i];
    StrobeEngine e;
    e.load(&b.st_in[27 * i]);
    run_case(e, &b.ops[c.op0], c.nops, &b.blob[c.blob0], b.chal.data() + 5 * (size_t)c.chal0);
    e.store(&b.st_out[27 * i]);
  }
  return true;
}

#if defined(__HIPCC__)
struct WaveEngine {
  WaveStrobe t;
  uint8_t* scratch;   // 64 bytes of LDS, as the product's kernels pass
  uint64_t* rt;       // 27 words of LDS for the round trip
  int lane;
  __device__ void init(const uint8_t* l, uint32_t n) { t.init(reinterpret_cast<const char*>(l), n, scratch); }
  __device__ void meta_ad(const uint8_t* d, uint32_t n, bool more) { t.meta_ad(d, n, more); }
  __device__ void append_message(const uint8_t* l, uint32_t n, const uint8_t* d, uint32_t len) { t.append_message(reinterpret_cast<const char*>(l), n, d, len, scratch); }
  __device__ void append_begin(const uint8_t* l, uint32_t n, uint32_t total) { t.append_begin(reinterpret_cast<const char*>(l), n, total, scratch); }
  __device__ void absorb(const uint8_t* d, uint32_t n) { t.absorb(d, n); }
  __device__ void append_scalar(const uint8_t* l, uint32_t n, const Fr& x_mont) { t.append_scalar(reinterpret_cast<const char*>(l), n, x_mont, scratch); }
  __device__ void challenge(const uint8_t* l, uint32_t n, uint64_t* out) {
    Fr c;
    uint64_t attempts = 1;
    while (!t.challenge_attempt(reinterpret_cast<const char*>(l), n, scratch, c)) attempts++;
    if (lane == 0) st_chal(out, c, attempts);   // (uniform over the wave)
  }
  __device__ void keccak() { t.keccak(); }
  __device__ void round_trip() {
    t.store(rt);
    wave_lds_sync();
    t.load(rt, lane);
    wave_lds_sync();
  }
};

// one 64-thread work-group (one wave) per case; LDS_COPY: the blob is absorbed from __shared__ memory
template <bool LDS_COPY>
__global__ __launch_bounds__(64) void k_wave(const Case* __restrict__ cases, uint32_t ncases, const Op* __restrict__ ops, const uint8_t* __restrict__ blob,
                                             const uint32_t* __restrict__ blob_len, const uint64_t* __restrict__ st_in, uint64_t* __restrict__ st_out,
                                             uint64_t* __restrict__ chal) {
  __shared__ uint8_t scratch[64];
  __shared__ uint64_t rt[27];
  __shared__ uint8_t msg[LDS_COPY ? LDS_BLOB : 8];
  const uint32_t p = blockIdx.x;
  if (p >= ncases) return;
  const Case c = cases[p];
  const uint8_t* data = blob + c.blob0;
  if (LDS_COPY) {
    const uint32_t n = blob_len[p];   // <= LDS_BLOB (checked on the host)
    for (uint32_t i = threadIdx.x; i < n; i += 64) msg[i] = data[i];
    wave_lds_sync();
    data = msg;
  }
  WaveEngine e;
  e.scratch = scratch;
  e.rt = rt;
  e.lane = (int)threadIdx.x;
  e.t.load(st_in + 27 * (size_t)p, (int)threadIdx.x);
  run_case(e, ops + c.op0, c.nops, data, chal + 5 * (size_t)c.chal0);
  e.t.store(st_out + 27 * (size_t)p);
}

struct LaneEngine {
  LaneStrobe t;
  uint64_t tmp[27];
  __device__ void load(const uint64_t* st27) {
    for (int i = 0; i < 25; i++) t.w(i) = st27[i];
    t.pos = (uint32_t)st27[25];
    t.pos_begin = (uint32_t)st27[26];
  }
  __device__ void store(uint64_t* st27) {   // as k_transcript_step1_lane exports it
    for (int i = 0; i < 25; i++) st27[i] = t.w(i);
    st27[25] = t.pos;
    st27[26] = t.pos_begin;
  }
  __device__ void init(const uint8_t* l, uint32_t n) { t.init(reinterpret_cast<const char*>(l), n); }
  __device__ void meta_ad(const uint8_t* d, uint32_t n, bool more) { t.meta_ad(d, n, more); }
  __device__ void append_message(const uint8_t* l, uint32_t n, const uint8_t* d, uint32_t len) {
    t.append_begin(reinterpret_cast<const char*>(l), n, len);
    t.absorb(d, len);
  }
  __device__ void append_begin(const uint8_t* l, uint32_t n, uint32_t total) { t.append_begin(reinterpret_cast<const char*>(l), n, total); }
  __device__ void absorb(const uint8_t* d, uint32_t n) { t.absorb(d, n); }
  __device__ void append_scalar(const uint8_t* l, uint32_t n, const Fr& x_mont) {
    const Fr c = fe_from_mont(x_mont);
    uint8_t b[32];
    for (int j = 0; j < 32; j++) b[j] = (uint8_t)(c.v[j >> 2] >> (8 * (j & 3)));
    t.append_begin(reinterpret_cast<const char*>(l), n, 32);
    t.absorb(b, 32);
  }
  __device__ void challenge(const uint8_t* l, uint32_t n, uint64_t* out) {
    Fr c;
    uint64_t attempts = 1;
    while (!t.challenge_attempt(reinterpret_cast<const char*>(l), n, c)) attempts++;
    st_chal(out, c, attempts);
  }
  __device__ void keccak() {   // as LaneStrobe::run_f calls the permutation
    uint64_t a[25];
    CPX_UNROLL for (int i = 0; i < 25; i++) a[i] = t.st[64 * i];
    keccak_f1600(a);
    CPX_UNROLL for (int i = 0; i < 25; i++) t.st[64 * i] = a[i];
  }
  __device__ void round_trip() {
    store(tmp);
    load(tmp);
  }
};

// 64 cases per work-group, one lane each (no barrier: a lane only touches its own words)
__global__ __launch_bounds__(64) void k_lane(const Case* __restrict__ cases, uint32_t ncases, const Op* __restrict__ ops, const uint8_t* __restrict__ blob,
                                             const uint64_t* __restrict__ st_in, uint64_t* __restrict__ st_out, uint64_t* __restrict__ chal) {
  __shared__ uint64_t lds[25 * 64];
  const uint32_t p = blockIdx.x * 64 + threadIdx.x;
  if (p >= ncases) return;
  const Case c = cases[p];
  LaneEngine e;
  e.t.st = lds + threadIdx.x;
  e.load(st_in + 27 * (size_t)p);
  run_case(e, ops + c.op0, c.nops, blob + c.blob0, chal + 5 * (size_t)c.chal0);
  e.store(st_out + 27 * (size_t)p);
}

__global__ __launch_bounds__(64) void k_strobe(const Case* __restrict__ cases, uint32_t ncases, const Op* __restrict__ ops, const uint8_t* __restrict__ blob,
                                               const uint64_t* __restrict__ st_in, uint64_t* __restrict__ st_out, uint64_t* __restrict__ chal) {
  const uint32_t p = blockIdx.x * 64 + threadIdx.x;
  if (p >= ncases) return;
  const Case c = cases[p];
  StrobeEngine e;
  e.load(st_in + 27 * (size_t)p);
  run_case(e, ops + c.op0, c.nops, blob + c.blob0, chal + 5 * (size_t)c.chal0);
  e.store(st_out + 27 * (size_t)p);
}

template <class T> static bool upload(T** d, const std::vector<T>& h) {
  HIPCHECK(hipMalloc(d, (h.size() + 1) * sizeof(T)));
  if (!h.empty()) HIPCHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return true;
}
enum { ENG_WAVE, ENG_WAVE_LDS, ENG_LANE, ENG_STROBE_DEV };
static bool run_device(Batch& b, int engine, const std::vector<uint32_t>& blob_len) {
  const uint32_t n = (uint32_t)b.cases.size();
  if (n == 0) return true;
  Case* d_cases = nullptr;
  Op* d_ops = nullptr;
  uint8_t* d_blob = nullptr;
  uint32_t* d_len = nullptr;
  uint64_t *d_in = nullptr, *d_out = nullptr, *d_chal = nullptr;
  if (!upload(&d_cases, b.cases) || !upload(&d_ops, b.ops) || !upload(&d_blob, b.blob) || !upload(&d_len, blob_len) || !upload(&d_in, b.st_in)) return false;
  HIPCHECK(hipMalloc(&d_out, b.st_out.size() * sizeof(uint64_t)));
  HIPCHECK(hipMalloc(&d_chal, (b.chal.size() + 1) * sizeof(uint64_t)));
  HIPCHECK(hipMemset(d_out, 0xa5, b.st_out.size() * sizeof(uint64_t)));
  HIPCHECK(hipMemset(d_chal, 0xa5, (b.chal.size() + 1) * sizeof(uint64_t)));
  const dim3 per_case(n), per_lane((n + 63) / 64);
  switch (engine) {
    case ENG_WAVE: hipLaunchKernelGGL(k_wave<false>, per_case, dim3(64), 0, 0, d_cases, n, d_ops, d_blob, d_len, d_in, d_out, d_chal); break;
    case ENG_WAVE_LDS: hipLaunchKernelGGL(k_wave<true>, per_case, dim3(64), 0, 0, d_cases, n, d_ops, d_blob, d_len, d_in, d_out, d_chal); break;
    case ENG_LANE: hipLaunchKernelGGL(k_lane, per_lane, dim3(64), 0, 0, d_cases, n, d_ops, d_blob, d_in, d_out, d_chal); break;
    default: hipLaunchKernelGGL(k_strobe, per_lane, dim3(64), 0, 0, d_cases, n, d_ops, d_blob, d_in, d_out, d_chal); break;
  }
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(b.st_out.data(), d_out, b.st_out.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (!b.chal.empty()) HIPCHECK(hipMemcpy(b.chal.data(), d_chal, b.chal.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(d_cases));
  HIPCHECK(hipFree(d_ops));
  HIPCHECK(hipFree(d_blob));
  HIPCHECK(hipFree(d_len));
  HIPCHECK(hipFree(d_in));
  HIPCHECK(hipFree(d_out));
  HIPCHECK(hipFree(d_chal));
  return true;
}
#endif

// ---- the bit helpers as row operations ----
OP(Unshuffle32, 1, 1, out[0] = bits_unshuffle32(in[0]);)
OP(Shuffle32, 1, 1, out[0] = bits_shuffle32(in[0]);)
OP(Split64, 2, 2, bits_split64((uint64_t)in[0] | ((uint64_t)in[1] << 32), out[0], out[1]);)                       // (lo, hi) -> (even, odd)
OP(Join64, 2, 2, const uint64_t v = bits_join64(in[0], in[1]); out[0] = (uint32_t)v; out[1] = (uint32_t)(v >> 32);)   // (even, odd) -> (lo, hi)

struct Engine {
  const char* name;
  int id;   // -1 = strobe_host, else the device engine
};
static const Engine ENGINES[] = {
#if defined(__HIPCC__)
    {"wave", ENG_WAVE}, {"wave_lds", ENG_WAVE_LDS}, {"lane", ENG_LANE}, {"strobe_dev", ENG_STROBE_DEV},
#endif
    {"strobe_host", -1},
};
static const Entry TABLE[] = {
    entry<Unshuffle32>("bits_unshuffle32"),
    entry<Shuffle32>("bits_shuffle32"),
    entry<Split64>("bits_split64"),
    entry<Join64>("bits_join64"),
};

struct CaseHeader {
  uint32_t nops, blob_len, msg_offset, reserved;
};

static bool bad(const char* name, uint64_t i, const char* what) {
  fprintf(stderr, "transcript_check: bad record '%s', case %llu: %s\n", name, (unsigned long long)i, what);
  return false;
}

// reads the cases of one engine record into `b`, refusing everything a kernel could not run inside its buffers
static bool read_cases(FILE* fi, const Header& h, bool lds_copy, Batch& b, std::vector<uint32_t>& blob_len) {
  for (uint64_t i = 0; i < h.rows; i++) {
    CaseHeader ch;
    uint64_t st[27];
    if (fread(&ch, 1, sizeof ch, fi) != sizeof ch || fread(st, 1, sizeof st, fi) != sizeof st) return bad(h.name, i, "truncated");
    if (ch.nops > MAX_OPS || ch.blob_len > MAX_BLOB || ch.msg_offset > 15 || ch.reserved != 0) return bad(h.name, i, "case header out of range");
    if (lds_copy && ch.blob_len > LDS_BLOB) return bad(h.name, i, "blob larger than the LDS copy");
    if (st[25] > 165 || st[26] > 166) return bad(h.name, i, "pos / pos_begin outside the rate");
    Case c;
    c.op0 = (uint32_t)b.ops.size();
    c.nops = ch.nops;
    c.chal0 = (uint32_t)(b.chal.size() / 5);
    b.ops.resize(b.ops.size() + ch.nops);
    if (ch.nops && fread(&b.ops[c.op0], sizeof(Op), ch.nops, fi) != ch.nops) return bad(h.name, i, "truncated");
    const size_t start = ((b.blob.size() + 15) & ~(size_t)15) + ch.msg_offset, padded = ((size_t)ch.blob_len + 7) & ~(size_t)7;
    c.blob0 = (uint32_t)start;
    b.blob.resize(start + padded + 8, 0);   // (8 spare bytes: no read of a whole word ends outside the buffer)
    if (padded && fread(&b.blob[start], 1, padded, fi) != padded) return bad(h.name, i, "truncated");
    const uint8_t* blob = &b.blob[start];
    auto inside = [&](uint64_t off, uint64_t n) { return off + n <= ch.blob_len; };
    auto label_ok = [&](const Op& o) { return o.b <= MAX_LABEL && inside(o.a, o.b) && !memchr(blob + o.a, 0, o.b); };
    for (uint32_t k = 0; k < ch.nops; k++) {
      const Op& o = b.ops[c.op0 + k];
      bool ok = false;
      switch (o.code) {
        case OP_INIT: ok = label_ok(o); break;
        case OP_META_AD: ok = inside(o.a, o.b) && o.c <= 1; break;
        case OP_APPEND_MESSAGE: ok = label_ok(o) && inside((uint64_t)o.a + o.b, o.c); break;
        case OP_APPEND_BEGIN: ok = label_ok(o); break;
        case OP_ABSORB: ok = inside(o.a, o.b); break;
        case OP_APPEND_SCALAR: ok = label_ok(o) && inside(o.c, 32); break;
        case OP_CHALLENGE:
          ok = label_ok(o);
          b.chal.resize(b.chal.size() + 5, 0);
          break;
        case OP_KECCAK:
        case OP_ROUND_TRIP: ok = true; break;
        default: break;
      }
      if (!ok) return bad(h.name, i, "operation out of range");
    }
    b.cases.push_back(c);
    blob_len.push_back(ch.blob_len);
    b.st_in.insert(b.st_in.end(), st, st + 27);
  }
  b.st_out.assign(b.st_in.size(), 0);
  return true;
}

static const Engine* find_engine(const char* name) {
  for (const Engine& e : ENGINES)
    if (!strcmp(e.name, name)) return &e;
  return nullptr;
}

// one engine record: the cases are decoded from the input file behind the header, the output is the record's payload as u32 words
static int run_engine(const Engine& eng, const Header& h, FILE* fi, std::vector<uint32_t>& out) {
  Batch b;
  std::vector<uint32_t> blob_len;
#if defined(__HIPCC__)
  if (!read_cases(fi, h, eng.id == ENG_WAVE_LDS, b, blob_len)) return CHECK_BAD;
  if (!(eng.id < 0 ? run_strobe_host(b) : run_device(b, eng.id, blob_len))) return CHECK_FAILED;
#else
  if (!read_cases(fi, h, false, b, blob_len)) return CHECK_BAD;
  if (!run_strobe_host(b)) return CHECK_FAILED;
#endif
  auto put64 = [&](const uint64_t* p, size_t n) {
    for (size_t i = 0; i < n; i++) {
      out.push_back((uint32_t)p[i]);
      out.push_back((uint32_t)(p[i] >> 32));
    }
  };
  for (size_t i = 0; i < b.cases.size(); i++) {
    const Case& c = b.cases[i];
    const uint32_t nchal = (i + 1 < b.cases.size() ? b.cases[i + 1].chal0 : (uint32_t)(b.chal.size() / 5)) - c.chal0;
    out.push_back(nchal);
    out.push_back(0);
    put64(&b.st_out[27 * i], 27);
    if (nchal) put64(&b.chal[5 * (size_t)c.chal0], 5 * (size_t)nchal);
  }
  return CHECK_OK;
}

int main(int argc, char** argv) {
  return check_main(
      argc, argv, true,
      [] {
        for (const Engine& e : ENGINES) printf("%s 0 0\n", e.name);
        rows_list(TABLE);
      },
      [](const Header& h) -> int64_t {
        if (h.reserved != 0) return -1;
        if (find_engine(h.name)) return h.words == 0 && h.rows <= (1u << 24) ? 0 : -1;
        return rows_payload(TABLE, h);
      },
      [](Header& h, std::vector<uint32_t>& in, std::vector<uint32_t>& out, const CheckLoop& loop) {
        const Engine* eng = find_engine(h.name);
        return eng ? run_engine(*eng, h, loop.in, out) : rows_run(TABLE, h, in, out);
      });
}
