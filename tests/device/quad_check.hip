// TEST-ONLY: the quad-cooperative point formulas (g1_28_quad.hpp) and the work-group inversion (block_inverse.hpp) on raw limbs.
// Device only: DPP and barriers have no host twin.  tests/test_gpu_quad.py feeds it the rows of tests/quad_check_lib.py and checks the
// results against Python integers and the oracle; tests/test_quad_check_cpu.py pins the table, the rows and the checker without a GPU.
// Nothing in curdleproofs_amd/ links it.
//
// The command line, the record format, the exit codes and the runner are those of check_harness.hpp; --list prints name, input words
// per row, output words per row.  A record this program refuses (exit 3) is judged on the host before any HIP call: an unknown name,
// a wrong width, too many rows, inversion rows that are no multiple of the block size, a chain count outside 1..128, a ladder pattern
// above 16 bits, a same-slot flag other than 0 or 1.
//
// Quad operations: one QUAD per row, 64-thread work-groups of 16 rows; the host pads the last group with copies of row 0, so all 64
// lanes of every wave execute every quad call and every barrier (no lane returns early anywhere: DPP reads of disabled lanes are
// undefined, a skipped barrier hangs).  Sub-lane 0 stages the operands into LDS, a barrier follows — how the callers hold them — and
// every one of the four lanes writes its own copy of the result: an output row is 4 x the result words.
// Inversion operations: rows are lanes, every group of n rows is one work-group with 2 n values of LDS.
#define CHECK_PROG "quad_check"
#include <hip/hip_runtime.h>
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/g1_28_quad.hpp"
#include "../../curdleproofs_amd/csrc/block_inverse.hpp"

using namespace cpx;

// ---- limbs <-> values (rows are u32 words; F28 limbs travel as their two's complement bit patterns) ----
CPX_HD F28 ld28(const uint32_t* w) {
  F28 r;
  CPX_UNROLL for (int i = 0; i < 14; i++) r.v[i] = (int32_t)w[i];
  return r;
}
CPX_HD void st28(uint32_t* w, const F28& a) {
  CPX_UNROLL for (int i = 0; i < 14; i++) w[i] = (uint32_t)a.v[i];
}
CPX_HD Xyzz28 ldxyzz(const uint32_t* w) { return Xyzz28{ld28(w), ld28(w + 14), ld28(w + 28), ld28(w + 42)}; }
CPX_HD Jac28 ldjac(const uint32_t* w) { return Jac28{ld28(w), ld28(w + 14), ld28(w + 28)}; }
CPX_HD void stxyzz(uint32_t* w, const Xyzz28& p) {
  st28(w, p.x);
  st28(w + 14, p.y);
  st28(w + 28, p.zz);
  st28(w + 42, p.zzz);
}
CPX_HD void stjac(uint32_t* w, const Jac28& p) {
  st28(w, p.x);
  st28(w + 14, p.y);
  st28(w + 28, p.z);
}

// ---- quad operations: NI input words per row, NO result words per LANE; run() is called by all 64 lanes ----
// `buf` is the work-group's LDS, `base` the first of the quad's Q_SLOTS slots, `in` the quad's row, `out` the lane's own result
constexpr int Q_ACC = 0, Q_OTHER = 1, Q_IDENT = 2, Q_SLOTS = 3;

struct AddQuadCore {
  static constexpr int NI = 112, NO = 57;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    if (sub == 0) {
      buf[base + Q_ACC] = ldxyzz(in);
      buf[base + Q_OTHER] = ldxyzz(in + 56);
    }
    __syncthreads();
    Xyzz28 r;
    const int code = xyzz28_add_quad_core(buf[base + Q_ACC], buf[base + Q_OTHER], r);
    out[0] = (uint32_t)code;
    stxyzz(out + 1, r);
  }
};
struct AddQuadMem {   // word 112: 1 = both operands are the same slot (ia == ib), the second point is ignored
  static constexpr int NI = 113, NO = 56;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    if (sub == 0) {
      buf[base + Q_ACC] = ldxyzz(in);
      buf[base + Q_OTHER] = ldxyzz(in + 56);
    }
    __syncthreads();
    stxyzz(out, xyzz28_add_quad_mem(buf, base + Q_ACC, in[112] ? base + Q_ACC : base + Q_OTHER));
  }
};
struct DblQuad {
  static constexpr int NI = 56, NO = 56;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    if (sub == 0) buf[base + Q_ACC] = ldxyzz(in);
    __syncthreads();
    stxyzz(out, xyzz28_dbl_quad(buf[base + Q_ACC]));
  }
};
// the Jacobian point waits in an XYZZ slot (x, y, z in zz) and is doubled in registers, as k_table_build_quad holds it
static __device__ Jac28 staged_jac(const uint32_t* in, Xyzz28* buf, int base, int sub) {
  if (sub == 0) buf[base + Q_ACC] = Xyzz28{ld28(in), ld28(in + 14), ld28(in + 28), F28::zero()};
  __syncthreads();
  return Jac28{buf[base + Q_ACC].x, buf[base + Q_ACC].y, buf[base + Q_ACC].zz};
}
struct JacDblQuad {
  static constexpr int NI = 42, NO = 42;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    stjac(out, jac28_dbl_quad(staged_jac(in, buf, base, sub)));
  }
};
struct JacDblQuadChain {   // word 42: the number of doublings, 1..128
  static constexpr int NI = 43, NO = 42;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    Jac28 acc = staged_jac(in, buf, base, sub);
    const int count = (int)in[42];
    // the wave runs as many doublings as its longest row asks for; a quad that has finished runs along and keeps its result
    for (int s = 0; __any(s < count); s++) {
      const Jac28 next = jac28_dbl_quad(acc);
      if (s < count) acc = next;
    }
    stjac(out, acc);
  }
};
// double-and-add over the 16 bits of word 112 from bit 15 down, the accumulator in LDS as in k_smul_quad: all quads of the wave
// double, sub-lane 0 stores, barrier; then all add (the identity slot where the quad's bit is clear: the sum is then the accumulator
// itself, bit for bit), sub-lane 0 stores, barrier.  A step at which no quad of the wave adds skips the addition (uniform).
struct QuadLadder {
  static constexpr int NI = 113, NO = 56;
  static __device__ void run(const uint32_t* in, Xyzz28* buf, int base, int sub, uint32_t* out) {
    if (sub == 0) {
      buf[base + Q_ACC] = ldxyzz(in);
      buf[base + Q_OTHER] = ldxyzz(in + 56);
      buf[base + Q_IDENT] = Xyzz28::identity();
    }
    __syncthreads();
    const uint32_t pattern = in[112];
    for (int bit = 15; bit >= 0; bit--) {
      const Xyzz28 dbl = xyzz28_dbl_quad(buf[base + Q_ACC]);
      if (sub == 0) buf[base + Q_ACC] = dbl;
      __syncthreads();
      const bool add = (pattern >> bit) & 1u;
      if (!__any(add)) continue;
      const Xyzz28 sum = xyzz28_add_quad_mem(buf, base + Q_ACC, add ? base + Q_OTHER : base + Q_IDENT);
      if (sub == 0) buf[base + Q_ACC] = sum;
      __syncthreads();
    }
    stxyzz(out, buf[base + Q_ACC]);
  }
};

// one work-group = one wave = 16 rows; `in` and `out` hold a whole number of work-groups
template <class Op> __global__ __launch_bounds__(64) void k_quad(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ Xyzz28 buf[16 * Q_SLOTS];
  const int quad = threadIdx.x >> 2, sub = threadIdx.x & 3;
  const size_t row = (size_t)blockIdx.x * 16 + quad;
  Op::run(in + row * Op::NI, buf, quad * Q_SLOTS, sub, out + (row * 4 + sub) * Op::NO);
}
template <class Op> static bool run_quad(const uint32_t* in, uint32_t* out, uint64_t n) {
  if (n == 0) return true;
  const uint64_t padded = (n + 15) / 16 * 16;
  std::vector<uint32_t> hin((size_t)padded * Op::NI), hout((size_t)padded * 4 * Op::NO);
  memcpy(hin.data(), in, (size_t)n * Op::NI * sizeof(uint32_t));
  for (uint64_t r = n; r < padded; r++) memcpy(hin.data() + r * Op::NI, in, Op::NI * sizeof(uint32_t));   // copies of row 0
  uint32_t *din = nullptr, *dout = nullptr;
  HIPCHECK(hipMalloc(&din, hin.size() * sizeof(uint32_t)));
  HIPCHECK(hipMalloc(&dout, hout.size() * sizeof(uint32_t)));
  HIPCHECK(hipMemcpy(din, hin.data(), hin.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(dout, 0xa5, hout.size() * sizeof(uint32_t)));
  hipLaunchKernelGGL(k_quad<Op>, dim3((unsigned)(padded / 16)), dim3(64), 0, 0, din, dout);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(hout.data(), dout, hout.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(din));
  HIPCHECK(hipFree(dout));
  memcpy(out, hout.data(), (size_t)n * 4 * Op::NO * sizeof(uint32_t));   // the padding rows are dropped
  return true;
}

// ---- the work-group inversions: rows are lanes, N rows one work-group (64: what every caller launches; 256: the multi-wave
//      contract of the header, wave 0 inverts and the others wait at the barriers) ----
struct TableInverse {
  static constexpr int W = 14;
  typedef TF V;
  static __device__ void run(const uint32_t* in, V* buf, uint32_t* out) { st28(out, t_block_batch_inverse(ld28(in), buf)); }
};
struct StdInverse {
  static constexpr int W = 12;
  typedef Fp V;
  static __device__ void run(const uint32_t* in, V* buf, uint32_t* out) {
    Fp z;
    CPX_UNROLL for (int i = 0; i < 12; i++) z.v[i] = in[i];
    const Fp r = block_batch_inverse(z, buf);
    CPX_UNROLL for (int i = 0; i < 12; i++) out[i] = r.v[i];
  }
};
template <class Op, int N> __global__ __launch_bounds__(N) void k_inverse(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
  __shared__ typename Op::V buf[2 * N];
  const size_t row = (size_t)blockIdx.x * N + threadIdx.x;
  Op::run(in + row * Op::W, buf, out + row * Op::W);
}
template <class Op, int N> static bool run_inverse(const uint32_t* in, uint32_t* out, uint64_t n) {
  if (n == 0) return true;   // (n is a multiple of N: quad_payload() has seen to it)
  uint32_t *din = nullptr, *dout = nullptr;
  HIPCHECK(hipMalloc(&din, n * Op::W * sizeof(uint32_t)));
  HIPCHECK(hipMalloc(&dout, n * Op::W * sizeof(uint32_t)));
  HIPCHECK(hipMemcpy(din, in, n * Op::W * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIPCHECK(hipMemset(dout, 0xa5, n * Op::W * sizeof(uint32_t)));
  hipLaunchKernelGGL((k_inverse<Op, N>), dim3((unsigned)(n / N)), dim3(N), 0, 0, din, dout);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(out, dout, n * Op::W * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIPCHECK(hipFree(din));
  HIPCHECK(hipFree(dout));
  return true;
}

// ---- a plain row operation (check_harness.hpp: one thread per row) ----
struct XyzzFromJac {   // (not an OP(...): xyzz28_from_jac is a device function)
  static constexpr int NI = 42, NO = 56;
  static __device__ void run(const uint32_t* in, uint32_t* out) { stxyzz(out, xyzz28_from_jac(ldjac(in))); }
};

// the table: an Entry of the harness, the rows that make one work-group (0: any number) and, for a row whose last word is a
// parameter, the values it may take
struct QuadEntry {
  Entry e;
  uint32_t block, par_lo, par_hi;
  bool par;
};
template <class Op> static QuadEntry quad(const char* name, bool par = false, uint32_t lo = 0, uint32_t hi = 0) {
  return QuadEntry{Entry{name, Op::NI, 4 * Op::NO, run_quad<Op>}, 0, lo, hi, par};
}
template <class Op, int N> static QuadEntry inverse(const char* name) { return QuadEntry{Entry{name, Op::W, Op::W, run_inverse<Op, N>}, N, 0, 0, false}; }

static const QuadEntry TABLE[] = {
    quad<AddQuadCore>("xyzz28_add_quad_core"),
    quad<AddQuadMem>("xyzz28_add_quad_mem", true, 0, 1),
    quad<DblQuad>("xyzz28_dbl_quad"),
    quad<JacDblQuad>("jac28_dbl_quad"),
    quad<JacDblQuadChain>("jac28_dbl_quad/chain", true, 1, 128),
    quad<QuadLadder>("xyzz28_quad_ladder", true, 0, 0xffff),
    QuadEntry{entry<XyzzFromJac>("xyzz28_from_jac"), 0, 0, 0, false},
    inverse<TableInverse, 64>("t_block_batch_inverse/64"),
    inverse<TableInverse, 256>("t_block_batch_inverse/256"),
    inverse<StdInverse, 64>("block_batch_inverse/64"),
    inverse<StdInverse, 256>("block_batch_inverse/256"),
};

static const QuadEntry* find_op(const char* name) {
  const QuadEntry* op = nullptr;
  for (const QuadEntry& q : TABLE)
    if (!strcmp(q.e.name, name)) op = &q;
  return op;
}

int main(int argc, char** argv) {
  return check_main(
      argc, argv, true,
      [] {
        for (const QuadEntry& q : TABLE) printf("%s %d %d\n", q.e.name, q.e.ni, q.e.no);
      },
      [](const Header& h) -> int64_t {
        const QuadEntry* op = find_op(h.name);
        if (!op || h.words != (uint32_t)op->e.ni || h.rows > (1u << 20) || (op->block && h.rows % op->block)) return -1;
        return (int64_t)h.rows * op->e.ni;
      },
      [](Header& h, std::vector<uint32_t>& in, std::vector<uint32_t>& out, const CheckLoop&) -> int {
        const QuadEntry* op = find_op(h.name);   // (never null: the payload callback has accepted the name)
        if (op->par)
          for (uint64_t r = 0; r < h.rows; r++) {
            const uint32_t v = in[(size_t)(r + 1) * op->e.ni - 1];
            if (v < op->par_lo || v > op->par_hi) {
              fprintf(stderr, "quad_check: bad record '%s': row %llu carries the parameter %u, outside %u..%u\n", h.name, (unsigned long long)r, v, op->par_lo, op->par_hi);
              return CHECK_BAD;
            }
          }
        out.resize((size_t)h.rows * op->e.no);
        if (!op->e.run(in.data(), out.data(), h.rows)) return CHECK_FAILED;
        h.words = (uint32_t)op->e.no;
        return CHECK_OK;
      });
}
