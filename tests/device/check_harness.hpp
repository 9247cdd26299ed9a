// TEST-ONLY: the runner shared by the check programs of tests/device/ (field_check, scalar_check, transcript_check, rng_check,
// rng_g1_check, msm_check, quad_check).  A program defines CHECK_PROG (its name, in every message), includes this header and calls check_main();
// a program whose operations all map one row of words to one row of words needs only OP(...) lines, a TABLE and rows_main().
// Nothing in curdleproofs_amd/ includes it.
//
//   <prog> IN OUT      runs every record of IN and writes one record per input record to OUT
//   <prog> --list      prints the program's operation table
//
// Record (little-endian): char name[48] (zero-padded) | u32 words per row | u32 reserved (0) | u64 rows | the payload, for a row
// operation rows x words x u32.  An input record carries the operation's input words per row, the output record its output words
// per row.  Exit codes: 0 every record ran; 2 usage or I/O (a file that cannot be opened or written); 3 a bad record (unknown name,
// wrong width, too many rows, truncated, trailing bytes after the last record, a case the program refuses); 4 a failed HIP call
// (device build); after 3 or 4 the output file is empty.  On success the program prints "<prog> (<host|device>): N records[, M rows]".
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/mont32.hpp"   // CPX_HD, CPX_UNROLL

#ifndef CHECK_PROG
#error "define CHECK_PROG (the program's name) before including check_harness.hpp"
#endif

struct Header {
  char name[48];
  uint32_t words, reserved;
  uint64_t rows;
};
static_assert(sizeof(Header) == 64, "record header layout");

enum Status { CHECK_OK = 0, CHECK_BAD = 3, CHECK_FAILED = 4 };

#if defined(__HIPCC__)
static const char* const BUILD = "device";
#define HIPCHECK(x)                                                                  \
  do {                                                                               \
    hipError_t e_ = (x);                                                             \
    if (e_ != hipSuccess) {                                                          \
      fprintf(stderr, CHECK_PROG ": %s: %s\n", #x, hipGetErrorString(e_));           \
      return false;                                                                  \
    }                                                                                \
  } while (0)
#else
static const char* const BUILD = "host";
#endif

// what run() may want to know about the loop: the input file behind the payload just read (transcript_check decodes its cases from
// it) and the number of records and rows finished so far
struct CheckLoop {
  FILE* in = nullptr;
  size_t records = 0, rows = 0;
};

// The record loop.  list(): prints the table.  payload(h): the u32 words that follow the header `h`, or -1 to refuse the record
// (the name, the width and the row count are judged here, before anything is allocated or read).  run(h, in, out, loop): runs one
// record on its payload `in`, fills `out` and sets h.words / h.rows to describe it; a status other than CHECK_OK ends the program
// with it (the callback has said why).  count_rows: the summary line carries the sum of the input rows.
template <class List, class Payload, class Run> static int check_main(int argc, char** argv, bool count_rows, List list, Payload payload, Run run) {
  if (argc == 2 && !strcmp(argv[1], "--list")) {
    list();
    return 0;
  }
  if (argc != 3) {
    fprintf(stderr, "usage: " CHECK_PROG " IN OUT | " CHECK_PROG " --list\n");
    return 2;
  }
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) {
    fprintf(stderr, CHECK_PROG ": cannot open %s\n", fi ? argv[2] : argv[1]);
    return 2;
  }
  CheckLoop loop;
  loop.in = fi;
  // a run that ends on a bad record or a failed HIP call leaves an empty output file: no record of it can pass for a result (no
  // caller reads the output of a failed run)
  auto refuse = [&](int status) {
    if (FILE* f = freopen(argv[2], "wb", fo)) fclose(f);
    return status;
  };
  Header h;
  size_t got;
  while ((got = fread(&h, 1, sizeof h, fi)) == sizeof h) {
    h.name[sizeof h.name - 1] = 0;
    const int64_t words = payload(h);
    if (words < 0) {
      fprintf(stderr, CHECK_PROG ": bad record '%s' (%u words per row, %llu rows)\n", h.name, h.words, (unsigned long long)h.rows);
      return refuse(CHECK_BAD);
    }
    std::vector<uint32_t> in((size_t)words), out;
    if (fread(in.data(), sizeof(uint32_t), in.size(), fi) != in.size()) {
      fprintf(stderr, CHECK_PROG ": record '%s' is truncated\n", h.name);
      return refuse(CHECK_BAD);
    }
    const uint64_t rows = h.rows;
    const int st = run(h, in, out, loop);
    if (st != CHECK_OK) return refuse(st);
    if (fwrite(&h, 1, sizeof h, fo) != sizeof h || fwrite(out.data(), sizeof(uint32_t), out.size(), fo) != out.size()) {
      fprintf(stderr, CHECK_PROG ": cannot write %s\n", argv[2]);
      return 2;
    }
    loop.records++;
    loop.rows += rows;
  }
  if (got != 0) {
    fprintf(stderr, CHECK_PROG ": trailing bytes after the last record\n");
    return refuse(CHECK_BAD);
  }
  if (fclose(fo) != 0) return 2;
  fclose(fi);
  if (count_rows)
    printf(CHECK_PROG " (%s): %zu records, %zu rows\n", BUILD, loop.records, loop.rows);
  else
    printf(CHECK_PROG " (%s): %zu records\n", BUILD, loop.records);
  return 0;
}

// ---- row operations: NI input words, NO output words, run() maps one row ----
// Every operation is a type of its own: the kernel template is instantiated once per operation and picked on the host, so each body
// is compiled on its own as it is inside the product's kernels.
#define OP(NAME, NI_, NO_, ...)                                       \
  struct NAME {                                                       \
    static constexpr int NI = NI_, NO = NO_;                          \
    static CPX_HD void run(const uint32_t* in, uint32_t* out) { __VA_ARGS__ } \
  };

// running one operation over n rows: the device build in a kernel of its own, one thread per row, 64-thread blocks, plain vector loads
// and stores into an output filled with 0xa5; the host build in a plain loop
#if defined(__HIPCC__)
template <class Op> __global__ __launch_bounds__(64) void k_rows(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
  const uint64_t row = (uint64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= n) return;
  uint32_t a[Op::NI], r[Op::NO];
  CPX_UNROLL for (int i = 0; i < Op::NI; i++) a[i] = in[row * Op::NI + i];
  Op::run(a, r);
  CPX_UNROLL for (int i = 0; i < Op::NO; i++) out[row * Op::NO + i] = r[i];
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
#else
template <class Op> static bool run_rows(const uint32_t* in, uint32_t* out, uint64_t n) {
  for (uint64_t i = 0; i < n; i++) Op::run(in + i * Op::NI, out + i * Op::NO);
  return true;
}
#endif

struct Entry {
  const char* name;
  int ni, no;
  bool (*run)(const uint32_t*, uint32_t*, uint64_t);
};
template <class Op> static Entry entry(const char* name) { return Entry{name, Op::NI, Op::NO, run_rows<Op>}; }

// the lister and the two callbacks of check_main over a table of row operations
template <size_t N> static const Entry* rows_find(const Entry (&table)[N], const char* name) {
  const Entry* op = nullptr;
  for (const Entry& e : table)
    if (!strcmp(e.name, name)) op = &e;
  return op;
}
template <size_t N> static void rows_list(const Entry (&table)[N]) {
  for (const Entry& e : table) printf("%s %d %d\n", e.name, e.ni, e.no);
}
template <size_t N> static int64_t rows_payload(const Entry (&table)[N], const Header& h) {
  const Entry* op = rows_find(table, h.name);
  if (!op || h.words != (uint32_t)op->ni || h.rows > (1u << 24)) return -1;
  return (int64_t)h.rows * op->ni;
}
template <size_t N> static int rows_run(const Entry (&table)[N], Header& h, std::vector<uint32_t>& in, std::vector<uint32_t>& out) {
  const Entry* op = rows_find(table, h.name);   // (never null: rows_payload() has accepted the name)
  out.resize((size_t)h.rows * op->no);
  if (!op->run(in.data(), out.data(), h.rows)) return CHECK_FAILED;
  h.words = (uint32_t)op->no;
  return CHECK_OK;
}
template <size_t N> static int rows_main(int argc, char** argv, const Entry (&table)[N]) {
  return check_main(
      argc, argv, true, [&] { rows_list(table); }, [&](const Header& h) { return rows_payload(table, h); },
      [&](Header& h, std::vector<uint32_t>& in, std::vector<uint32_t>& out, const CheckLoop&) { return rows_run(table, h, in, out); });
}
