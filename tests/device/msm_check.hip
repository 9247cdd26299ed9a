// TEST-ONLY: the MSM wave bodies of curdleproofs_amd/csrc/msm_body.hpp and the library's set reducers, bucket by bucket.  A device
// program without a host twin (the bodies use wave shuffles, LDS atomics and barriers): the reference is the Python model of
// tests/msm_check_lib.py plus the oracle.  The bodies are wrapped in kernels of this file with the library's launch bounds and dynamic
// LDS sizes; the reducers, the finalisation and the Horner tail are the library's own (libcpx.so, kernels.h), on crafted inputs.
//
// The command line, the exit codes and the record loop are those of check_harness.hpp; --list prints name, group.
//
// Record (little-endian): char name[48] (zero-padded) | u32 1 | u32 reserved (0) | u64 words | words x u32 — the record format of
// check_harness.hpp with one word per row; the payload of every operation is described beside its runner.  Points enter as standard-form
// words (Aff: 24, Jac: 36) and are converted on the host (t_from_std); raw-set entries leave as standard-form Jacobian points
// (t_acc_to_jac, t_jac_to_std) followed by a flag word (bit 0: the raw entry is the identity, bit 1: it still holds the poison).
// A "pool" record holds the points the later records of the file name by index; a reference is a pool index, bit 31 set for the
// negated point, ~0u for the identity.
// Every HIP call is checked: on an error the program stops with a nonzero status and starts no further kernel.  Every index of a case
// is checked against the size of what it addresses before anything is launched (exit 3).
#include <string>
#define CHECK_PROG "msm_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/msm_body.hpp"

using namespace cpx;

#define REQUIRE(c)                                                           \
  do {                                                                       \
    if (!(c)) {                                                              \
      fprintf(stderr, "msm_check: bad case: %s (line %d)\n", #c, __LINE__);  \
      g_bad_case = true;                                                     \
      return false;                                                          \
    }                                                                        \
  } while (0)

static bool g_bad_case = false;
static constexpr uint32_t POISON = 0xa5a5a5a5u;
static constexpr uint32_t MAX_WORDS = 1u << 27;

// ---- kernels: the bodies with the library's launch bounds ----
template <int WPW, bool PERWIN> __global__ __launch_bounds__(64, 2) void k_tblw(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot,
                                                                                int slices) {
  msm_tblw_body<WPW, PERWIN>(tasks, raw, raw_slot, slices, blockIdx.x);
}
template <int WPW> __global__ __launch_bounds__(64, 2) void k_tblw2(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot, int slices) {
  msm_tblw_body<WPW, false, false, 2>(tasks, raw, raw_slot, slices, blockIdx.x);
}
__global__ __launch_bounds__(64, 2) void k_pair(const TblTask* __restrict__ tasks, uint32_t* __restrict__ raw, uint32_t* __restrict__ raw_slot) {
  msm_tblw_body<2, true, true>(tasks, raw, raw_slot, 1, blockIdx.x);
}
template <int CB, int FIX_WPW> __global__ __launch_bounds__(64, 2) void k_fix(const FixTask* __restrict__ tasks, const TFix* __restrict__ tab, int nc, uint32_t* __restrict__ raw,
                                                                              uint32_t* __restrict__ raw_slot) {
  msm_fix_body<CB, FIX_WPW>(tasks, tab, nc, raw, raw_slot, blockIdx.x);
}

// tbw_sort round by round, exactly as msm_tblw_body calls it (CACHE = WPW == 2 && !PERWIN); wave = blockIdx.x.  After every round the
// wave copies end, cnt[], cur[], order[], the number of entries and the list to its record [wave][round] of `out`.
template <int NBINS> constexpr uint32_t sort_rec_words() { return 2 + 3 * NBINS + TBW_CAP; }
template <int WPW, bool PERWIN, int NBINS> __global__ __launch_bounds__(64, 2) void k_sort(const TblTask* __restrict__ tasks, uint32_t first, uint32_t ntot,
                                                                                          uint32_t* __restrict__ out, uint32_t maxrounds) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const TbwSort<NBINS> ts(smem);
  const TblTask task = tasks[0];
  const int wv = blockIdx.x, w0 = PERWIN ? wv : wv * WPW, lane = threadIdx.x;
  constexpr uint32_t REC = sort_rec_words<NBINS>();
  uint32_t* mine = out + (size_t)wv * (1 + (size_t)maxrounds * REC);
  uint32_t next = first, rounds = 0;
  do {
    if (rounds >= maxrounds) break;   // (never with a sort that advances: the host sized the buffer by one slab per round)
    const uint32_t end = tbw_sort<WPW, PERWIN, NBINS, WPW == 2 && !PERWIN>(ts, task, w0, next, ntot);
    uint32_t* rec = mine + 1 + (size_t)rounds * REC;
    uint32_t total = 0;
    for (int b = 0; b < NBINS; b++) total += ts.cnt[b];
    if (total > (uint32_t)TBW_CAP) total = TBW_CAP;
    if (lane == 0) {
      rec[0] = end;
      rec[1] = total;
    }
    for (int b = lane; b < NBINS; b += 64) {
      rec[2 + b] = ts.cnt[b];
      rec[2 + NBINS + b] = ts.cur[b];
      rec[2 + 2 * NBINS + b] = ts.order[b];
    }
    for (uint32_t i = lane; i < total; i += 64) rec[2 + 3 * NBINS + i] = ts.list[i];
    __syncthreads();
    rounds++;
    if (end <= next && next < ntot) break;   // a sort that does not advance
    next = end;
  } while (next < ntot);
  if (lane == 0) mine[0] = rounds;
}

// ---- case reader ----
struct Reader {
  const uint32_t* p;
  size_t n, o = 0;
  bool ok = true;
  uint32_t u() {
    if (o >= n) {
      ok = false;
      return 0;
    }
    return p[o++];
  }
  const uint32_t* take(size_t k) {
    if (k > n - o) {
      ok = false;
      return nullptr;
    }
    const uint32_t* r = p + o;
    o += k;
    return r;
  }
};

static std::vector<Aff> g_pool;   // standard form
static bool ref_point(uint32_t ref, TAff& out) {
  if (ref == ~0u) {
    out = TAff::identity();
    return true;
  }
  const uint32_t i = ref & 0x7fffffffu;
  if (i >= g_pool.size()) return false;
  out = t_from_std((ref >> 31) ? aff_neg(g_pool[i]) : g_pool[i]);
  return true;
}
static Aff ld_aff(const uint32_t* w) {
  Aff a;
  for (int i = 0; i < 12; i++) {
    a.x.v[i] = w[i];
    a.y.v[i] = w[12 + i];
  }
  return a;
}
static Jac ld_jac(const uint32_t* w) {
  Jac a;
  for (int i = 0; i < 12; i++) {
    a.x.v[i] = w[i];
    a.y.v[i] = w[12 + i];
    a.z.v[i] = w[24 + i];
  }
  return a;
}
static void st_jac(std::vector<uint32_t>& out, const Jac& a) {
  for (int i = 0; i < 12; i++) out.push_back(a.x.v[i]);
  for (int i = 0; i < 12; i++) out.push_back(a.y.v[i]);
  for (int i = 0; i < 12; i++) out.push_back(a.z.v[i]);
}
// one raw-set entry: 36 words of the standard-form Jacobian point and the flag word
static void st_acc(std::vector<uint32_t>& out, const uint32_t* words) {
  bool poison = true;
  for (int i = 0; i < ACC_WORDS; i++) poison = poison && words[i] == POISON;
  TAcc a;
  memcpy(&a, words, sizeof a);
  if (poison) {
    for (int i = 0; i < 36; i++) out.push_back(0);
    out.push_back(2u);
    return;
  }
  st_jac(out, t_jac_to_std(t_acc_to_jac(a)));
  out.push_back(a.is_identity() ? 1u : 0u);
}
static uint32_t count_not_poison(const uint32_t* w, size_t n) {
  uint32_t c = 0;
  for (size_t i = 0; i < n; i++) c += w[i] != POISON ? 1u : 0u;
  return c;
}
template <class T> static bool dev_upload(T** d, const std::vector<T>& h, size_t at_least = 1) {
  const size_t n = h.size() > at_least ? h.size() : at_least;
  HIPCHECK(hipMalloc((void**)d, n * sizeof(T)));
  if (!h.empty()) HIPCHECK(hipMemcpy(*d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
  return true;
}
static bool finish_launch() {
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  return true;
}

// ---- pool: words = 24 per point ----
static bool run_pool(const std::string&, Reader& r, std::vector<uint32_t>& out) {
  REQUIRE(r.n % 24 == 0);
  g_pool.clear();
  for (size_t i = 0; i < r.n / 24; i++) g_pool.push_back(ld_aff(r.p + 24 * i));
  out.push_back((uint32_t)g_pool.size());
  return true;
}

// ---- sort/<WPW>,<PERWIN>,<NBINS>[,digits]: flags | has_digits | first | ntot | n | n x 8 scalar words | has_digits x n x 9 digit words
// out: waves | maxrounds | per wave: rounds | per round: end | total | cnt[NBINS] | cur[NBINS] | order[NBINS] | list[total]
template <int WPW, bool PERWIN, int NBINS> static bool run_sort(const std::string&, Reader& r, std::vector<uint32_t>& out) {
  const uint32_t flags = r.u(), has_digits = r.u(), first = r.u(), ntot = r.u(), n = r.u();
  REQUIRE(r.ok && n <= 8192 && first <= ntot && ntot <= n && has_digits <= 1 && (!has_digits || PERWIN));
  const uint32_t* sc = r.take((size_t)n * 8);
  const uint32_t* dg = has_digits ? r.take((size_t)n * 9) : nullptr;
  REQUIRE(r.ok && r.o == r.n);
  std::vector<uint32_t> hs(sc, sc + (size_t)n * 8), hd;
  if (dg) hd.assign(dg, dg + (size_t)n * 9);
  uint32_t *d_sc = nullptr, *d_dg = nullptr, *d_out = nullptr;
  TblTask* d_task = nullptr;
  if (!dev_upload(&d_sc, hs) || !dev_upload(&d_dg, hd)) return false;
  TblTask task;
  memset(&task, 0, sizeof task);
  task.scalars = reinterpret_cast<const Fr*>(d_sc);
  task.flags = flags;
  task.digits = dg ? d_dg : nullptr;
  task.seg[0].n = n;
  if (!dev_upload(&d_task, std::vector<TblTask>(1, task))) return false;
  constexpr int WV = PERWIN ? 16 : TBW_WINDOWS / WPW;
  constexpr uint32_t REC = sort_rec_words<NBINS>();
  const uint32_t maxrounds = (ntot - first + 63) / 64 + 1;
  const size_t per_wave = 1 + (size_t)maxrounds * REC, words = per_wave * WV;
  REQUIRE(words <= MAX_WORDS);
  HIPCHECK(hipMalloc((void**)&d_out, words * 4));
  HIPCHECK(hipMemset(d_out, 0xa5, words * 4));
  const size_t lds = NBINS == 256 ? TBW2_LDS : (WPW == 2 && !PERWIN) ? TBW_LDS_CACHE : TBW_LDS;
  hipLaunchKernelGGL((k_sort<WPW, PERWIN, NBINS>), dim3(WV), dim3(64), lds, 0, d_task, first, ntot, d_out, maxrounds);
  if (!finish_launch()) return false;
  std::vector<uint32_t> h(words);
  HIPCHECK(hipMemcpy(h.data(), d_out, words * 4, hipMemcpyDeviceToHost));
  out.push_back(WV);
  out.push_back(maxrounds);
  for (int wv = 0; wv < WV; wv++) {
    const uint32_t* mine = h.data() + (size_t)wv * per_wave;
    const uint32_t rounds = mine[0] <= maxrounds ? mine[0] : 0;
    out.push_back(mine[0]);
    for (uint32_t k = 0; k < rounds; k++) {
      const uint32_t* rec = mine + 1 + (size_t)k * REC;
      const uint32_t total = rec[1] <= (uint32_t)TBW_CAP ? rec[1] : 0;
      out.insert(out.end(), rec, rec + 2 + 3 * NBINS + total);
    }
  }
  HIPCHECK(hipFree(d_sc));
  HIPCHECK(hipFree(d_dg));
  HIPCHECK(hipFree(d_out));
  HIPCHECK(hipFree(d_task));
  return true;
}

// ---- the bucket-list waves.  Payload:
//   slices | ntasks | ntables | per table: nrefs | refs                      (all tables of a case lie in ONE device array, in order)
//   per task: flags | pad | has_digits | n | seg 0: table | offset | copy_stride | n | nidx | seg 1: the same five
//             | n x 8 scalar words | has_digits x n x 9 digit words | idx of seg 0 | idx of seg 1        (nidx = 0: no gather list)
// out: waves | sets per wave | words of the front guard that lost the poison | of the back guard | of the raw_slot guards
//      | raw_slot[waves x sets] | per (wave, set, lane): 36 words + flag
enum { F_TBLW, F_TBLW2, F_PAIR };
struct TblwForm {
  int kind, wpw, perwin;
  int nsets() const { return (kind == F_PAIR || (kind == F_TBLW2 && wpw >= 16)) ? 4 : 2; }
  int waves() const { return perwin ? 16 : TBW_WINDOWS / wpw; }
  int copies() const { return perwin ? 2 : kind == F_TBLW2 ? 16 : 32; }
  size_t lds() const { return kind == F_TBLW2 && wpw >= 16 ? TBW2_LDS : (wpw == 2 && !perwin) ? TBW_LDS_CACHE : TBW_LDS; }
};
static bool launch_form(const TblwForm& f, int grid, const TblTask* t, uint32_t* raw, uint32_t* slot, int slices) {
  const dim3 g(grid), b(64);
  const size_t lds = f.lds();
#define L1(W, P) hipLaunchKernelGGL((k_tblw<W, P>), g, b, lds, 0, t, raw, slot, slices)
#define L2(W) hipLaunchKernelGGL((k_tblw2<W>), g, b, lds, 0, t, raw, slot, slices)
  if (f.kind == F_PAIR) hipLaunchKernelGGL(k_pair, g, b, lds, 0, t, raw, slot);
  else if (f.kind == F_TBLW && f.perwin) L1(2, true);
  else if (f.kind == F_TBLW) {
    switch (f.wpw) {
      case 2: L1(2, false); break;
      case 4: L1(4, false); break;
      case 8: L1(8, false); break;
      case 16: L1(16, false); break;
      default: L1(32, false); break;
    }
  } else {
    switch (f.wpw) {
      case 2: L2(2); break;
      case 4: L2(4); break;
      case 8: L2(8); break;
      case 16: L2(16); break;
      default: L2(32); break;
    }
  }
#undef L1
#undef L2
  return finish_launch();
}
static bool run_tblw_form(const TblwForm& f, Reader& r, std::vector<uint32_t>& out) {
  const uint32_t slices = r.u(), ntasks = r.u(), ntables = r.u();
  REQUIRE(r.ok && (slices == 1 || slices == 2 || slices == 4) && ntasks >= 1 && ntasks <= 64 && ntables >= 1 && ntables <= 64);
  REQUIRE(f.kind != F_PAIR || (slices == 1 && ntasks % 2 == 0));
  std::vector<TAff> tab;
  std::vector<size_t> tab_first, tab_size;
  for (uint32_t t = 0; t < ntables; t++) {
    const uint32_t nrefs = r.u();
    const uint32_t* refs = r.take(nrefs);
    REQUIRE(r.ok);
    tab_first.push_back(tab.size());
    tab_size.push_back(nrefs);
    for (uint32_t i = 0; i < nrefs; i++) {
      TAff a;
      REQUIRE(ref_point(refs[i], a));
      tab.push_back(a);
    }
  }
  TAff* d_tab = nullptr;
  if (!dev_upload(&d_tab, tab)) return false;
  std::vector<TblTask> tasks(ntasks);
  std::vector<void*> owned;
  for (uint32_t t = 0; t < ntasks; t++) {
    TblTask& tk = tasks[t];
    memset(&tk, 0, sizeof tk);
    tk.flags = r.u();
    tk.pad = r.u();
    const uint32_t has_digits = r.u(), n = r.u();
    uint32_t tb[2], off[2], nidx[2];
    for (int s = 0; s < 2; s++) {
      tb[s] = r.u();
      off[s] = r.u();
      tk.seg[s].copy_stride = r.u();
      tk.seg[s].n = r.u();
      nidx[s] = r.u();
    }
    REQUIRE(r.ok && n <= 8192 && tk.seg[0].n + tk.seg[1].n == n && has_digits <= 1 && (!has_digits || f.perwin));
    const uint32_t* sc = r.take((size_t)n * 8);
    const uint32_t* dg = has_digits ? r.take((size_t)n * 9) : nullptr;
    REQUIRE(r.ok);
    uint32_t* d_sc = nullptr;
    if (!dev_upload(&d_sc, std::vector<uint32_t>(sc, sc + (size_t)n * 8))) return false;
    owned.push_back(d_sc);
    tk.scalars = reinterpret_cast<const Fr*>(d_sc);
    if (dg) {
      uint32_t* d_dg = nullptr;
      if (!dev_upload(&d_dg, std::vector<uint32_t>(dg, dg + (size_t)n * 9))) return false;
      owned.push_back(d_dg);
      tk.digits = d_dg;
    }
    for (int s = 0; s < 2; s++) {
      REQUIRE(nidx[s] == 0 || nidx[s] == tk.seg[s].n);
      const uint32_t* ix = r.take(nidx[s]);
      REQUIRE(r.ok);
      if (tk.seg[s].n == 0) continue;
      REQUIRE(tb[s] < ntables);
      // every address a wave can form: copy * copy_stride + index, copy < copies(), index < n or a gather entry
      uint32_t top = tk.seg[s].n - 1;
      if (nidx[s]) {
        top = 0;
        for (uint32_t i = 0; i < nidx[s]; i++) top = ix[i] > top ? ix[i] : top;
      }
      REQUIRE((size_t)off[s] + (size_t)(f.copies() - 1) * tk.seg[s].copy_stride + top < tab_size[tb[s]]);
      tk.seg[s].base = d_tab + tab_first[tb[s]] + off[s];
      if (nidx[s]) {
        uint32_t* d_ix = nullptr;
        if (!dev_upload(&d_ix, std::vector<uint32_t>(ix, ix + nidx[s]))) return false;
        owned.push_back(d_ix);
        tk.seg[s].idx = d_ix;
      }
    }
  }
  REQUIRE(r.ok && r.o == r.n);
  if (f.kind == F_PAIR)   // a pair's second task: the same shape and scalars, other bases
    for (uint32_t t = 0; t < ntasks; t += 2)
      REQUIRE(tasks[t].seg[0].n == tasks[t + 1].seg[0].n && tasks[t].seg[1].n == 0 && tasks[t + 1].seg[1].n == 0 && tasks[t].seg[0].copy_stride == tasks[t + 1].seg[0].copy_stride &&
              !tasks[t].seg[0].idx && !tasks[t + 1].seg[0].idx);
  TblTask* d_tasks = nullptr;
  if (!dev_upload(&d_tasks, tasks)) return false;
  const int nsets = f.nsets(), waves = (int)(f.kind == F_PAIR ? ntasks / 2 : ntasks) * f.waves() * (int)slices;
  const size_t sets = (size_t)waves * nsets, raw_words = (sets + 2) * RAW_SET_WORDS, slot_words = sets + 128;
  uint32_t *d_raw = nullptr, *d_slot = nullptr;
  HIPCHECK(hipMalloc((void**)&d_raw, raw_words * 4));
  HIPCHECK(hipMemset(d_raw, 0xa5, raw_words * 4));   // one guard set before and one after the raw sets, poisoned with them
  HIPCHECK(hipMalloc((void**)&d_slot, slot_words * 4));
  HIPCHECK(hipMemset(d_slot, 0xa5, slot_words * 4));
  if (!launch_form(f, waves, d_tasks, d_raw + RAW_SET_WORDS, d_slot + 64, (int)slices)) return false;
  std::vector<uint32_t> raw(raw_words), slot(slot_words);
  HIPCHECK(hipMemcpy(raw.data(), d_raw, raw_words * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(slot.data(), d_slot, slot_words * 4, hipMemcpyDeviceToHost));
  out.push_back((uint32_t)waves);
  out.push_back((uint32_t)nsets);
  out.push_back(count_not_poison(raw.data(), RAW_SET_WORDS));
  out.push_back(count_not_poison(raw.data() + (sets + 1) * RAW_SET_WORDS, RAW_SET_WORDS));
  out.push_back(count_not_poison(slot.data(), 64) + count_not_poison(slot.data() + 64 + sets, 64));
  out.insert(out.end(), slot.begin() + 64, slot.begin() + 64 + sets);
  for (size_t e = 0; e < sets * 64; e++) st_acc(out, raw.data() + RAW_SET_WORDS + e * ACC_WORDS);
  for (void* p : owned) HIPCHECK(hipFree(p));
  HIPCHECK(hipFree(d_tab));
  HIPCHECK(hipFree(d_tasks));
  HIPCHECK(hipFree(d_raw));
  HIPCHECK(hipFree(d_slot));
  return true;
}
static bool run_tblw(const std::string& name, Reader& r, std::vector<uint32_t>& out) {
  TblwForm f{F_TBLW, 2, 0};
  if (name == "pair") f = TblwForm{F_PAIR, 2, 1};
  else if (name == "tblw/2,perwin") f = TblwForm{F_TBLW, 2, 1};
  else if (name.rfind("tblw2/", 0) == 0) f = TblwForm{F_TBLW2, atoi(name.c_str() + 6), 0};
  else f = TblwForm{F_TBLW, atoi(name.c_str() + 5), 0};
  return run_tblw_form(f, r, out);
}

// ---- fix/<CB>,<WPW>: nc | ntasks | nrows | per row: window | |d| - 1 | column | ref
//      | per task: flags | off | n | out_first | nidx | n x 8 scalar words | idx
// The table has the full extent the body addresses (W x 2^(CB-1) x nc entries, poisoned) and holds the listed entries only.
// out: waves | guard words front | back | raw_slot guards | raw_slot[waves] | per (wave, lane): 36 words + flag
template <int CB, int FIX_WPW> static bool run_fix(const std::string&, Reader& r, std::vector<uint32_t>& out) {
  constexpr int W = (256 + CB - 1) / CB, WG = W / FIX_WPW;
  constexpr uint32_t M = 1u << (CB - 1);
  const uint32_t nc = r.u(), ntasks = r.u(), nrows = r.u();
  REQUIRE(r.ok && nc >= 1 && nc <= 16 && ntasks >= 1 && ntasks <= 64 && nrows <= (1u << 20));
  const size_t entries = (size_t)W * M * nc;
  REQUIRE(entries * sizeof(TFix) <= ((size_t)3 << 30));
  TFix* d_tab = nullptr;
  HIPCHECK(hipMalloc((void**)&d_tab, entries * sizeof(TFix)));
  HIPCHECK(hipMemset(d_tab, 0x5a, entries * sizeof(TFix)));
  for (uint32_t i = 0; i < nrows; i++) {
    const uint32_t w = r.u(), m = r.u(), col = r.u(), ref = r.u();
    REQUIRE(r.ok && w < (uint32_t)W && m < M && col < nc);
    TFix e;
    memset(&e, 0, sizeof e);
    REQUIRE(ref_point(ref, e.a));
    HIPCHECK(hipMemcpy(d_tab + ((size_t)w * M + m) * nc + col, &e, sizeof e, hipMemcpyHostToDevice));
  }
  std::vector<FixTask> tasks(ntasks);
  std::vector<void*> owned;
  for (uint32_t t = 0; t < ntasks; t++) {
    FixTask& tk = tasks[t];
    memset(&tk, 0, sizeof tk);
    tk.flags = r.u();
    tk.off = r.u();
    tk.n = r.u();
    tk.out_first = r.u();
    const uint32_t nidx = r.u();
    REQUIRE(r.ok && tk.n <= 4096 && (nidx == 0 || nidx == tk.n));
    const uint32_t* sc = r.take((size_t)tk.n * 8);
    const uint32_t* ix = r.take(nidx);
    REQUIRE(r.ok);
    for (uint32_t i = 0; i < nidx; i++) REQUIRE((size_t)tk.off + ix[i] < nc);
    REQUIRE(nidx || tk.n == 0 || (size_t)tk.off + tk.n - 1 < nc);
    uint32_t* d_sc = nullptr;
    if (!dev_upload(&d_sc, std::vector<uint32_t>(sc, sc + (size_t)tk.n * 8))) return false;
    owned.push_back(d_sc);
    tk.scalars = reinterpret_cast<const Fr*>(d_sc);
    if (nidx) {
      uint32_t* d_ix = nullptr;
      if (!dev_upload(&d_ix, std::vector<uint32_t>(ix, ix + nidx))) return false;
      owned.push_back(d_ix);
      tk.idx = d_ix;
    }
  }
  REQUIRE(r.ok && r.o == r.n);
  FixTask* d_tasks = nullptr;
  if (!dev_upload(&d_tasks, tasks)) return false;
  const size_t sets = (size_t)ntasks * WG, raw_words = (sets + 2) * RAW_SET_WORDS, slot_words = sets + 128;
  uint32_t *d_raw = nullptr, *d_slot = nullptr;
  HIPCHECK(hipMalloc((void**)&d_raw, raw_words * 4));
  HIPCHECK(hipMemset(d_raw, 0xa5, raw_words * 4));
  HIPCHECK(hipMalloc((void**)&d_slot, slot_words * 4));
  HIPCHECK(hipMemset(d_slot, 0xa5, slot_words * 4));
  hipLaunchKernelGGL((k_fix<CB, FIX_WPW>), dim3((unsigned)sets), dim3(64), 16 * FIX_CHUNK * 2, 0, d_tasks, d_tab, (int)nc, d_raw + RAW_SET_WORDS, d_slot + 64);
  if (!finish_launch()) return false;
  std::vector<uint32_t> raw(raw_words), slot(slot_words);
  HIPCHECK(hipMemcpy(raw.data(), d_raw, raw_words * 4, hipMemcpyDeviceToHost));
  HIPCHECK(hipMemcpy(slot.data(), d_slot, slot_words * 4, hipMemcpyDeviceToHost));
  out.push_back((uint32_t)sets);
  out.push_back(count_not_poison(raw.data(), RAW_SET_WORDS));
  out.push_back(count_not_poison(raw.data() + (sets + 1) * RAW_SET_WORDS, RAW_SET_WORDS));
  out.push_back(count_not_poison(slot.data(), 64) + count_not_poison(slot.data() + 64 + sets, 64));
  out.insert(out.end(), slot.begin() + 64, slot.begin() + 64 + sets);
  for (size_t e = 0; e < sets * 64; e++) st_acc(out, raw.data() + RAW_SET_WORDS + e * ACC_WORDS);
  for (void* p : owned) HIPCHECK(hipFree(p));
  HIPCHECK(hipFree(d_tab));
  HIPCHECK(hipFree(d_tasks));
  HIPCHECK(hipFree(d_raw));
  HIPCHECK(hipFree(d_slot));
  return true;
}

// ---- reduce/wave, reduce/sets (Options::reduce_wave_max forced to "every launch" / 0): nplain | nweighted | per set: slot | 64 refs
// The entries enter as the accumulator a wave holds after adding the point to the identity.  out: nslots | per slot: 36 words + flag
// (flag bit 1: the slot still holds the poison)
static bool run_reduce(const std::string& name, Reader& r, std::vector<uint32_t>& out) {
  const uint32_t nplain = r.u(), nweighted = r.u(), nsets = nplain + nweighted;
  REQUIRE(r.ok && nsets >= 1 && nsets <= 4096 && nplain % 2 == 0);
  std::vector<uint32_t> raw((size_t)nsets * RAW_SET_WORDS), slot(nsets);
  std::vector<bool> seen(nsets, false);
  for (uint32_t s = 0; s < nsets; s++) {
    slot[s] = r.u();
    const uint32_t* refs = r.take(64);
    REQUIRE(r.ok && slot[s] < nsets && !seen[slot[s]]);
    seen[slot[s]] = true;
    for (int l = 0; l < 64; l++) {
      TAff a;
      REQUIRE(ref_point(refs[l], a));
      const TAcc acc = t_acc_add_mixed(TAcc::identity(), a);
      memcpy(raw.data() + (size_t)s * RAW_SET_WORDS + (size_t)l * ACC_WORDS, &acc, sizeof acc);
    }
  }
  REQUIRE(r.o == r.n);
  uint32_t *d_raw = nullptr, *d_slot = nullptr;
  TJac *d_mid = nullptr, *d_part = nullptr;
  if (!dev_upload(&d_raw, raw) || !dev_upload(&d_slot, slot)) return false;
  HIPCHECK(hipMalloc((void**)&d_mid, (size_t)nsets * reduce_mid_per_set() * sizeof(TJac)));
  HIPCHECK(hipMalloc((void**)&d_part, (size_t)nsets * sizeof(TJac)));
  HIPCHECK(hipMemset(d_part, 0xa5, (size_t)nsets * sizeof(TJac)));
  Options o = default_options();
  o.reduce_wave_max = name == "reduce/wave" ? (1L << 30) : 0;
  launch_reduce_sets(o, d_raw, d_slot, (int)nplain, (int)nweighted, d_mid, d_part, 0);
  if (!finish_launch()) return false;
  std::vector<TJac> part(nsets);
  HIPCHECK(hipMemcpy(part.data(), d_part, (size_t)nsets * sizeof(TJac), hipMemcpyDeviceToHost));
  out.push_back(nsets);
  for (uint32_t s = 0; s < nsets; s++) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(&part[s]);
    if (count_not_poison(w, sizeof(TJac) / 4) == 0) {
      for (int i = 0; i < 36; i++) out.push_back(0);
      out.push_back(2u);
      continue;
    }
    st_jac(out, t_jac_to_std(part[s]));
    out.push_back(part[s].is_identity() ? 1u : 0u);
  }
  HIPCHECK(hipFree(d_raw));
  HIPCHECK(hipFree(d_slot));
  HIPCHECK(hipFree(d_mid));
  HIPCHECK(hipFree(d_part));
  return true;
}

// ---- finalize/wave, finalize/ranges (Options::finalize_wave_max forced): n | nparts | naff | ncomp | has_dst | has_comp_index | has_addends
//      | nparts x 36 words (Jacobian, standard form) | naff x 24 words (the affine array before the launch) | first[n] | count[n]
//      | dst_index[n] | comp_index[n] | addends[3 n]                                                       (each only if flagged)
// out: naff x 24 words | ncomp x 12 words (0xa5 where nothing was written)
static bool run_finalize(const std::string& name, Reader& r, std::vector<uint32_t>& out) {
  const uint32_t n = r.u(), nparts = r.u(), naff = r.u(), ncomp = r.u(), has_dst = r.u(), has_ci = r.u(), has_add = r.u();
  REQUIRE(r.ok && n >= 1 && n <= 4096 && nparts <= 65536 && naff >= 1 && naff <= 65536 && ncomp >= 1 && ncomp <= 65536 && has_dst <= 1 && has_ci <= 1 && has_add <= 1);
  const uint32_t* pw = r.take((size_t)nparts * 36);
  const uint32_t* aw = r.take((size_t)naff * 24);
  const uint32_t* first = r.take(n);
  const uint32_t* count = r.take(n);
  const uint32_t* dst = has_dst ? r.take(n) : nullptr;
  const uint32_t* ci = has_ci ? r.take(n) : nullptr;
  const uint32_t* add = has_add ? r.take((size_t)3 * n) : nullptr;
  REQUIRE(r.ok && r.o == r.n);
  for (uint32_t g = 0; g < n; g++) {
    const uint32_t c = count[g] & 0xffffu, hi = count[g] >> 16;
    REQUIRE(hi <= c && (size_t)first[g] + c <= nparts && first[g] < (nparts ? nparts : 1u));
    REQUIRE((dst ? dst[g] : g) < naff && (ci ? ci[g] : g) < ncomp);
    for (int j = 0; add && j < 3; j++) REQUIRE(add[3 * g + j] == ~0u || add[3 * g + j] < naff);
  }
  std::vector<TJac> parts(nparts);
  for (uint32_t i = 0; i < nparts; i++) parts[i] = t_jac_from_std(ld_jac(pw + 36 * (size_t)i));
  std::vector<Aff> aff(naff);
  for (uint32_t i = 0; i < naff; i++) aff[i] = ld_aff(aw + 24 * (size_t)i);
  TJac* d_part = nullptr;
  Aff* d_aff = nullptr;
  uint32_t *d_first = nullptr, *d_count = nullptr, *d_dst = nullptr, *d_ci = nullptr, *d_add = nullptr;
  uint8_t* d_comp = nullptr;
  if (!dev_upload(&d_part, parts) || !dev_upload(&d_aff, aff)) return false;
  if (!dev_upload(&d_first, std::vector<uint32_t>(first, first + n)) || !dev_upload(&d_count, std::vector<uint32_t>(count, count + n))) return false;
  if (dst && !dev_upload(&d_dst, std::vector<uint32_t>(dst, dst + n))) return false;
  if (ci && !dev_upload(&d_ci, std::vector<uint32_t>(ci, ci + n))) return false;
  if (add && !dev_upload(&d_add, std::vector<uint32_t>(add, add + (size_t)3 * n))) return false;
  HIPCHECK(hipMalloc((void**)&d_comp, (size_t)ncomp * 48));
  HIPCHECK(hipMemset(d_comp, 0xa5, (size_t)ncomp * 48));
  Options o = default_options();
  o.finalize_wave_max = name == "finalize/wave" ? (1L << 30) : 0;
  launch_finalize_ranges(o, d_part, d_first, d_count, (int)n, d_aff, d_dst, d_comp, 0, d_add, d_ci);
  if (!finish_launch()) return false;
  HIPCHECK(hipMemcpy(aff.data(), d_aff, (size_t)naff * sizeof(Aff), hipMemcpyDeviceToHost));
  std::vector<uint32_t> comp((size_t)ncomp * 12);
  HIPCHECK(hipMemcpy(comp.data(), d_comp, (size_t)ncomp * 48, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < naff; i++) {
    for (int k = 0; k < 12; k++) out.push_back(aff[i].x.v[k]);
    for (int k = 0; k < 12; k++) out.push_back(aff[i].y.v[k]);
  }
  out.insert(out.end(), comp.begin(), comp.end());
  HIPCHECK(hipFree(d_part));
  HIPCHECK(hipFree(d_aff));
  HIPCHECK(hipFree(d_first));
  HIPCHECK(hipFree(d_count));
  if (d_dst) HIPCHECK(hipFree(d_dst));
  if (d_ci) HIPCHECK(hipFree(d_ci));
  if (d_add) HIPCHECK(hipFree(d_add));
  HIPCHECK(hipFree(d_comp));
  return true;
}

// ---- tail/wave, tail/lanes (Options::tail_wave_max forced): nout | group | shift | dup | extra_per_out
//      | nout x group x dup x 36 words | nout x extra_per_out x 36 words.      out: nout x 36 words (standard form)
static bool run_tail(const std::string& name, Reader& r, std::vector<uint32_t>& out) {
  const uint32_t nout = r.u(), group = r.u(), shift = r.u(), dup = r.u(), extra = r.u();
  REQUIRE(r.ok && nout >= 1 && nout <= 1024 && group >= 1 && group <= 16 && shift >= 1 && shift <= 16 && (dup == 1 || dup == 2 || dup == 4 || dup == 8) && extra <= 64 &&
          group * dup + extra <= 255);
  const size_t nin = (size_t)nout * group * dup, nex = (size_t)nout * extra;
  const uint32_t* iw = r.take(nin * 36);
  const uint32_t* ew = r.take(nex * 36);
  REQUIRE(r.ok && r.o == r.n);
  std::vector<TJac> in(nin), ex(nex);
  for (size_t i = 0; i < nin; i++) in[i] = t_jac_from_std(ld_jac(iw + 36 * i));
  for (size_t i = 0; i < nex; i++) ex[i] = t_jac_from_std(ld_jac(ew + 36 * i));
  TJac *d_in = nullptr, *d_ex = nullptr;
  Jac* d_out = nullptr;
  if (!dev_upload(&d_in, in) || !dev_upload(&d_ex, ex)) return false;
  HIPCHECK(hipMalloc((void**)&d_out, (size_t)nout * sizeof(Jac)));
  HIPCHECK(hipMemset(d_out, 0xa5, (size_t)nout * sizeof(Jac)));
  Options o = default_options();
  o.tail_wave_max = name == "tail/wave" ? (1L << 30) : 0;
  launch_msm_tail(o, d_in, nullptr, d_out, (int)nout, (int)group, (int)shift, 0, extra ? d_ex : nullptr, (int)extra, (int)dup);
  if (!finish_launch()) return false;
  std::vector<Jac> res(nout);
  HIPCHECK(hipMemcpy(res.data(), d_out, (size_t)nout * sizeof(Jac), hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < nout; i++) st_jac(out, res[i]);
  HIPCHECK(hipFree(d_in));
  HIPCHECK(hipFree(d_ex));
  HIPCHECK(hipFree(d_out));
  return true;
}

struct MsmEntry {
  const char* name;
  const char* group;
  bool (*run)(const std::string&, Reader&, std::vector<uint32_t>&);
};
static const MsmEntry TABLE[] = {
    {"pool", "pool", run_pool},
    // tbw_sort<WPW, PERWIN, NBINS, CACHE> as msm_tblw_body instantiates it for the kernels the library launches
    {"sort/2,0,128", "sort", run_sort<2, false, 128>},
    {"sort/4,0,128", "sort", run_sort<4, false, 128>},
    {"sort/8,0,128", "sort", run_sort<8, false, 128>},
    {"sort/16,0,128", "sort", run_sort<16, false, 128>},
    {"sort/32,0,128", "sort", run_sort<32, false, 128>},
    {"sort/16,0,256", "sort", run_sort<16, false, 256>},
    {"sort/32,0,256", "sort", run_sort<32, false, 256>},
    {"sort/2,1,128", "sort", run_sort<2, true, 128>},
    {"sort/2,1,128,digits", "sort", run_sort<2, true, 128>},
    // k_msm_tblw<2|4|8|16|32>, k_msm_tblw<2, true>, k_msm_tblw2<2|4|8|16|32>, k_msm_tblw_pair
    {"tblw/2", "tblw", run_tblw},
    {"tblw/4", "tblw", run_tblw},
    {"tblw/8", "tblw", run_tblw},
    {"tblw/16", "tblw", run_tblw},
    {"tblw/32", "tblw", run_tblw},
    {"tblw/2,perwin", "tblw", run_tblw},
    {"tblw2/2", "tblw", run_tblw},
    {"tblw2/4", "tblw", run_tblw},
    {"tblw2/8", "tblw", run_tblw},
    {"tblw2/16", "tblw", run_tblw},
    {"tblw2/32", "tblw", run_tblw},
    {"pair", "pair", run_tblw},
    // k_msm_fix<CB, FIX_WPW> (<16, 2> also in k_msm_fix_tblw)
    {"fix/16,16", "fix", run_fix<16, 16>},
    {"fix/16,8", "fix", run_fix<16, 8>},
    {"fix/16,4", "fix", run_fix<16, 4>},
    {"fix/16,2", "fix", run_fix<16, 2>},
    {"fix/8,16", "fix", run_fix<8, 16>},
    {"fix/8,8", "fix", run_fix<8, 8>},
    {"fix/19,7", "fix", run_fix<19, 7>},
    {"reduce/wave", "reduce", run_reduce},
    {"reduce/sets", "reduce", run_reduce},
    {"finalize/wave", "finalize", run_finalize},
    {"finalize/ranges", "finalize", run_finalize},
    {"tail/wave", "finalize", run_tail},
    {"tail/lanes", "finalize", run_tail},
};

static const MsmEntry* find_op(const char* name) {
  const MsmEntry* op = nullptr;
  for (const MsmEntry& e : TABLE)
    if (!strcmp(e.name, name)) op = &e;
  return op;
}

int main(int argc, char** argv) {
  return check_main(
      argc, argv, false,
      [] {
        for (const MsmEntry& e : TABLE) printf("%s %s\n", e.name, e.group);
      },
      [](const Header& h) -> int64_t { return find_op(h.name) && h.words == 1 && h.rows <= MAX_WORDS ? (int64_t)h.rows : -1; },
      [](Header& h, std::vector<uint32_t>& in, std::vector<uint32_t>& out, const CheckLoop& loop) -> int {
        Reader r{in.data(), in.size()};
        if (!find_op(h.name)->run(h.name, r, out)) {   // (never null: the payload callback has accepted the name)
          fprintf(stderr, "msm_check: record %zu '%s' failed\n", loop.records, h.name);
          return g_bad_case ? CHECK_BAD : CHECK_FAILED;
        }
        h.rows = out.size();
        return CHECK_OK;
      });
}
