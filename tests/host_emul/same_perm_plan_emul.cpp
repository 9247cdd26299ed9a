// g++ program over curdleproofs_amd/csrc/same_perm_plan.hpp and same_perm_algebra.hpp (tests/test_same_perm_cpu.py): the layouts of
// cpx_same_perm_prove / cpx_same_perm_verify exactly as the engine and the kernels of same_perm.hip use them, and the layer's algebra
// computed the way k_same_perm_step computes it (`workers` threads, each with its chunk, the chunk products combined in log steps), printed
// as plain "key value..." lines.  The test builds it twice, the second time with -fsanitize=address,undefined.
//   same_perm_plan_emul plan <count> <ell> <nb>      the prover's plan: every region as "name start size", or the status alone
//   same_perm_plan_emul check <count> <ell> <nb>     the verifier's plan likewise
//   same_perm_plan_emul layer <workers> <ell> <nb> <hex>...   alpha, beta, a [ell], perm [ell] (hex u32), ra [nb], rm [nb]:
//                                                    "factors" [ell], "product", "serial" (the product by one worker), "vproduct" (the
//                                                    verifier's, index order), "rb" [nb], "bsc" [ell + 1]
//   same_perm_plan_emul weights <a0> <alpha> <beta>  "w" g_add B A M
//   same_perm_plan_emul canon <hex>                  the eight canonical words of a scalar, as the transcript absorbs them
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../curdleproofs_amd/csrc/same_perm_algebra.hpp"
#include "../../curdleproofs_amd/csrc/same_perm_plan.hpp"

using namespace cpx;

static Fr from_hex(const char* s) {   // canonical integer -> Montgomery
  Fr c = Fr::zero();
  const size_t len = strlen(s);
  for (size_t i = 0; i < len && i < 64; i++) {
    const char ch = s[len - 1 - i];
    const uint32_t d = ch >= '0' && ch <= '9' ? (uint32_t)(ch - '0') : (uint32_t)((ch | 0x20) - 'a' + 10);
    c.v[i / 8] |= (d & 15u) << (4 * (i % 8));
  }
  return fe_to_mont(c);
}
static void print_hex(const Fr& mont) {
  const Fr c = fe_from_mont(mont);
  printf(" ");
  for (int j = 7; j >= 0; j--) printf("%08x", c.v[j]);
}
static void print_vec(const char* name, const std::vector<Fr>& v) {
  printf("%s", name);
  for (const Fr& x : v) print_hex(x);
  printf("\n");
}
static void region(const char* name, size_t start, size_t end) { printf("%s %zu %zu\n", name, start, end - start); }
static void print_totals(const char* name, const SubargTotals& t) {   // what the engine reserves at a depth, and what leads the inner proof
  printf("%s %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", name, t.fr, t.jac, t.aff, t.bytes, t.flags, t.ix, t.tasks, t.res, t.lead_bytes, t.lead_challenges);
}

// the product of the factors the way the work-group forms it; `factors` may be empty (the verifier keeps none)
static Fr product(int workers, int ell, const Fr* a, const uint32_t* perm, const Fr& alpha, const Fr& beta, Fr* factors, Fr& serial) {
  std::vector<Fr> part((size_t)workers), next((size_t)workers);
  for (int t = 0; t < workers; t++) {
    int lo, hi;
    gprod_chunk(ell, workers, t, lo, hi);
    part[(size_t)t] = same_perm_fill_chunk(a, perm, lo, hi, alpha, beta, factors);
  }
  serial = same_perm_product_serial(part.data(), workers);
  for (int off = 1; off < workers; off <<= 1) {
    for (int t = 0; t < workers; t++) next[(size_t)t] = gprod_scan_step(part.data(), t, off);
    part.swap(next);
  }
  return part[(size_t)workers - 1];
}

int main(int argc, char** argv) {
  if (argc >= 5 && !strcmp(argv[1], "layer")) {
    const int workers = atoi(argv[2]), ell = atoi(argv[3]), nb = atoi(argv[4]);
    if (workers < 1 || ell < 1 || nb < 0 || argc != 5 + 2 + 2 * ell + 2 * nb) {
      fprintf(stderr, "layer: workers >= 1, ell >= 1 and 2 + 2 ell + 2 nb values expected\n");
      return 2;
    }
    const Fr alpha = from_hex(argv[5]), beta = from_hex(argv[6]);
    std::vector<Fr> a((size_t)ell), ra((size_t)nb), rm((size_t)nb), factors((size_t)ell), rb((size_t)nb), bsc((size_t)ell + 1);
    std::vector<uint32_t> perm((size_t)ell);
    for (int i = 0; i < ell; i++) a[(size_t)i] = from_hex(argv[7 + i]);
    for (int i = 0; i < ell; i++) {
      perm[(size_t)i] = (uint32_t)strtoul(argv[7 + ell + i], nullptr, 16);
      if (perm[(size_t)i] >= (uint32_t)ell) return 2;   // the engine refuses such a call before a kernel sees it
    }
    for (int k = 0; k < nb; k++) ra[(size_t)k] = from_hex(argv[7 + 2 * ell + k]);
    for (int k = 0; k < nb; k++) rm[(size_t)k] = from_hex(argv[7 + 2 * ell + nb + k]);
    Fr serial, vserial;
    const Fr p = product(workers, ell, a.data(), perm.data(), alpha, beta, factors.data(), serial);
    const Fr vp = product(workers, ell, a.data(), nullptr, alpha, beta, nullptr, vserial);
    for (int k = 0; k < nb; k++) rb[(size_t)k] = same_perm_blinder(ra[(size_t)k], rm[(size_t)k], alpha);
    for (int i = 0; i < ell; i++) bsc[(size_t)i] = beta;
    bsc[(size_t)ell] = alpha;
    print_vec("factors", factors);
    print_vec("product", {p});
    print_vec("serial", {serial});
    print_vec("vproduct", {vp});
    print_vec("vserial", {vserial});
    print_vec("rb", rb);
    print_vec("bsc", bsc);
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "weights")) {
    const SamePermWeights<Fr> w = same_perm_weights(from_hex(argv[2]), from_hex(argv[3]), from_hex(argv[4]));
    print_vec("w", {w.g_add, w.B, w.A, w.M});
    return 0;
  }
  if (argc == 3 && !strcmp(argv[1], "canon")) {
    uint32_t w[8];
    same_perm_canonical(from_hex(argv[2]), w);
    printf("words");
    for (int j = 0; j < 8; j++) printf(" %u", w[j]);
    printf("\n");
    return 0;
  }
  if (argc != 5 || (strcmp(argv[1], "plan") && strcmp(argv[1], "check"))) {
    fprintf(stderr, "usage: same_perm_plan_emul plan|check <count> <ell> <nb> | layer ... | weights ... | canon <hex>\n");
    return 2;
  }
  const size_t count = (size_t)strtoull(argv[2], nullptr, 10), ell = (size_t)strtoull(argv[3], nullptr, 10), nb = (size_t)strtoull(argv[4], nullptr, 10);
  if (!strcmp(argv[1], "plan")) {
    SamePermProvePlan pl;
    const int status = (int)same_perm_prove_plan(count, ell, nb, pl);
    printf("status %d\n", status);
    if (status != GPROD_OK) return 0;
    const GprodProvePlan& gp = pl.gp;
    printf("draws_each %zu\nchallenges %zu\nproof_bytes %zu\nmessage_bytes %zu\nbytes %zu %zu %zu %zu\n", pl.draws_each(), pl.challenges(), pl.proof_bytes(),
           pl.message_bytes(), pl.byte_B(), pl.byte_gprod(), pl.byte_gprod() + gp.byte_rp(), pl.byte_gprod() + gp.byte_ipa());
    region("fr.gp", 0, gp.fr_total());
    region("fr.a", pl.fr_a(), pl.fr_ra());
    region("fr.ra", pl.fr_ra(), pl.fr_rm());
    region("fr.rm", pl.fr_rm(), pl.fr_bsc());
    region("fr.bsc", pl.fr_bsc(), pl.fr_chal());
    region("fr.chal", pl.fr_chal(), pl.fr_total());
    region("ix.gp", 0, gp.ix_total());
    region("ix.perm", pl.ix_perm(), pl.ix_gather());
    region("ix.gather", pl.ix_gather(), pl.ix_addend());
    region("ix.addend", pl.ix_addend(), pl.ix_total());
    region("jac.gp", 0, gp.jac_total());
    region("jac.A", pl.jac_A(), pl.jac_M());
    region("jac.M", pl.jac_M(), pl.jac_total());
    region("aff.gp", 0, gp.aff_total());
    region("aff.A", pl.aff_A(), pl.aff_M());
    region("aff.M", pl.aff_M(), pl.aff_total());
    region("by.gp", 0, gp.by_total());
    region("by.A", pl.by_A(), pl.by_M());
    region("by.M", pl.by_M(), pl.by_total());
    region("task.gp", 0, gp.task_total());
    region("task.B", pl.task_B(), pl.task_total());
    printf("aff_B %zu\nrow %zu %zu\n", pl.aff_B(), gp.sp.lp.base_stride(), gp.sp.lp.h_index());
    print_totals("totals", pl.totals());
    print_totals("totals_gp", gp.totals());
    print_totals("totals_core", gp.sp.totals());
    printf("flags_total %zu\nres_end %zu %zu\n", gp.flags_total(), gp.res_total(), gp.sp.lp.results());
    std::vector<uint32_t> gather, addend, lens;
    pl.fill_lists(gather, addend);
    printf("gather");
    for (uint32_t v : gather) printf(" %u", v);
    printf("\naddend");
    for (uint32_t v : addend) printf(" %u", v);
    printf("\n");
    Tier0MsmPlan mp;
    const bool ok = pl.item_msm(mp, lens);
    printf("msm %d %zu %zu %u\n", ok ? 1 : 0, mp.count, mp.points, mp.max_n);
    return 0;
  }
  SamePermCheckPlan pl;
  const int status = (int)same_perm_check_plan(count, ell, nb, pl);
  printf("status %d\n", status);
  if (status != SUBARG_OK) return 0;
  const GprodCheckPlan& gp = pl.gp;
  printf("checks %d\nchallenges %zu\nproof_bytes %zu\npoints %zu\nrow %zu %zu %zu %zu\n", pl.checks(), pl.challenges(), pl.proof_bytes(), gp.sp.points(),
         gp.sp.statement_off(), pl.row_B(), pl.row_A(), pl.row_M());
  region("fr.gp", 0, gp.fr_total());
  region("fr.a0", pl.fr_a0(), pl.fr_a());
  region("fr.a", pl.fr_a(), pl.fr_chal());
  region("fr.chal", pl.fr_chal(), pl.fr_total());
  region("by.gp", 0, gp.by_total());
  region("by.A", pl.by_A(), pl.by_M());
  region("by.M", pl.by_M(), pl.by_total());
  region("st.gp", 0, gp.st_total());
  region("st.B", pl.st_B(), pl.st_total());
  region("ix.gp", 0, gp.ix_total());
  region("ix.AM", pl.ix_AM_dst(), pl.ix_total());
  region("jac.stmt", 0, pl.jac_A());
  region("jac.AM", pl.jac_A(), pl.jac_total());
  printf("fr_weights_end %zu\n", gp.sp.fr_z());
  print_totals("totals", pl.totals());
  print_totals("totals_gp", gp.totals());
  print_totals("totals_core", gp.sp.totals());
  printf("aff_total %zu\n", gp.aff_total());
  std::vector<uint32_t> ix;
  pl.fill_idx(ix);
  printf("lists");
  for (uint32_t v : ix) printf(" %u", v);
  printf("\n");
  return 0;
}
