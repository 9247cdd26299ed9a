// The scalar side of SamePermutationProof::new and ::verify (same_permutation_argument.rs:40-171) over a scalar type F with the library's
// fe_* functions — host and device code, no HIP call: the kernels of same_perm.hip run it for every item of cpx_same_perm_prove /
// cpx_same_perm_verify, tests/host_emul/same_perm_plan_emul.cpp compiles it for the CPU (tests/test_same_perm_cpu.py).
//
//   factors        a_sigma(i) + sigma(i) alpha + beta (:66-72); the verifier's a_i + i alpha + beta (:140-144)
//   gprod_result   their product (:73, :145): every worker multiplies its chunk of gprod_algebra.hpp together, the chunks' products are
//                  combined by that header's log steps, and the last worker's inclusive product is the result — the scan of
//                  k_gprod_products, of which only the total is kept
//   vec_b_blinders r_a + alpha r_m (:78-81)
//   B's scalars    B = A + alpha M + beta sum G (:76): beta on the ell positions of G, alpha on M; A is added as a point
//   the check      accumulate_check(B - A - alpha M, beta repeated, G) (:149) with the factor a_0, in the convention of
//                  subarg_check_plan.hpp (sum_k a_k (<x_k, V_k> - lhs_k) == O): a_0 beta more on every G_i, -a_0 on B, +a_0 on A,
//                  +a_0 alpha on M
#pragma once
#include <cstdint>
#include "mont32.hpp"
#include "gprod_algebra.hpp"

namespace cpx {

template <class F> CPX_HD F same_perm_from_u32(uint32_t x) {   // Fr::from(u32)
  F c = F::zero();
  c.v[0] = x;
  return fe_to_mont(c);
}
template <class F> CPX_HD F same_perm_factor(const F& a, uint32_t index, const F& alpha, const F& beta) {
  return fe_add(fe_add(a, fe_mul(same_perm_from_u32<F>(index), alpha)), beta);
}
template <class F> CPX_HD F same_perm_blinder(const F& r_a, const F& r_m, const F& alpha) { return fe_add(r_a, fe_mul(alpha, r_m)); }
// the canonical little-endian bytes of a scalar as eight words (ark-serialize Fr), what the transcript absorbs
template <class F> CPX_HD void same_perm_canonical(const F& x_mont, uint32_t* w) {
  const F c = fe_from_mont(x_mont);
  for (int j = 0; j < 8; j++) w[j] = c.v[j];
}
// the factors of the positions [lo, hi): permuted (perm != nullptr, every entry < ell) or in index order; returns their product
template <class F> CPX_HD F same_perm_fill_chunk(const F* a, const uint32_t* perm, int lo, int hi, const F& alpha, const F& beta, F* factors) {
  F p = F::one();
  for (int i = lo; i < hi; i++) {
    const uint32_t s = perm ? perm[i] : (uint32_t)i;
    const F f = same_perm_factor(a[s], s, alpha, beta);
    if (factors) factors[i] = f;
    p = fe_mul(p, f);
  }
  return p;
}
// the product of all chunks by one worker: what the log steps of gprod_scan_step leave with the last worker
template <class F> CPX_HD F same_perm_product_serial(const F* part, int workers) {
  F run = F::one();
  for (int t = 0; t < workers; t++) run = fe_mul(run, part[t]);
  return run;
}
// ---- the verifier's extra weights ----
template <class F> struct SamePermWeights {
  F g_add, B, A, M;
};
template <class F> CPX_HD SamePermWeights<F> same_perm_weights(const F& a0, const F& alpha, const F& beta) {
  SamePermWeights<F> w;
  w.g_add = fe_mul(a0, beta);
  w.B = fe_neg(a0);
  w.A = a0;
  w.M = fe_mul(a0, alpha);
  return w;
}

}  // namespace cpx
