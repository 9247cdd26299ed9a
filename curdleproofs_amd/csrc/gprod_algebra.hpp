// The scalar side of GrandProductProof::new (grand_product_argument.rs:43-166) over a scalar type F with the library's fe_* functions —
// host and device code, no HIP call: k_gprod_products and k_gprod_setup (gprod.hip) run it for every item of cpx_gprod_prove,
// tests/host_emul/gprod_plan_emul.cpp compiles it for the CPU (tests/test_gprod_cpu.py).
//
//   vec_c          1, b_0, b_0 b_1, ... (:69-73): entry i is the product of b_j, j < i.  The scan is split the way the kernel splits it:
//                  worker t of `workers` owns the positions [lo, hi) of gprod_chunk, multiplies its b together (gprod_chunk_product), the
//                  workers' products are combined exclusively — in log steps across the work-group (gprod_scan_step), or by one worker
//                  (gprod_scan_exclusive: the same values, what the CPU emulation checks the steps against) —, and every worker writes its positions starting from
//                  what came before it (gprod_chunk_fixup).  b[ell - 1] enters no entry.
//   r_p            <vec_b_blinders + alpha, vec_c_blinders> (:79-81)
//   u              beta^-(i+1), i < ell, then beta^-(ell+1) on the blinder positions: G' = u o (G | H) (:90-102).  The prover never forms
//                  G': u seeds the fold coefficients of the loop (loop_plan.hpp) and multiplies r_d for B_d.
//   vec_d          b_i beta^(i+1) - beta^i, i < ell, then beta^(ell+1) (r_b,k + alpha) (:105-126)
//   D's scalars    B - <beta-powers, G'> + <alpha beta^(ell+1), H'> (:129-132) is B - beta^-1 sum G + alpha sum H: -beta^-1 on the ell
//                  positions of G, alpha on those of H
//   inner_prod     r_p beta^(ell+1) + gprod_result beta^ell - 1 (:141-142)
#pragma once
#include <cstdint>
#include "mont32.hpp"

namespace cpx {

// the positions worker `tid` of `workers` owns: ceil(ell / workers) consecutive ones, the last owners fewer or none
CPX_HD void gprod_chunk(int ell, int workers, int tid, int& lo, int& hi) {
  const int per = (ell + workers - 1) / workers;
  lo = tid * per < ell ? tid * per : ell;
  hi = lo + per < ell ? lo + per : ell;
}
template <class F> CPX_HD F gprod_chunk_product(const F* b, int lo, int hi) {
  F p = F::one();
  for (int i = lo; i < hi; i++) p = fe_mul(p, b[i]);
  return p;
}
// part[t] = the product of part[s], s < t (in place, one worker)
template <class F> CPX_HD void gprod_scan_exclusive(F* part, int workers) {
  F run = F::one();
  for (int t = 0; t < workers; t++) {
    const F x = part[t];
    part[t] = run;
    run = fe_mul(run, x);
  }
}
// ... or by all workers in ceil(log2 workers) steps (k_gprod_products): step `off` = 1, 2, 4, ... takes worker tid's inclusive product over
// the 2 off chunks ending at tid from those over `off` chunks in `in`; after the last step worker t's exclusive product is out[t - 1], and 1 for t = 0
template <class F> CPX_HD F gprod_scan_step(const F* in, int tid, int off) { return tid >= off ? fe_mul(in[tid - off], in[tid]) : in[tid]; }
// c[i] for the worker's positions, `before` = the product of every b ahead of lo
template <class F> CPX_HD void gprod_chunk_fixup(const F* b, int lo, int hi, const F& before, F* c) {
  F run = before;
  for (int i = lo; i < hi; i++) {
    c[i] = run;
    run = fe_mul(run, b[i]);
  }
}
template <class F> CPX_HD F gprod_r_p(const F* rb, const F* c_blinders, int nb, const F& alpha) {
  F s = F::zero();
  for (int k = 0; k < nb; k++) s = fe_add(s, fe_mul(fe_add(rb[k], alpha), c_blinders[k]));
  return s;
}
template <class F> CPX_HD F gprod_pow(const F& x, uint64_t e) {
  F r = F::one(), sq = x;
  for (; e; e >>= 1) {
    if (e & 1) r = fe_mul(r, sq);
    sq = fe_mul(sq, sq);
  }
  return r;
}
// u, vec_d and D's scalars on the positions [lo, hi) of the ell factors
template <class F> CPX_HD void gprod_fill_chunk(const F* b, int lo, int hi, const F& beta, const F& beta_inv, F* u, F* d, F* d_scalars) {
  if (lo >= hi) return;
  F pw = gprod_pow(beta, (uint64_t)lo), ipw = gprod_pow(beta_inv, (uint64_t)lo + 1);   // beta^i, beta^-(i+1)
  const F minus = fe_neg(beta_inv);
  for (int i = lo; i < hi; i++) {
    const F next = fe_mul(pw, beta);
    d[i] = fe_sub(fe_mul(b[i], next), pw);
    u[i] = ipw;
    d_scalars[i] = minus;
    pw = next;
    ipw = fe_mul(ipw, beta_inv);
  }
}
// ... and on the blinder positions k = first, first + step, ... < nb (at ell + k)
template <class F> CPX_HD void gprod_fill_blinders(const F* rb, int ell, int nb, int first, int step, const F& alpha, const F& beta_l1, const F& beta_inv_l1, F* u, F* d,
                                                   F* d_scalars) {
  for (int k = first; k < nb; k += step) {
    d[ell + k] = fe_mul(beta_l1, fe_add(rb[k], alpha));
    u[ell + k] = beta_inv_l1;
    d_scalars[ell + k] = alpha;
  }
}
// the verifier's vec_u (:214-220) on the positions [lo, hi) of all n: beta^-(i+1) below ell, beta_inv_l1 = beta^-(ell+1) from there on
template <class F> CPX_HD void gprod_fill_u(int lo, int hi, int ell, const F& beta_inv, const F& beta_inv_l1, F* u) {
  if (lo >= hi) return;
  F ipw = lo < ell ? gprod_pow(beta_inv, (uint64_t)lo + 1) : beta_inv_l1;
  for (int i = lo; i < hi; i++) {
    u[i] = i < ell ? ipw : beta_inv_l1;
    ipw = fe_mul(ipw, beta_inv);
  }
}
// beta_l = beta^ell
template <class F> CPX_HD F gprod_inner_prod(const F& r_p, const F& gprod_result, const F& beta_l, const F& beta) {
  return fe_sub(fe_add(fe_mul(r_p, fe_mul(beta_l, beta)), fe_mul(gprod_result, beta_l)), F::one());
}

}  // namespace cpx
