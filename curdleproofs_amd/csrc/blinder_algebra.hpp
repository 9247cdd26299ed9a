// generate_ipa_blinders (inner_product_argument.rs:42-82) on the library's Fr — host and device code, no HIP call: k_subarg_blinders
// (subarg_prove.hip) runs it for every item of cpx_ipa_prove, tests/host_emul/subarg_prove_plan_emul.cpp compiles it for the CPU
// (tests/test_subarg_prove_cpu.py).  The same algebra stands in k_ps_gprod (protocol.hip) for the whole-proof prover.
//
// r = n draws, z = n - 2 draws; the two last entries of z are solved for so that <r, d> + <z, c> = 0 and <r, z> = 0:
//     omega = <r, d> + <z[..n-2], c[..n-2]>,  delta = <r[..n-2], z[..n-2]>,  inv_c = 1 / c[n-2]
//     last_z = (r[n-2] inv_c omega - delta) / (-r[n-2] inv_c c[n-1] + r[n-1]),  pen_z = -inv_c (last_z c[n-1] + omega)
// The reference panics where an inverse does not exist (:69 c[n-2] = 0, :71 the denominator = 0): `singular`, nothing else is claimed.
// At n = 2 there is no free z and delta is an empty sum.
#pragma once
#include "mont32.hpp"
#include "modinv30.hpp"

namespace cpx {

// what one of `step` workers adds to omega and delta: the elements first, first + step, ...
CPX_HD void ipa_blinder_partial(const Fr* r, const Fr* z, const Fr* c, const Fr* d, int n, int first, int step, Fr& omega, Fr& delta) {
  for (int i = first; i < n; i += step) {
    omega = fe_add(omega, fe_mul(r[i], d[i]));
    if (i < n - 2) {
      omega = fe_add(omega, fe_mul(z[i], c[i]));
      delta = fe_add(delta, fe_mul(r[i], z[i]));
    }
  }
}

struct IpaBlinderTail {
  Fr pen_z, last_z;   // z[n-2], z[n-1]; zero when singular
  bool singular;
};
// r_pen, r_last = r[n-2], r[n-1]; c_pen, c_last = c[n-2], c[n-1]
CPX_HD IpaBlinderTail ipa_blinder_solve(const Fr& omega, const Fr& delta, const Fr& r_pen, const Fr& r_last, const Fr& c_pen, const Fr& c_last) {
  IpaBlinderTail t{Fr::zero(), Fr::zero(), true};
  // den = den_c / c[n-2] with den_c = r[n-1] c[n-2] - r[n-2] c[n-1]: both inverses from ONE inversion of c[n-2] den_c (inverses are
  // unique, so the field values are the reference's); either factor zero <=> one of the reference's two inverses does not exist
  const Fr den_c = fe_sub(fe_mul(r_last, c_pen), fe_mul(r_pen, c_last));
  const Fr prod = fe_mul(c_pen, den_c);
  if (prod.is_zero()) return t;
  const Fr inv = fr_inv_divsteps(prod);
  const Fr inv_c = fe_mul(inv, den_c), inv_den = fe_mul(fe_mul(inv, c_pen), c_pen);
  t.last_z = fe_mul(fe_sub(fe_mul(fe_mul(r_pen, inv_c), omega), delta), inv_den);
  t.pen_z = fe_mul(fe_neg(inv_c), fe_add(fe_mul(t.last_z, c_last), omega));
  t.singular = false;
  return t;
}

}  // namespace cpx
