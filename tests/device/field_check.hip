// TEST-ONLY: every operation of the field and point headers (mont32.hpp, fp28.hpp, g1_28.hpp) on raw limbs, one source
// compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row,
//                                         64-thread blocks, plain vector loads and stores
// tests/test_field_check_cpu.py and tests/test_gpu_field.py feed both the same rows and compare the results with each other
// and with Python integers.  Nothing in curdleproofs_amd/ links it.
//
// The command line, the record format, the exit codes and the runner are those of check_harness.hpp; --list prints name, input
// words per row, output words per row.
//
// Every (operation, body) pair is a type of its own, so each body is compiled on its own as it is inside the product's kernels.
// Body numbers as in tests/host_emul/f28_redc_bodies.cpp: 0 = schoolbook, 1 = Karatsuba a b columns with the schoolbook
// reduction, 2 = Karatsuba a b columns and Karatsuba reduction (squares: 0 = schoolbook, 2 = Karatsuba), -1 = the default.
#define CHECK_PROG "field_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/mont32.hpp"
#include "../../curdleproofs_amd/csrc/fp28.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"

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
template <class C> CPX_HD Fe<C> ldfe(const uint32_t* w) {
  Fe<C> r;
  CPX_UNROLL for (int i = 0; i < C::N; i++) r.v[i] = w[i];
  return r;
}
template <class C> CPX_HD void stfe(uint32_t* w, const Fe<C>& a) {
  CPX_UNROLL for (int i = 0; i < C::N; i++) w[i] = a.v[i];
}
CPX_HD Aff28 ldaff(const uint32_t* w) { return Aff28{ld28(w), ld28(w + 14)}; }
CPX_HD Jac28 ldjac(const uint32_t* w) { return Jac28{ld28(w), ld28(w + 14), ld28(w + 28)}; }
CPX_HD Xyzz28 ldxyzz(const uint32_t* w) { return Xyzz28{ld28(w), ld28(w + 14), ld28(w + 28), ld28(w + 42)}; }
CPX_HD void stjac(uint32_t* w, const Jac28& p) {
  st28(w, p.x);
  st28(w + 14, p.y);
  st28(w + 28, p.z);
}
CPX_HD void stxyzz(uint32_t* w, const Xyzz28& p) {
  st28(w, p.x);
  st28(w + 14, p.y);
  st28(w + 28, p.zz);
  st28(w + 42, p.zzz);
}

// fp28.hpp products, every body, inlined (_body) and through the out-of-line register entry
template <bool K, bool RK> OP(F28MulBody, 28, 14, st28(out, f28_mul_body<K, RK>(ld28(in), ld28(in + 14)));)
OP(F28MulBodyDef, 28, 14, st28(out, f28_mul_body<>(ld28(in), ld28(in + 14)));)
template <bool K, bool RK> OP(F28Mul, 28, 14, st28(out, f28_mul<K, RK>(ld28(in), ld28(in + 14)));)
OP(F28MulDef, 28, 14, st28(out, f28_mul<>(ld28(in), ld28(in + 14)));)
template <bool K, bool RK> OP(F28MulsubBody, 56, 14, st28(out, f28_mulsub_body<K, RK>(ld28(in), ld28(in + 14), ld28(in + 28), ld28(in + 42)));)
OP(F28MulsubBodyDef, 56, 14, st28(out, f28_mulsub_body<>(ld28(in), ld28(in + 14), ld28(in + 28), ld28(in + 42)));)
template <bool K> OP(F28SqrBody, 14, 14, st28(out, f28_sqr_body<K>(ld28(in)));)
OP(F28SqrBodyDef, 14, 14, st28(out, f28_sqr_body<>(ld28(in)));)
template <bool K> OP(F28Sqr, 14, 14, st28(out, f28_sqr<K>(ld28(in)));)
OP(F28SqrDef, 14, 14, st28(out, f28_sqr<>(ld28(in)));)

// fp28.hpp linear operations, zero test, conversions, inversions, constants
OP(F28Normalize, 14, 14, F28 a = ld28(in); f28_normalize(a); st28(out, a);)
OP(F28Add, 28, 14, st28(out, f28_add(ld28(in), ld28(in + 14)));)
OP(F28Sub, 28, 14, st28(out, f28_sub(ld28(in), ld28(in + 14)));)
OP(F28SubSub2, 42, 14, st28(out, f28_sub_sub2(ld28(in), ld28(in + 14), ld28(in + 28)));)
OP(F28Neg, 14, 14, st28(out, f28_neg(ld28(in)));)
OP(F28Cneg, 15, 14, st28(out, f28_cneg(ld28(in), in[14] != 0));)
template <int K> OP(F28Shl, 14, 14, st28(out, f28_shl<K>(ld28(in)));)
OP(F28ProductIsZero, 14, 1, out[0] = f28_product_is_zero(ld28(in)) ? 1u : 0u;)
OP(F28FromStd, 12, 14, st28(out, f28_from_std(ldfe<FpCfg>(in)));)
OP(F28ToStd, 14, 12, stfe<FpCfg>(out, f28_to_std(ld28(in)));)
OP(F28CanonicalWords, 14, 12, uint32_t w[12]; f28_canonical_words(ld28(in), w); CPX_UNROLL for (int i = 0; i < 12; i++) out[i] = w[i];)
OP(F28FromWords, 12, 14, uint32_t w[12]; CPX_UNROLL for (int i = 0; i < 12; i++) w[i] = in[i]; st28(out, f28_from_words(w));)
OP(F28InvEuclid, 14, 14, st28(out, f28_inv_euclid(ld28(in)));)
OP(F28Inv, 14, 14, st28(out, f28_inv(ld28(in)));)
// the constants of F28Cfg as the code reads them: ONE, C_IN, C_OUT, C_INV, FOUR (the input word is ignored)
OP(F28Consts, 1, 70, st28(out, f28_one()); st28(out + 14, f28_const(F28Cfg::C_IN)); st28(out + 28, f28_const(F28Cfg::C_OUT));
   st28(out + 42, f28_const(F28Cfg::C_INV)); st28(out + 56, f28_const(F28Cfg::FOUR));)

// mont32.hpp for either field: fe_mul is the out-of-line register entry (fe_mul_regs12 / fe_mul_regs8)
template <class C> OP(FeMul, 2 * C::N, C::N, stfe<C>(out, fe_mul(ldfe<C>(in), ldfe<C>(in + C::N)));)
template <class C> OP(FeMulBody, 2 * C::N, C::N, stfe<C>(out, fe_mul_body<C>(ldfe<C>(in), ldfe<C>(in + C::N)));)
template <class C> OP(FeSqr, C::N, C::N, stfe<C>(out, fe_sqr(ldfe<C>(in)));)
template <class C> OP(FeAdd, 2 * C::N, C::N, stfe<C>(out, fe_add(ldfe<C>(in), ldfe<C>(in + C::N)));)
template <class C> OP(FeSub, 2 * C::N, C::N, stfe<C>(out, fe_sub(ldfe<C>(in), ldfe<C>(in + C::N)));)
template <class C> OP(FeNeg, C::N, C::N, stfe<C>(out, fe_neg(ldfe<C>(in)));)
template <class C> OP(FeDbl, C::N, C::N, stfe<C>(out, fe_dbl(ldfe<C>(in)));)
template <class C> OP(FeFromMont, C::N, C::N, stfe<C>(out, fe_from_mont(ldfe<C>(in)));)
template <class C> OP(FeToMont, C::N, C::N, stfe<C>(out, fe_to_mont(ldfe<C>(in)));)

// g1_28.hpp: every coordinate as 14 limbs (XYZZ: x, y, zz, zzz; Jacobian: x, y, z; affine: x, y)
template <bool INL, bool K, bool RK> OP(XyzzAddMixed, 84, 56, stxyzz(out, xyzz28_add_mixed_t<INL, K, RK>(ldxyzz(in), ldaff(in + 56)));)
OP(XyzzAddMixedDef, 84, 56, stxyzz(out, xyzz28_add_mixed(ldxyzz(in), ldaff(in + 56)));)           // t_acc_add_mixed
OP(XyzzAddMixedInlDef, 84, 56, stxyzz(out, t_acc_add_mixed_inl(ldxyzz(in), ldaff(in + 56)));)      // the bucket loops
OP(XyzzAdd, 112, 56, stxyzz(out, xyzz28_add(ldxyzz(in), ldxyzz(in + 56)));)
OP(XyzzDbl, 56, 56, stxyzz(out, xyzz28_dbl(ldxyzz(in)));)
OP(XyzzDblAffine, 28, 56, stxyzz(out, xyzz28_dbl_affine(ldaff(in)));)
OP(XyzzToJac, 56, 42, stjac(out, xyzz28_to_jac(ldxyzz(in)));)
OP(JacDbl, 42, 42, stjac(out, jac28_dbl(ldjac(in)));)
OP(JacAddMixed, 70, 42, stjac(out, jac28_add_mixed(ldjac(in), ldaff(in + 42)));)
OP(JacAdd, 84, 42, stjac(out, jac28_add(ldjac(in), ldjac(in + 42)));)

static const Entry TABLE[] = {
    entry<F28MulBody<false, false>>("f28_mul_body/0"), entry<F28MulBody<true, false>>("f28_mul_body/1"),
    entry<F28MulBody<true, true>>("f28_mul_body/2"), entry<F28MulBodyDef>("f28_mul_body/-1"),
    entry<F28Mul<false, false>>("f28_mul/0"), entry<F28Mul<true, false>>("f28_mul/1"),
    entry<F28Mul<true, true>>("f28_mul/2"), entry<F28MulDef>("f28_mul/-1"),
    entry<F28MulsubBody<false, false>>("f28_mulsub_body/0"), entry<F28MulsubBody<true, false>>("f28_mulsub_body/1"),
    entry<F28MulsubBody<true, true>>("f28_mulsub_body/2"), entry<F28MulsubBodyDef>("f28_mulsub_body/-1"),
    entry<F28SqrBody<false>>("f28_sqr_body/0"), entry<F28SqrBody<true>>("f28_sqr_body/2"), entry<F28SqrBodyDef>("f28_sqr_body/-1"),
    entry<F28Sqr<false>>("f28_sqr/0"), entry<F28Sqr<true>>("f28_sqr/2"), entry<F28SqrDef>("f28_sqr/-1"),
    entry<F28Normalize>("f28_normalize"), entry<F28Add>("f28_add"), entry<F28Sub>("f28_sub"), entry<F28SubSub2>("f28_sub_sub2"),
    entry<F28Neg>("f28_neg"), entry<F28Cneg>("f28_cneg"), entry<F28Shl<1>>("f28_shl/1"), entry<F28Shl<2>>("f28_shl/2"),
    entry<F28Shl<3>>("f28_shl/3"), entry<F28ProductIsZero>("f28_product_is_zero"), entry<F28FromStd>("f28_from_std"),
    entry<F28ToStd>("f28_to_std"), entry<F28CanonicalWords>("f28_canonical_words"), entry<F28FromWords>("f28_from_words"),
    entry<F28InvEuclid>("f28_inv_euclid"), entry<F28Inv>("f28_inv"), entry<F28Consts>("f28_consts"),
    entry<FeMul<FpCfg>>("fp_mul"), entry<FeMulBody<FpCfg>>("fp_mul_body"), entry<FeSqr<FpCfg>>("fp_sqr"), entry<FeAdd<FpCfg>>("fp_add"),
    entry<FeSub<FpCfg>>("fp_sub"), entry<FeNeg<FpCfg>>("fp_neg"), entry<FeDbl<FpCfg>>("fp_dbl"), entry<FeFromMont<FpCfg>>("fp_from_mont"),
    entry<FeToMont<FpCfg>>("fp_to_mont"),
    entry<FeMul<FrCfg>>("fr_mul"), entry<FeMulBody<FrCfg>>("fr_mul_body"), entry<FeSqr<FrCfg>>("fr_sqr"), entry<FeAdd<FrCfg>>("fr_add"),
    entry<FeSub<FrCfg>>("fr_sub"), entry<FeNeg<FrCfg>>("fr_neg"), entry<FeDbl<FrCfg>>("fr_dbl"), entry<FeFromMont<FrCfg>>("fr_from_mont"),
    entry<FeToMont<FrCfg>>("fr_to_mont"),
    // the mixed addition as the kernels instantiate it: xyzz28_add_mixed (<false>, t_acc_add_mixed) and t_acc_add_mixed_inl
    // (<true, F28_KARA, F28_REDC_KARA>); then every explicit choice of bodies for the inlined form
    entry<XyzzAddMixedDef>("xyzz28_add_mixed"), entry<XyzzAddMixedInlDef>("xyzz28_add_mixed_inl"),
    entry<XyzzAddMixed<true, true, true>>("xyzz28_add_mixed_t/1,1,1"), entry<XyzzAddMixed<true, true, false>>("xyzz28_add_mixed_t/1,1,0"),
    entry<XyzzAddMixed<true, false, false>>("xyzz28_add_mixed_t/1,0,0"), entry<XyzzAddMixed<false, false, false>>("xyzz28_add_mixed_t/0,0,0"),
    entry<XyzzAdd>("xyzz28_add"), entry<XyzzDbl>("xyzz28_dbl"), entry<XyzzDblAffine>("xyzz28_dbl_affine"), entry<XyzzToJac>("xyzz28_to_jac"),
    entry<JacDbl>("jac28_dbl"), entry<JacAddMixed>("jac28_add_mixed"), entry<JacAdd>("jac28_add"),
};

int main(int argc, char** argv) { return rows_main(argc, argv, TABLE); }
