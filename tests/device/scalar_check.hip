// TEST-ONLY: every function of the scalar-side headers (glv.hpp, recode.hpp, gen_table.hpp, tracker_ladder.hpp, modinv30.hpp and the
// inversions, powers and compares of mont32.hpp that field_check.hip leaves out) on raw words, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row,
//                                         64-thread blocks, plain vector loads and stores
// tests/test_scalar_check_cpu.py and tests/test_gpu_scalar.py feed both the same rows (tests/scalar_cases.py) and compare the results
// with each other and with Python integers (tests/scalar_check_lib.py).  Nothing in curdleproofs_amd/ links it.
//
// The command line, the record format, the exit codes and the runner are those of check_harness.hpp; --list prints name, input words
// per row, output words per row.  Rows are u32 words; narrow digits (int8_t, int16_t, int) travel one per word, sign-extended.
#define CHECK_PROG "scalar_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/mont32.hpp"
#include "../../curdleproofs_amd/csrc/glv.hpp"
#include "../../curdleproofs_amd/csrc/recode.hpp"
#include "../../curdleproofs_amd/csrc/gen_table.hpp"
#include "../../curdleproofs_amd/csrc/tracker_ladder.hpp"
#include "../../curdleproofs_amd/csrc/modinv30.hpp"

using namespace cpx;

template <class C> CPX_HD Fe<C> ldfe(const uint32_t* w) {
  Fe<C> r;
  CPX_UNROLL for (int i = 0; i < C::N; i++) r.v[i] = w[i];
  return r;
}
template <class C> CPX_HD void stfe(uint32_t* w, const Fe<C>& a) {
  CPX_UNROLL for (int i = 0; i < C::N; i++) w[i] = a.v[i];
}
CPX_HD uint32_t sx(int d) { return (uint32_t)(int32_t)d; }   // a digit as one sign-extended word
CPX_HD void st_naf(uint32_t* w, const SmulNaf& o) {           // nz[0], nz[1], ng[0], ng[1]: the order of the struct
  for (int h = 0; h < 2; h++)
    for (int i = 0; i < 5; i++) {
      w[5 * h + i] = o.nz[h][i];
      w[10 + 5 * h + i] = o.ng[h][i];
    }
}

// glv.hpp
OP(GlvSplit, 8, 10, uint32_t nk, nt; glv_split(in, out, out + 4, nk, nt); out[8] = nk; out[9] = nt;)
OP(GlvBiasedBytes, 4, 4, glv_biased_bytes(in, out);)

// recode.hpp.  recode_signed16 as k_msm_accw calls it (the default stride) and with a stride of 3 into a buffer filled with 0x55: the
// 65th word counts the slots between the digits that still hold the fill (126 of 190)
OP(RecodeSigned16, 8, 64, int8_t d[64]; recode_signed16(in, d); for (int w = 0; w < 64; w++) out[w] = sx(d[w]);)
OP(RecodeSigned16Stride, 8, 65, int8_t d[190]; for (int i = 0; i < 190; i++) d[i] = 0x55; recode_signed16(in, d, 3); uint32_t kept = 0;
   for (int i = 0; i < 190; i++) if (i % 3) kept += d[i] == 0x55 ? 1u : 0u;
   for (int w = 0; w < 64; w++) out[w] = sx(d[3 * w]);
   out[64] = kept;)
OP(RecodeNaf, 8, 18, recode_naf(in, out, out + 9);)
OP(RecodeSmulGlv, 8, 20, SmulNaf o; recode_smul_glv(in, o); st_naf(out, o);)
// the digit stream of k_late_fix and the window slices of k_msm_fix<CB, NW>: every slice [w0, w0 + NW), w0 = 0, NW, 2 NW, ..., each by a
// call of its own as the waves of a task make it, the digits strided in a buffer of the kernels' digit type
template <int CB> OP(FixStream, 8, FixWin<CB>::W, FixDigitStream<CB> ds(in); for (int w = 0; w < FixWin<CB>::W; w++) out[w] = sx(ds.next());)
template <int CB> struct FixDigitT { typedef int16_t type; };
template <> struct FixDigitT<19> { typedef int32_t type; };
template <int CB, int NW> OP(FixWindows, 8, FixWin<CB>::W, typedef typename FixDigitT<CB>::type DT; static_assert(FixWin<CB>::W % NW == 0, "whole slices");
   for (int w0 = 0; w0 < FixWin<CB>::W; w0 += NW) {
     DT buf[3 * NW];
     for (int i = 0; i < 3 * NW; i++) buf[i] = 0;
     fix_window_digits<CB, NW>(in, w0, buf, 3);
     for (int j = 0; j < NW; j++) out[w0 + j] = sx(buf[3 * j]);
   })
OP(RecodeSignedNibblesBiased, 4, 4, recode_signed_nibbles_biased(in, out);)

// gen_table.hpp: the recoded scalar, and the pick (index, neg) of every (half, window): word 2 (16 half + w)
OP(GenRecode, 8, 10, GenDigits o; gen_recode(in, o); for (int h = 0; h < 2; h++) { for (int i = 0; i < 4; i++) out[4 * h + i] = o.bytes[h][i]; out[8 + h] = o.neg[h]; })
OP(GenPickAll, 8, 64, GenDigits o; gen_recode(in, o);
   for (int h = 0; h < 2; h++)
     for (int w = 0; w < GEN_WINDOWS; w++) {
       const GenPick pk = gen_pick(o, h, w);
       out[2 * (GEN_WINDOWS * h + w)] = sx(pk.index);
       out[2 * (GEN_WINDOWS * h + w) + 1] = pk.neg ? 1u : 0u;
     })

// tracker_ladder.hpp: the table entry of every step of one scalar; the steps of a pair of scalars (e[0], e[1] of step i at 2 i)
OP(GlvTableEntry, 8, TRACKER_LADDER_TOP + 1, SmulNaf o; recode_smul_glv(in, o); for (int i = 0; i <= TRACKER_LADDER_TOP; i++) out[i] = sx(glv_table_entry(o, i));)
OP(TrackerLadderStep, 16, 2 * (TRACKER_LADDER_TOP + 1), SmulNaf a; SmulNaf b; recode_smul_glv(in, a); recode_smul_glv(in + 8, b);
   for (int i = 0; i <= TRACKER_LADDER_TOP; i++) {
     const TrackerStep s = tracker_ladder_step(a, b, i);
     out[2 * i] = sx(s.e[0]);
     out[2 * i + 1] = sx(s.e[1]);
   })

// modinv30.hpp: one batch of 30 division steps (eta, f0, g0) -> (eta', u, v, q, r); the inversions on canonical words and on
// Montgomery residues
OP(ModInv30Divsteps, 3, 5, Trans2x2 t; out[0] = sx(modinv30_divsteps((int32_t)in[0], in[1], in[2], t)); out[1] = sx(t.u); out[2] = sx(t.v); out[3] = sx(t.q); out[4] = sx(t.r);)
OP(WordsInvModPDivsteps, 12, 12, words_inv_mod_p_divsteps(in, out);)
OP(WordsInvModRDivsteps, 8, 8, words_inv_divsteps<ModInv30FrCfg>(in, out);)
OP(FpInvDivsteps, 12, 12, stfe<FpCfg>(out, fe_inv_divsteps(ldfe<FpCfg>(in)));)
OP(FrInvDivsteps, 8, 8, stfe<FrCfg>(out, fr_inv_divsteps(ldfe<FrCfg>(in)));)

// mont32.hpp, what field_check.hip leaves out: Fermat inverse, power by an exponent of N words (the row's second operand), the binary
// Euclidean inversion, the raw compare
template <class C> OP(FeInv, C::N, C::N, stfe<C>(out, fe_inv(ldfe<C>(in)));)
template <class C> OP(FePow, 2 * C::N, C::N, stfe<C>(out, fe_pow(ldfe<C>(in), in + C::N, C::N));)
OP(WordsInvModP, 12, 12, words_inv_mod_p(in, out);)
OP(FpInvEuclid, 12, 12, stfe<FpCfg>(out, fe_inv_euclid(ldfe<FpCfg>(in)));)
template <class C> OP(FeRawGt, 2 * C::N, 1, out[0] = fe_raw_gt(ldfe<C>(in), ldfe<C>(in + C::N)) ? 1u : 0u;)

static const Entry TABLE[] = {
    entry<GlvSplit>("glv_split"), entry<GlvBiasedBytes>("glv_biased_bytes"),
    entry<RecodeSigned16>("recode_signed16"), entry<RecodeSigned16Stride>("recode_signed16/stride3"), entry<RecodeNaf>("recode_naf"),
    entry<RecodeSmulGlv>("recode_smul_glv"),
    // FixDigitStream<CB>: k_late_fix<8 / 16 / 19>;  fix_window_digits<CB, NW>: k_msm_fix<8, 16>, <8, 8>, <16, 16>, <16, 8>, <16, 4>,
    // <16, 2> (also k_msm_fix_tblw), <19, 7>
    entry<FixStream<8>>("fix_digit_stream/8"), entry<FixStream<16>>("fix_digit_stream/16"), entry<FixStream<19>>("fix_digit_stream/19"),
    entry<FixWindows<8, 16>>("fix_window_digits/8,16"), entry<FixWindows<8, 8>>("fix_window_digits/8,8"),
    entry<FixWindows<16, 16>>("fix_window_digits/16,16"), entry<FixWindows<16, 8>>("fix_window_digits/16,8"),
    entry<FixWindows<16, 4>>("fix_window_digits/16,4"), entry<FixWindows<16, 2>>("fix_window_digits/16,2"),
    entry<FixWindows<19, 7>>("fix_window_digits/19,7"),
    entry<RecodeSignedNibblesBiased>("recode_signed_nibbles_biased"),
    entry<GenRecode>("gen_recode"), entry<GenPickAll>("gen_pick"),
    entry<GlvTableEntry>("glv_table_entry"), entry<TrackerLadderStep>("tracker_ladder_step"),
    entry<ModInv30Divsteps>("modinv30_divsteps"), entry<WordsInvModPDivsteps>("words_inv_mod_p_divsteps"),
    entry<WordsInvModRDivsteps>("words_inv_mod_r_divsteps"), entry<FpInvDivsteps>("fp_inv_divsteps"), entry<FrInvDivsteps>("fr_inv_divsteps"),
    entry<FeInv<FpCfg>>("fp_inv"), entry<FeInv<FrCfg>>("fr_inv"), entry<FePow<FpCfg>>("fp_pow"), entry<FePow<FrCfg>>("fr_pow"),
    entry<WordsInvModP>("words_inv_mod_p"), entry<FpInvEuclid>("fp_inv_euclid"), entry<FeRawGt<FpCfg>>("fp_raw_gt"),
    entry<FeRawGt<FrCfg>>("fr_raw_gt"),
};

int main(int argc, char** argv) { return rows_main(argc, argv, TABLE); }
