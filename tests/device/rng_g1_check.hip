// TEST-ONLY: the pieces of G1::rand (curdleproofs_amd/csrc/rng.hpp: rng_fp_accept, rng_g1_candidate; g1_28.hpp: g1_28_point_from_x,
// g1_28_clear_cofactor) on raw words, one source compiled twice:
//   g++ -x c++ ...                     -> the host twin: every operation in a plain loop over the rows
//   hipcc --offload-arch=gfx950 ...    -> the device program: every operation in a kernel of its own, one thread per row, 64-thread blocks
// tests/test_rng_g1_check_cpu.py and tests/test_gpu_rng_g1.py feed both the same rows (tests/rng_g1_cases.py) and compare the results with
// each other and with the Python model (tests/stdrng_g1_ref.py).  Nothing in curdleproofs_amd/ links it.
//
// The command line, the record format, the exit codes and the runner are those of check_harness.hpp; --list prints name, input words per
// row, output words per row.  A state travels as ten words (key[8], word_pos low, high), a field
// element as its twelve standard-form limbs (Montgomery, R = 2^384, least significant first), the identity as x = y = 0.
#define CHECK_PROG "rng_g1_check"
#include "check_harness.hpp"
#include "../../curdleproofs_amd/csrc/rng.hpp"
#include "../../curdleproofs_amd/csrc/g1_28.hpp"

using namespace cpx;

CPX_HD Fp fp_of(const uint32_t* w) {
  Fp a;
  for (int i = 0; i < 12; i++) a.v[i] = w[i];
  return a;
}
CPX_HD void fp_to(const Fp& a, uint32_t* w) {
  for (int i = 0; i < 12; i++) w[i] = a.v[i];
}

OP(FpAccept, 12, 13, uint32_t l[12]; for (int i = 0; i < 12; i++) l[i] = in[i]; out[12] = rng_fp_accept(l) ? 1u : 0u; for (int i = 0; i < 12; i++) out[i] = l[i];)
// state in; x, greatest, the position behind the token out
OP(G1Candidate, 10, 15, RngStream s(rng_state_from_words(in)); bool g; rng_g1_candidate(s, out, g); out[12] = g ? 1u : 0u; out[13] = (uint32_t)s.st.word_pos;
   out[14] = (uint32_t)(s.st.word_pos >> 32);)
// x (below p), greatest in; hit, x, y out (zero where there is no root)
OP(PointFromX, 13, 25, Aff28 p; const bool hit = g1_28_point_from_x(f28_from_std(fp_of(in)), in[12] != 0, &p); out[0] = hit ? 1u : 0u;
   for (int i = 1; i < 25; i++) out[i] = 0; if (hit) { fp_to(f28_to_std(p.x), out + 1); fp_to(f28_to_std(p.y), out + 13); })
// an affine point of E(Fp) in; affine([h] P) out
OP(ClearCofactor, 24, 24, Aff a; a.x = fp_of(in); a.y = fp_of(in + 12); const Jac28 q = g1_28_clear_cofactor(aff28_from_std(a));
   Aff r = Aff::identity(); if (!q.is_identity()) r = aff28_to_std(jac28_to_affine_with_zinv(q, f28_inv(q.z))); fp_to(r.x, out); fp_to(r.y, out + 12);)

static const Entry TABLE[] = {
    entry<FpAccept>("fp_accept"), entry<G1Candidate>("g1_candidate"), entry<PointFromX>("point_from_x"), entry<ClearCofactor>("clear_cofactor"),
};

int main(int argc, char** argv) { return rows_main(argc, argv, TABLE); }
