// Device-resident protocol steps (protocol.hip): the Fiat-Shamir transcript and the scalar-field algebra between the MSM
// phases of CurdleproofsProof::{new,verify}, one wave per proof — shared declarations of the kernels and the host engine.
//
// With these kernels a whole batch advances through the protocol without the host: every phase's MSM requests read
// their scalars from device memory, the finalisation kernels leave the compressed results in a per-proof slot registry
// and the next step kernel hashes them and derives the next scalars.  Mirrors /root/reference/src/curdleproofs.rs:59-298,
// same_permutation_argument.rs, grand_product_argument.rs, inner_product_argument.rs, same_scalar_argument.rs,
// same_multiscalar_argument.rs (cited at the individual steps in protocol.hip).
#pragma once
#include <hip/hip_runtime.h>
#include "mont32.hpp"
#include "layout.hpp"

namespace cpx {

// ---- per-proof device state of the device-resident prover ----
// small scalars (Montgomery form), sc[p][SC_COUNT]; neighbours that one MSM request reads as a scalar vector are adjacent
enum {
  SC_BETA_SP = 0, SC_ALPHA_SP,          // B = A + alpha M + beta sum(G): request scalars [beta | alpha]
  SC_NEG_BETA_G_INV, SC_ALPHA_G,        // D = B - beta^-1 sum(G) + alpha sum(H): request scalars [-beta^-1 | alpha]
  SC_GPROD, SC_BETA_G, SC_BETA_G_INV, SC_RP, SC_ZIP, SC_ALPHA_I, SC_BETA_I, SC_ALPHA_S, SC_ALPHA_M,
  SC_ZK, SC_ZT, SC_ZU, SC_CFIN, SC_DFIN, SC_XFIN,
  SC_K_INV, SC_RK_K_INV,                // k^-1 and r_k k^-1: the side stream's scalars when R and S come from the tables (ProveDev::rs_tables)
  SC_COUNT = 24
};
// the names CPX_TRACE prints them under, for both provers (no name: an unused index)
static constexpr const char* kScNames[SC_COUNT] = {"beta_sp", "alpha_sp", "-beta_g_inv", "alpha_g", "gprod", "beta_g", "beta_g_inv", "r_p", "z_ip", "alpha_i", "beta_i",
                                                   "alpha_s", "alpha_m", "z_k", "z_t", "z_u", "c_final", "d_final", "x_final"};
// vectors of n scalars, vec[p][V_COUNT][n]
enum { V_APERM = 0, V_FACT, V_C, V_D, V_U, V_ZZ, V_ZZU, V_COUNT };

struct ProveDev {
  int ell, n, L, NS;              // NS = SlotMap(L).count()
  int rs_tables;                  // != 0: k_ps_aperm also leaves SC_K_INV, SC_RK_K_INV (prove_reqs.hpp prove_rs_tables)
  size_t psz;                     // proof size in bytes
  const uint32_t* perm;           // [B][ell]
  const Fr* k;                    // [B]
  const Fr* mbl;                  // [B][4]   vec_m_blinders
  const Fr* rnd;                  // [B][3n+9]
  uint64_t* tstate;               // [B][27]  transcript state (25 lanes, pos, pos_begin)
  const Fr* veca;                 // [B][ell]
  Fr* vec;                        // [B][V_COUNT][n]
  Fr* sc;                         // [B][SC_COUNT]
  uint8_t* slotcomp;              // [B][NS][48]  compressed bytes of every slot
  const uint8_t* inst_comp;       // [B][4 ell][48]  compressed R | S | T | U
  const uint8_t* mcomp;           // [B][48]
  Fr* rvec;                       // [B][4][n]  IPA round vectors: c | d | SG | SGp
  Fr* rvec2;                      // [B][2][n]  SameMSM round vectors: x | SM
  Fr* rgam;                       // [B][2]     gamma, gamma^-1
  Fr* rbeta;                      // [B]        IPA beta
  uint8_t* proofs;                // [B][psz]
  uint8_t crs_h_comp[48];         // compressed H (the blinder slots of vec_T / vec_U in the SameMSM transcript)
};

// ---- per-proof device state of the device-resident verifier ----
enum {   // vsc[p][VSC_COUNT]
  VSC_NEG_BETA_G_INV = 0, VSC_ALPHA_G,   // D request scalars
  VSC_ALPHA_SP, VSC_BETA_SP, VSC_GPROD, VSC_BETA_G, VSC_BETA_G_INV, VSC_RP, VSC_CFIN, VSC_DFIN, VSC_ZK, VSC_ZT, VSC_ZU, VSC_XFIN, VSC_COUNT = 16
};
struct VerifyDev {
  int ell, n, L, NS, NM;          // NM = misc points of the accumulated check (6 + 18 + 10 L)
  size_t psz;
  int rand_stride;                // 8 (per-proof verdicts) or 12 (fused batch: four extra weights for the SameScalar relations)
  const uint8_t* proofs;          // [B][psz]
  const Fr* rnd;                  // [B][rand_stride]
  uint64_t* tstate;               // [B][27]
  const Fr* veca;                 // [B][ell]
  Fr* vsc;                        // [B][VSC_COUNT]
  uint8_t* slotcomp;              // [B][NS][48]: D and A' (computed on the device) land here
  const uint8_t* inst_comp;       // [B][4 ell][48]
  const uint8_t* mcomp;           // [B][48]
  const uint8_t* status;          // [B][n_points]  decompression status of the proof points
  Fr* scal;                       // [B][4 ell + NM]: instance part | misc part of the accumulated check
  Fr* scal_crs;                   // [B][n]: its CRS part (G | Hvec)
  uint32_t* flags;                // [B]: bit 0 = undecodable (bad scalar / point encoding), bit 1 = structural rejection
  uint8_t crs_h_comp[48];
};

// ---- launchers (protocol.hip); B proofs, one wave each ----
void launch_ps_aperm(const ProveDev& d, int B, hipStream_t s);
void launch_ps_sameperm(const ProveDev& d, int B, hipStream_t s);
void launch_ps_gprod(const ProveDev& d, int B, hipStream_t s);
void launch_ps_ipa_setup(const ProveDev& d, int B, hipStream_t s);
void launch_ps_ipa_round(const ProveDev& d, int B, int j, hipStream_t s);
void launch_ps_smsm_setup(const ProveDev& d, int B, hipStream_t s);
void launch_ps_smsm_round(const ProveDev& d, int B, int j, hipStream_t s);
void launch_ps_serialize(const ProveDev& d, int B, hipStream_t s);
void launch_vs_prefix(const VerifyDev& d, int B, hipStream_t s);
void launch_vs_scalars(const VerifyDev& d, int B, hipStream_t s);
// d_out[g * n + i] = sum over the proofs p of group g of d_scal_crs[p * n + i]; NT groups of G proofs, the last one ragged: the groups of the
// grouped verifier (locate_plan.hpp), or G = B, NT = 1 for the CRS scalars of a fused batch
void launch_vs_crs_sum_groups(const Fr* d_scal_crs, int B, int n, int G, int NT, Fr* d_out, hipStream_t s);

}  // namespace cpx
