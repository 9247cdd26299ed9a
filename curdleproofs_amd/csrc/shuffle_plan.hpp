// Index arithmetic of the batched Whisk shuffle calls (whisk.cpp, shuffle.hip) — plain integers, no HIP: one definition for the host
// that builds the decoder's offset table, the kernels that read the decoded planes, and the g++ twin tests/host_emul/shuffle_plan_emul.cpp.
//
// The bytes of one call lie in one device buffer: pre trackers [count][ell][96] | post trackers [count][ell][96] | M [count][48]
// (verifier form; the prover form holds the pre trackers only).  The decoder reads them plane-major, so that every family of points
// comes out as one dense [count][ell] array: r_G of the pre trackers (vec_R), their k_r_G (vec_S), r_G and k_r_G of the post trackers
// (vec_T, vec_U), and behind them the count commitments M.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mont32.hpp"

namespace cpx {

enum { SHP_R = 0, SHP_S, SHP_T, SHP_U };   // planes of the decoded points

struct ShufflePlan {
  uint32_t count, ell;
  uint32_t verifier;   // 1: pre | post | M (4 planes + M), 0: pre only (2 planes)
  CPX_HD ShufflePlan(size_t count_, size_t ell_, bool verifier_) : count((uint32_t)count_), ell((uint32_t)ell_), verifier(verifier_ ? 1u : 0u) {}
  CPX_HD uint32_t planes() const { return verifier ? 4u : 2u; }
  CPX_HD size_t plane_points() const { return (size_t)count * ell; }
  CPX_HD size_t points() const { return planes() * plane_points() + (verifier ? count : 0u); }   // encodings the decoder reads
  CPX_HD size_t tracker_bytes() const { return plane_points() * 96; }                            // one side's trackers
  CPX_HD size_t upload_bytes() const { return verifier ? 2 * tracker_bytes() + (size_t)count * 48 : tracker_bytes(); }
  // the 32-bit byte offsets and int grids of the kernels behind this plan
  CPX_HD bool fits() const { return ell != 0 && (uint64_t)count * ell < ((uint64_t)1 << 30) / 4 && (uint64_t)count * (2 * (uint64_t)ell * 96 + 48) < ((uint64_t)1 << 32); }
  // decoded point e of item i in plane pl; M of item i
  CPX_HD size_t point_index(uint32_t pl, uint32_t i, uint32_t e) const { return pl * plane_points() + (size_t)i * ell + e; }
  CPX_HD size_t m_index(uint32_t i) const { return 4 * plane_points() + i; }
  // byte offset of encoding j < points() inside the uploaded bytes
  CPX_HD size_t src_offset(size_t j) const {
    const size_t pp = plane_points();
    if (j >= 4 * pp) return 2 * tracker_bytes() + (j - 4 * pp) * 48;
    const size_t pl = j / pp, r = j % pp;
    return (pl >> 1) * tracker_bytes() + r * 96 + (pl & 1) * 48;
  }
  // Status fold: true iff one of the statuses `first, first + step, ...` among the item's planes() * ell (+ 1) points is non-zero.
  // The host and the twin pass (0, 1); lane l of the wave that owns the item passes (l, 64) and the wave ors the answers.
  CPX_HD bool item_bad(const uint8_t* status, uint32_t i, uint32_t first, uint32_t step) const {
    const uint32_t per = planes() * ell + verifier;
    bool bad = false;
    for (uint32_t t = first; t < per; t += step) {
      const size_t j = t < planes() * ell ? point_index(t / ell, i, t % ell) : m_index(i);
      bad |= status[j] != 0;
    }
    return bad;
  }
  // Gather T[i][j] = (k R)[i][perm[i][j]]: the source column.  An entry that is no index of the row (the host refuses such a call
  // before anything is launched) reads the row's own column j: the kernel stays inside its buffers whatever `perm` holds.
  CPX_HD uint32_t gather_src(uint32_t perm_entry, uint32_t j) const { return perm_entry < ell ? perm_entry : j; }
  // where element g = i * ell + j goes: the dense T / U arrays, and the interleaved (T_j, U_j) order of the post trackers
  CPX_HD size_t dense_dst(size_t g) const { return g; }
  CPX_HD size_t zip_dst(size_t g, uint32_t u) const { return 2 * g + u; }
};

// Placeholder rule: an item with an undecodable point keeps its place in the batch as a well-formed instance whose every point is
// the generator; its own result is overwritten afterwards.
template <class P> CPX_HD P shuffle_row_point(bool item_is_bad, const P& decoded, const P& generator) { return item_is_bad ? generator : decoded; }

}  // namespace cpx
