// g++ twin of curdleproofs_amd/csrc/shuffle_plan.hpp (tests/test_whisk_shuffle_batch_cpu.py): the index arithmetic the host and the
// kernels of the batched Whisk shuffle calls share, run on the CPU exactly as whisk.cpp and shuffle.hip call it.
#include <cstdint>
#include <cstddef>
#include "../../curdleproofs_amd/csrc/shuffle_plan.hpp"

using cpx::ShufflePlan;

extern "C" {

// sizes[0..4] = planes, points, upload_bytes, plane_points, fits
void emul_shuffle_sizes(uint32_t count, uint32_t ell, int verifier, uint64_t* sizes) {
  const ShufflePlan pl(count, ell, verifier != 0);
  sizes[0] = pl.planes();
  sizes[1] = pl.points();
  sizes[2] = pl.upload_bytes();
  sizes[3] = pl.plane_points();
  sizes[4] = pl.fits() ? 1 : 0;
}
// off[j] = byte offset of encoding j (the table whisk.cpp uploads); idx[(pl * count + i) * ell + e] = point_index; midx[i] = m_index
void emul_shuffle_offsets(uint32_t count, uint32_t ell, int verifier, uint64_t* off, uint64_t* idx, uint64_t* midx) {
  const ShufflePlan pl(count, ell, verifier != 0);
  for (size_t j = 0; j < pl.points(); j++) off[j] = pl.src_offset(j);
  for (uint32_t p = 0; p < pl.planes(); p++)
    for (uint32_t i = 0; i < count; i++)
      for (uint32_t e = 0; e < ell; e++) idx[((size_t)p * count + i) * ell + e] = pl.point_index(p, i, e);
  if (verifier)
    for (uint32_t i = 0; i < count; i++) midx[i] = pl.m_index(i);
}
// the fold as the host calls it (one pass) and as a wave of `lanes` lanes does (the or of the lanes' slices): bad[i], bad_lanes[i]
void emul_shuffle_fold(uint32_t count, uint32_t ell, int verifier, const uint8_t* status, uint32_t lanes, uint8_t* bad, uint8_t* bad_lanes) {
  const ShufflePlan pl(count, ell, verifier != 0);
  for (uint32_t i = 0; i < count; i++) {
    bad[i] = pl.item_bad(status, i, 0, 1) ? 1 : 0;
    bool any = false;
    for (uint32_t l = 0; l < lanes; l++) any |= pl.item_bad(status, i, l, lanes);
    bad_lanes[i] = any ? 1 : 0;
  }
}
// k_shuffle_status's placeholder rule on stand-in points (one word each): rows of a bad item become `gen`
void emul_shuffle_placeholder(uint32_t count, uint32_t ell, int verifier, const uint8_t* status, uint32_t* pts, uint32_t gen) {
  const ShufflePlan pl(count, ell, verifier != 0);
  for (uint32_t i = 0; i < count; i++) {
    const bool bad = pl.item_bad(status, i, 0, 1);
    for (uint32_t p = 0; p < pl.planes(); p++)
      for (uint32_t e = 0; e < ell; e++) pts[pl.point_index(p, i, e)] = cpx::shuffle_row_point(bad, pts[pl.point_index(p, i, e)], gen);
    if (verifier) pts[pl.m_index(i)] = cpx::shuffle_row_point(bad, pts[pl.m_index(i)], gen);
  }
}
// k_shuffle_gather on stand-in points: t / u dense [count][ell], zipped [count][ell][2]; src[g] = the element read
void emul_shuffle_gather(uint32_t count, uint32_t ell, const uint32_t* perm, const uint32_t* kr, const uint32_t* ks, uint32_t* t, uint32_t* u, uint32_t* zipped,
                         uint64_t* src) {
  const ShufflePlan pl(count, ell, false);
  for (size_t g = 0; g < pl.plane_points(); g++) {
    const uint32_t j = (uint32_t)(g % ell);
    const size_t s = g - j + pl.gather_src(perm[g], j);
    src[g] = s;
    t[pl.dense_dst(g)] = kr[s];
    u[pl.dense_dst(g)] = ks[s];
    zipped[pl.zip_dst(g, 0)] = kr[s];
    zipped[pl.zip_dst(g, 1)] = ks[s];
  }
}
}
