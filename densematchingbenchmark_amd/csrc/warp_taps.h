// The reference's tri-linear sampler on a (size - 1)-normalised grid with align_corners=False (layers/inverse_warp_3d.py:29-50 ->
// F.grid_sample), FP32 operation for operation: shared by the sample-based volume builders (warp_volume.hip) and the PatchMatch
// step (patch_match.hip), so that both warp exactly as the reference does.  Include only from translation units that build.py
// compiles with -ffp-contract=off.
#pragma once
#include "dmb_common.h"

namespace dmb {

struct WarpTaps {
  float w[8];      // tnw, tne, tsw, tse, bnw, bne, bsw, bse (top/bottom = plane, north/south = row, west/east = column)
  int off[4];      // nw, ne, sw, se offsets into a feature plane (0 when the tap is out of range)
  int xi[2], yi[2];   // west / east column, north / south row (0 when out of range)
  unsigned valid;  // bit t: tap t is inside the volume
};

// No contraction: every product and sum below rounds as the reference's does (build.py also compiles the including
// translation units with -ffp-contract=off).
#pragma clang fp contract(off)
__device__ inline WarpTaps warp_taps(float disp, int k, int y, int x, int D, int H, int W) {
  // inverse_warp_3d.py:33-43: mesh + disparity, then (g / (size - 1) * 2) - 1
  const float gd = ((((float)k / (float)(D - 1)) * 2.f) - 1.f);
  const float gh = ((((float)y / (float)(H - 1)) * 2.f) - 1.f);
  const float gw = (((((float)x + disp) / (float)(W - 1)) * 2.f) - 1.f);
  // grid_sample, align_corners=False: ((g + 1) * size - 1) / 2
  const float ix = ((((gw + 1.f) * (float)W) - 1.f) / 2.f);
  const float iy = ((((gh + 1.f) * (float)H) - 1.f) / 2.f);
  const float iz = ((((gd + 1.f) * (float)D) - 1.f) / 2.f);
  const float x0 = floorf(ix), y0 = floorf(iy), z0 = floorf(iz);
  const float x1 = (x0 + 1.f), y1 = (y0 + 1.f), z1 = (z0 + 1.f);
  const float wx0 = (x1 - ix), wx1 = (ix - x0);
  const float wy0 = (y1 - iy), wy1 = (iy - y0);
  const float wz0 = (z1 - iz), wz1 = (iz - z0);
  WarpTaps t;
  t.w[0] = ((wx0 * wy0) * wz0);
  t.w[1] = ((wx1 * wy0) * wz0);
  t.w[2] = ((wx0 * wy1) * wz0);
  t.w[3] = ((wx1 * wy1) * wz0);
  t.w[4] = ((wx0 * wy0) * wz1);
  t.w[5] = ((wx1 * wy0) * wz1);
  t.w[6] = ((wx0 * wy1) * wz1);
  t.w[7] = ((wx1 * wy1) * wz1);
  const bool vx0 = x0 >= 0.f && x0 < (float)W, vx1 = x1 >= 0.f && x1 < (float)W;   // false for NaN samples
  const bool vy0 = y0 >= 0.f && y0 < (float)H, vy1 = y1 >= 0.f && y1 < (float)H;
  const bool vz0 = z0 >= 0.f && z0 < (float)D, vz1 = z1 >= 0.f && z1 < (float)D;
  const int xi0 = vx0 ? (int)x0 : 0, xi1 = vx1 ? (int)x1 : 0, yi0 = vy0 ? (int)y0 : 0, yi1 = vy1 ? (int)y1 : 0;
  t.xi[0] = xi0;
  t.xi[1] = xi1;
  t.yi[0] = yi0;
  t.yi[1] = yi1;
  t.off[0] = yi0 * W + xi0;
  t.off[1] = yi0 * W + xi1;
  t.off[2] = yi1 * W + xi0;
  t.off[3] = yi1 * W + xi1;
  const unsigned q = (vx0 && vy0 ? 1u : 0u) | (vx1 && vy0 ? 2u : 0u) | (vx0 && vy1 ? 4u : 0u) | (vx1 && vy1 ? 8u : 0u);
  t.valid = (vz0 ? q : 0u) | (vz1 ? q << 4 : 0u);
  return t;
}

// the sampler's accumulation: out = 0; out += v * w for each tap inside the volume, in tap order
#pragma clang fp contract(off)
__device__ inline float warp_blend(const WarpTaps& t, const float* __restrict__ plane) {
  float v[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) v[q] = ((t.valid | (t.valid >> 4)) >> q & 1u) ? plane[t.off[q]] : 0.f;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (t.valid >> i & 1u) acc = (acc + (v[i & 3] * t.w[i]));
  return acc;
}

// warp_blend on four image values the caller has loaded already, v[q] = plane[t.off[q]] (an out-of-range tap's offset is 0, a
// valid address; its value is not used): the same accumulation, for callers that issue the loads of several planes at once
#pragma clang fp contract(off)
__device__ inline float warp_blend_loaded(const WarpTaps& t, const float v[4]) {
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i)
    if (t.valid >> i & 1u) acc = (acc + (v[i & 3] * t.w[i]));
  return acc;
}

}  // namespace dmb
