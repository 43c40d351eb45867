// Half-pixel (align_corners=False) bilinear interpolation, as ATen's CPU path evaluates it: the ONE statement of the source index,
// the weights and the blend, shared by bilinear_hp_kernel (conv2d.hip, dmb_bilinear_scale_f32) and the fused refinement head
// (refine_head.hip), which must agree bit for bit.  src = max(scale * (dst + 0.5) - 0.5, 0), scale = in / out in FP32.
// src must round before the subtraction that gives the weight, so contraction is off INSIDE these functions (the pragma stays with
// their instructions when they are inlined into a translation unit that contracts elsewhere).
#pragma once
#include "dmb_common.h"

namespace dmb {

__host__ __device__ inline float hp_scale(int in, int out) { return (float)in / (float)out; }

struct HpTap {
  int i0, i1;   // the two source indices, both inside [0, in - 1]
  float l;      // the weight of i1; i0 has 1 - l
};

__device__ __forceinline__ HpTap hp_tap(int dst, int in, float scale) {
#pragma clang fp contract(off)
  const float s = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.f);
  HpTap t;
  t.i0 = (int)s;
  t.i0 = t.i0 > in - 1 ? in - 1 : t.i0;
  t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
  t.l = fminf(fmaxf(s - (float)t.i0, 0.f), 1.f);
  return t;
}

// p[y][x] are the four source values; the rows are blended along x first, then along y, then scaled.
__device__ __forceinline__ float hp_blend(float p00, float p01, float p10, float p11, float lx, float ly, float mult) {
#pragma clang fp contract(off)
  const float a0 = fmaf(p01, lx, p00 * (1.f - lx));
  const float a1 = fmaf(p11, lx, p10 * (1.f - lx));
  return fmaf(a1, ly, a0 * (1.f - ly)) * mult;
}

}  // namespace dmb
