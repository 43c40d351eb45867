// What the translation units of the 3-D convolution family share (conv3d.hip: packers and dispatch; conv3d_s1s2.hip,
// deconv3d.hip: the MFMA kernels): the scalar epilogue and the entries through which dmb_conv3d_k3_f32 reaches its kernels.
#pragma once
#include "dmb_common.h"

namespace dmb {

// Epilogue shared by the three MFMA kernels: v = acc*scale + shift (+ residual) (relu) for the 16 accumulator
// registers of one 32x32 tile; `o` is the voxel offset inside one channel plane, `cstride` the channel stride.
// Residual loads are issued as one batch before the stores (one latency per tile instead of sixteen).
// relu: 0 none, 1 after the residual add (hourglass.py:67-81), 2 before it (GC-Net adds the skip to the activated
// output, aggregators/GCNet.py:108-116).  cvalid: channels >= cvalid are padding rows and are neither read nor written.
template <int VEC>
__device__ __forceinline__ void store_tile(const f32x16 (&a)[VEC], const float (&sc)[16], const float (&sh)[16],
                                           const float* __restrict__ rb, float* __restrict__ yb, int co0, int h,
                                           unsigned cstride, unsigned o, int relu, int cvalid = 1 << 30) {
  float rv[16][VEC];
  if (rb) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (co0 + cd_row(r, h) >= cvalid) {
        rv[r][0] = 0.f;
        rv[r][VEC - 1] = 0.f;
        continue;
      }
      const float* rp = rb + (size_t)(co0 + cd_row(r, h)) * cstride + o;
      if (VEC == 2) {
        const float2 t = *reinterpret_cast<const float2*>(rp);
        rv[r][0] = t.x;
        rv[r][VEC - 1] = t.y;
      } else {
        rv[r][0] = *rp;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float v[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
      v[e] = fmaf(a[e][r], sc[r], sh[r]);
      if (relu == 2) v[e] = fmaxf(v[e], 0.f);
      if (rb) v[e] += rv[r][e];
      if (relu == 1) v[e] = fmaxf(v[e], 0.f);
    }
    if (co0 + cd_row(r, h) >= cvalid) continue;
    float* yp = yb + (size_t)(co0 + cd_row(r, h)) * cstride + o;
    if (VEC == 2)
      *reinterpret_cast<float2*>(yp) = make_float2(v[0], v[VEC - 1]);
    else
      *yp = v[0];
  }
}

// csrc/conv3d_s1s2.hip: the full-grid stride-1 and stride-2 kernels behind dmb_conv3d_k3_f32, which has checked the arguments and tried
// the split-K form.  `relu` carries the development build's diagnostic bits above bit 7.  They return the launch's code, or
// conv3d_unsupported() for a channel count they do not build.
int conv3d_s1_run(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B, int Ci,
                  int Co, int D, int H, int W, int relu, bool out_small, hipStream_t st);
int conv3d_s2_run(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B, int Ci,
                  int Co, int D, int H, int W, int relu, hipStream_t st);
inline int conv3d_unsupported() {
  return fail(DMB_EUNSUPPORTED, "conv3d: output channels must be 32 or 64 (or 1: dmb_conv3d_k3_c1_f32), stride 1 or 2");
}

}  // namespace dmb
