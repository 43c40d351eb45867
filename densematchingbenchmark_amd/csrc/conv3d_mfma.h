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

// Launch plan of dmb_conv3d_k3_f32: WHICH kernel form and WHICH tile instantiation a launch runs, as one pure host function of the
// launch's description (conv3d_plan, conv3d.hip; dmb_conv3d_k3_plan returns it as an integer, tests/test_conv3d_plan_host.py).
// Plan code = (form << 8) | index:
//   CONV_SPLIT_K   index = variant (conv3d_sk.hip) + 4 at stride 2
//   CONV_S1_VEC    stride 1, 16-byte rows: index into S1Tiles32, or 4 + index into S1Tiles64
//   CONV_S1_FLAT   stride 1, flattened dword tiles: 0 / 1 = 32 output channels, TX 60 / 52; 2 / 3 = 64 output channels
//   CONV_S1_C128   stride 1, 128 output channels: index 0
//   CONV_S2        stride 2: S2_ROWS1 ... below
// (the development build's options force among these codes: it holds no instantiation of its own)
enum { CONV_SPLIT_K = 1, CONV_S1_VEC = 2, CONV_S1_FLAT = 3, CONV_S1_C128 = 4, CONV_S2 = 5 };
// stride-2 indices: the 64-channel tiles of the vector path (30 columns x 1 / 2 / 4 rows with the 8-byte epilogue, 22 columns x 4
// rows, 30 x 4 with the dword epilogue), then the dword-staged 30 x 4 tile per output width
enum { S2_ROWS1 = 0, S2_ROWS2 = 1, S2_ROWS4 = 2, S2_NARROW = 3, S2_ROWS4_DWORD = 4, S2_FLAT64 = 5, S2_FLAT32 = 6, S2_FLAT128 = 7 };
constexpr const char* CONV3D_UNSUPPORTED = "conv3d: output channels must be 32 or 64 (or 1: dmb_conv3d_k3_c1_f32), stride 1 or 2";

// csrc/conv3d_s1s2.hip: the full-grid stride-1 and stride-2 kernels behind dmb_conv3d_k3_f32.  conv3d_s1_plan / conv3d_s2_plan hold
// every choice among their tiles and their refusals (-> the plan code, or minus the DMB_E* code with its message in *why), after
// conv3d_plan has checked the arguments and tried the split-K form; conv3d_s1_run / conv3d_s2_run launch the planned instantiation
// and cannot decline.  Both take the same `relu` word: bits 8 .. 15 carry the development build's diagnostic bits (option 6).
int conv3d_s1_plan(const ConvDesc& d, const char** why);
int conv3d_s2_plan(const ConvDesc& d, const char** why);
int conv3d_s1_run(int plan, const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B,
                  int Ci, int D, int H, int W, int relu, hipStream_t st);
int conv3d_s2_run(int plan, const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B,
                  int Ci, int D, int H, int W, int relu, hipStream_t st);

}  // namespace dmb
