// The tail of a DeepPruner refinement stage (disp_refinement/DeepPruner.py:36,40-42,87) in ONE launch:
//   y[B, 1, 2H, 2W] = up2(2 * relu(conv3x3(x[B, Ci, H, W], w[1, Ci, 3, 3]) + init[B, 1, H, W]))
// classify (3x3, Ci -> 1, no bias, padding 1), the residual add, the ReLU, the doubling and the half-pixel bilinear up-sampling by
// two.  As two launches (dmb_conv2d_f32 with one output channel, then dmb_bilinear_scale_f32) the 32-row MFMA tile multiplies 31
// rows of zeros and the refined map makes a round trip through memory; here it lives in LDS only.  Forward only.
//
// A direct FMA kernel, in the manner of dmb_conv2d_k5_small_f32: on gfx950 the FP32 MFMA runs at the vector FP32 rate, so with one
// output channel there is nothing to gain from it.
//   tile      a workgroup of 256 threads owns a 2 * RH_TW x 2 * RH_TH = 64 x 16 output tile of one batch item: the refined values
//             of the RH_TW x RH_TH input tile plus the one-pixel ring the interpolation reads, (RH_TW + 2) x (RH_TH + 2) = 340
//             values, one or two per thread.  A ring position outside the image is never read: the source indices of
//             bilinear_hp.h are clamped to the image, as align_corners=False clamps them.
//   input     all Ci channels of the (RH_TH + 4) x (RH_TW + 4) haloed tile in LDS, zero outside the image (27 KB at Ci = 16);
//             the weights are read at wave-uniform addresses.
//   sum       per refined value ONE ascending (ci, ky, kx) fmaf chain from 0, then + init, then max(., 0): a chain never depends
//             on the grid or the tile, so batch item i equals the same item run alone bit for bit.  A ring value is recomputed by
//             the neighbouring tile with the same chain, hence the same bits.
//   output    hp_blend(..., mult = 2) of bilinear_hp.h, the expression of dmb_bilinear_scale_f32: doubling is exact in FP32, so
//             up2(v) * 2 has the bits of up2(2 * v).  Each output element is written once; a wave stores one row of 64 floats.
#include "bilinear_hp.h"
#include "dmb_common.h"

namespace dmb {

constexpr int RH_TW = 32, RH_TH = 8, RH_MAXC = DMB_REFINE_HEAD_MAX_C;
constexpr int RH_RW = RH_TW + 2, RH_RH = RH_TH + 2;   // refined values: the tile and its ring
constexpr int RH_IW = RH_TW + 4, RH_IH = RH_TH + 4;   // staged input: the ring's own 3x3 halo
constexpr int RH_NT = 256;

__global__ __launch_bounds__(RH_NT) void refine_head_up2_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                const float* __restrict__ init, float* __restrict__ y, int Ci, int H,
                                                                int W, int tiles_x, float sh, float sw) {
#pragma clang fp contract(off)
  __shared__ float xt[RH_MAXC * RH_IH * RH_IW];
  __shared__ float rf[RH_RH * RH_RW];
  const int tid = threadIdx.x;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int b = blockIdx.y;
  const int x0 = tile_x * RH_TW, y0 = tile_y * RH_TH;   // the input tile's origin; the ring starts one before, the halo two
  const size_t HW = (size_t)H * W;
  const float* xb = x + (size_t)b * Ci * HW;
  for (int i = tid; i < Ci * RH_IH * RH_IW; i += RH_NT) {
    const int c = i / (RH_IH * RH_IW), rem = i - c * (RH_IH * RH_IW), row = rem / RH_IW, col = rem - row * RH_IW;
    const int gy = y0 + row - 2, gx = x0 + col - 2;
    xt[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[(size_t)c * HW + (size_t)gy * W + gx] : 0.f;
  }
  __syncthreads();
  // refined values r = tid and tid + RH_NT of the RH_RH x RH_RW ring tile; a thread without a second one repeats its first
  int rr[2], rc[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int r = tid + k * RH_NT;
    r = r < RH_RH * RH_RW ? r : tid;
    rr[k] = r / RH_RW;
    rc[k] = r - rr[k] * RH_RW;
  }
  float acc[2] = {0.f, 0.f};
  for (int c = 0; c < Ci; ++c) {
    const float* wp = w + c * 9;
    float wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = wp[t];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const float* xp = xt + (c * RH_IH + rr[k]) * RH_IW + rc[k];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) acc[k] = fmaf(xp[ky * RH_IW + kx], wv[ky * 3 + kx], acc[k]);
    }
  }
  const float* ib = init + (size_t)b * HW;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (k == 1 && tid + RH_NT >= RH_RH * RH_RW) break;
    const int gy = y0 + rr[k] - 1, gx = x0 + rc[k] - 1;
    float v = 0.f;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = fmaxf(acc[k] + ib[(size_t)gy * W + gx], 0.f);
    rf[rr[k] * RH_RW + rc[k]] = v;
  }
  __syncthreads();
  const int Ho = 2 * H, Wo = 2 * W;
  const int ox = 2 * x0 + (tid & 63);
  if (ox >= Wo) return;
  const HpTap tx = hp_tap(ox, W, sw);
  const int c0 = tx.i0 - (x0 - 1), c1 = tx.i1 - (x0 - 1);   // in [0, RH_RW): i0 >= x0 - 1 and i1 <= x0 + RH_TW for this tile's columns
  float* yb = y + (size_t)b * Ho * Wo;
#pragma unroll
  for (int j = 0; j < 2 * RH_TH / (RH_NT / 64); ++j) {
    const int oy = 2 * y0 + (tid >> 6) + j * (RH_NT / 64);
    if (oy >= Ho) break;
    const HpTap ty = hp_tap(oy, H, sh);
    const float* r0 = rf + (ty.i0 - (y0 - 1)) * RH_RW;
    const float* r1 = rf + (ty.i1 - (y0 - 1)) * RH_RW;
    yb[(size_t)oy * Wo + ox] = hp_blend(r0[c0], r0[c1], r1[c0], r1[c1], tx.l, ty.l, 2.f);
  }
}

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_refine_head_up2_f32(const float* x, const float* w, const float* init, float* y, int B, int Ci, int H, int W,
                                       void* stream) {
  if (!x || !w || !init || !y || B <= 0 || H <= 0 || W <= 0) return fail(DMB_EINVAL, "refine_head: bad argument");
  if (Ci < 1 || Ci > RH_MAXC) return fail(DMB_EUNSUPPORTED, "refine_head: 1 .. 16 input channels");
  const long long tiles = (long long)cdiv(W, RH_TW) * cdiv(H, RH_TH);
  // a batch item of x and of y stays below 2 GiB, so that every index inside an item fits 31 bits
  if (B > 65535 || tiles >= 0x7fffffffLL || 4LL * Ci * H * W >= 0x80000000LL || 16LL * H * W >= 0x80000000LL)
    return fail(DMB_EUNSUPPORTED, "refine_head: map too large");
  const int tiles_x = cdiv(W, RH_TW);
  hipLaunchKernelGGL(refine_head_up2_kernel, dim3((unsigned)tiles, B), dim3(RH_NT), 0, (hipStream_t)stream, x, w, init, y, Ci, H, W,
                     tiles_x, hp_scale(H, 2 * H), hp_scale(W, 2 * W));
  return launch_status("refine_head launch failed");
}
