// DeepPruner's cost processor (cost_processors/DeepPruner.py): the two pieces between the sampler and the aggregator that no
// other kernel of the library covers.  Forward only.
//
//   dmb_deeppruner_volume_f32   the raw cost volume of DeepPruner.py:192-195,204-208 in ONE pass: fast_cat_fms on per-pixel
//                               samples, the sample itself as a channel, and (stage "post") the two confidence-range feature maps
//                               repeated on every plane.  Every output element is written exactly once; the reference writes the
//                               volume up to three times (fast_cat_fms, torch.cat, torch.cat) and reads it twice.
//   dmb_conv2d_k5_small_f32     nn.Conv2d(Ci, Co, 5, stride 1, padding 2) on 1 .. 16 channels with a bias or a folded BatchNorm and
//                               an optional ReLU in the epilogue: the 1 -> 1 disparity convolutions and the N -> N feature
//                               convolutions of DeepPruner.py:69-84,180-188.  A direct FMA kernel: for so few output channels a
//                               32-row MFMA tile would mostly multiply zeros.
#include "dmb_common.h"
#include "warp_taps.h"

namespace dmb {

// ---------------------------------------------------------------------------------------------------------------------
// The raw cost volume.  HBM-write-bound, like warp_volume_kernel<WARP_CAT> whose channel loop this restates: one thread per
// (b, k, y, x), lanes along x so that every (b, channel, k) row is stored as W contiguous floats; the two columns of R a blend
// reads come from L1 / L2; the sample and feature channels are streaming copies (the feature maps are re-read once per plane,
// from L2).  No contraction anywhere in the sampler arithmetic (warp_taps.h; build.py compiles this file with -ffp-contract=off).
// ---------------------------------------------------------------------------------------------------------------------
#pragma clang fp contract(off)
__global__ __launch_bounds__(256) void deeppruner_volume_kernel(const float* __restrict__ L, const float* __restrict__ R,
                                                                const float* __restrict__ sample,
                                                                const float* __restrict__ min_feat,
                                                                const float* __restrict__ max_feat, float* __restrict__ out, int C,
                                                                int D, int H, int W, int P) {
  const int HW = H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int k = blockIdx.y, b = blockIdx.z;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  const float s = sample[((size_t)b * D + k) * HW + i];
  const WarpTaps t = warp_taps(-s, k, y, x, D, H, W);   // the warp uses -sample (cat_fms.py:74)
  const float* Lp = L + (size_t)b * C * HW + i;
  const float* Rp = R + (size_t)b * C * HW;
  const size_t DHW = (size_t)D * HW;
  const int OC = 2 * C + 1 + 2 * P;
  float* o = out + ((size_t)b * OC * D + k) * HW + i;
#pragma unroll 4
  for (int c = 0; c < C; ++c) {
    const float tv = warp_blend(t, Rp + (size_t)c * HW);
    const float lv = Lp[(size_t)c * HW] * (tv > 0.f ? 1.f : 0.f);   // reference features masked where the warped target <= 0
    __builtin_nontemporal_store(lv, o + (size_t)c * DHW);
    __builtin_nontemporal_store(tv, o + (size_t)(C + c) * DHW);
  }
  o += (size_t)2 * C * DHW;
  __builtin_nontemporal_store(s, o);                                  // DeepPruner.py:195
  o += DHW;
  if (P > 0) {                                                        // :204-208: [B, P, H, W] -> every plane k
    const float* mn = min_feat + (size_t)b * P * HW + i;
    const float* mx = max_feat + (size_t)b * P * HW + i;
#pragma unroll 4
    for (int p = 0; p < P; ++p) {
      __builtin_nontemporal_store(mn[(size_t)p * HW], o + (size_t)p * DHW);
      __builtin_nontemporal_store(mx[(size_t)p * HW], o + (size_t)(P + p) * DHW);
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The 5x5 convolution.  A workgroup of 128 threads owns a K5_TW x K5_TH = 32 x 8 output tile of one batch item and ALL output
// channels; lane = column (stores and LDS reads of a wave are two rows of 32 consecutive floats: coalesced, conflict-free for
// ds_read_b32 whose lane groups are the two halves of the wave), each thread two rows, so a weight read from LDS feeds two FMAs.
//   weights   all of them in LDS as [ci][ky][kx][COT] (COT = Co rounded up, the tail zero): the COT weights of a tap are one
//             or more 16-byte reads at an address the whole wave shares (a broadcast, no conflict);
//   input     a haloed (K5_TH + 4) x (K5_TW + 4) tile per input channel, K5_CC channels per stage, zero outside the image;
//   sum       per output ONE ascending (ci, ky, kx) fmaf chain from 0: the chunks are taken in ascending order and a thread's
//             chain never depends on the grid, so batch item i equals the same item run alone bit for bit.
// LDS: 16 * 25 * COT * 4 (at most 25.6 KB) + 8 * 12 * 36 * 4 = 13.8 KB: four workgroups per CU; 2 * COT accumulators, ten
// staged inputs and the 5 * COT weights of one filter row per thread.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int K5_TW = 32, K5_TH = 8, K5_CC = 8, K5_MAXC = 16;
constexpr int K5_IW = K5_TW + 4, K5_IH = K5_TH + 4;

template <int COT>
__global__ __launch_bounds__(128) void conv2d_k5_small_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ scale, const float* __restrict__ shift,
                                                              float* __restrict__ y, int Ci, int Co, int H, int W, int relu,
                                                              int tiles_x) {
  __shared__ __attribute__((aligned(16))) float wl[K5_MAXC * 25 * COT];
  __shared__ float xt[K5_CC * K5_IH * K5_IW];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  const int tile_y = blockIdx.x / tiles_x, tile_x = blockIdx.x - tile_y * tiles_x;
  const int b = blockIdx.y;
  const int x0 = tile_x * K5_TW, y0 = tile_y * K5_TH;
  for (int i = tid; i < Ci * 25 * COT; i += 128) {
    const int co = i % COT, q = i / COT, ci = q / 25, tap = q - ci * 25;
    wl[i] = co < Co ? w[((size_t)co * Ci + ci) * 25 + tap] : 0.f;
  }
  float acc[2][COT];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int j = 0; j < COT; ++j) acc[r][j] = 0.f;
  const float* xb = x + (size_t)b * Ci * H * W;
  for (int c0 = 0; c0 < Ci; c0 += K5_CC) {
    const int nc = min(K5_CC, Ci - c0);
    __syncthreads();   // the previous chunk has been read
    for (int i = tid; i < nc * K5_IH * K5_IW; i += 128) {
      const int c = i / (K5_IH * K5_IW), rem = i - c * (K5_IH * K5_IW), row = rem / K5_IW, col = rem - row * K5_IW;
      const int gy = y0 + row - 2, gx = x0 + col - 2;
      xt[i] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[((size_t)(c0 + c) * H + gy) * W + gx] : 0.f;
    }
    __syncthreads();   // (also: the weights are in place)
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
      const float* xp = xt + (c * K5_IH + 2 * ty) * K5_IW + tx;
      const float* wp = wl + (size_t)(c0 + c) * 25 * COT;
#pragma unroll 1
      for (int ky = 0; ky < 5; ++ky) {   // not unrolled: the weights of one filter row at a time, not all 25 * COT, are held in registers
        float v[2][5];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int kx = 0; kx < 5; ++kx) v[r][kx] = xp[(r + ky) * K5_IW + kx];
#pragma unroll
        for (int kx = 0; kx < 5; ++kx) {
          float wv[COT];
#pragma unroll
          for (int j = 0; j < COT; ++j) wv[j] = wp[(ky * 5 + kx) * COT + j];
#pragma unroll
          for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int j = 0; j < COT; ++j) acc[r][j] = fmaf(v[r][kx], wv[j], acc[r][j]);
        }
      }
    }
  }
  const int ox = x0 + tx;
  if (ox >= W) return;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int oy = y0 + 2 * ty + r;
    if (oy >= H) continue;
#pragma unroll
    for (int j = 0; j < COT; ++j) {
      if (j >= Co) continue;
      float o = acc[r][j];
      if (scale != nullptr) o = shift != nullptr ? fmaf(o, scale[j], shift[j]) : o * scale[j];
      else if (shift != nullptr) o = o + shift[j];
      if (relu) o = fmaxf(o, 0.f);
      y[(((size_t)b * Co + j) * H + oy) * W + ox] = o;
    }
  }
}

template <int COT>
static int launch_k5(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int Ci, int Co, int H,
                     int W, int relu, hipStream_t st) {
  const int tiles_x = cdiv(W, K5_TW), tiles_y = cdiv(H, K5_TH);
  hipLaunchKernelGGL((conv2d_k5_small_kernel<COT>), dim3(tiles_x * tiles_y, B), dim3(128), 0, st, x, w, scale, shift, y, Ci, Co, H,
                     W, relu, tiles_x);
  return launch_status("conv2d_k5_small launch failed");
}

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_deeppruner_volume_f32(const float* L, const float* R, const float* sample, const float* min_feat,
                                         const float* max_feat, float* out, int B, int C, int D, int H, int W, int P, void* stream) {
  if (!L || !R || !sample || !out || B <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || P < 0 || (P > 0 && (!min_feat || !max_feat)) ||
      (P == 0 && (min_feat || max_feat)))
    return fail(DMB_EINVAL, "deeppruner_volume: bad argument");
  if (D < 2 || H < 2 || W < 2)
    return fail(DMB_EUNSUPPORTED, "deeppruner_volume: the reference divides by (size - 1); D, H, W must be >= 2");
  if (P > DMB_PATCH_MATCH_MAX_SAMPLES) return fail(DMB_EUNSUPPORTED, "deeppruner_volume: more feature channels than the sampler makes");
  if ((long long)C * H * W >= 0x7fffffffLL || (long long)P * H * W >= 0x7fffffffLL || D > 65535 || B > 65535)
    return fail(DMB_EUNSUPPORTED, "deeppruner_volume: feature map too large");
  hipLaunchKernelGGL(deeppruner_volume_kernel, dim3(cdiv(H * W, 256), D, B), dim3(256), 0, (hipStream_t)stream, L, R, sample,
                     min_feat, max_feat, out, C, D, H, W, P);
  return launch_status("deeppruner_volume launch failed");
}

extern "C" int dmb_conv2d_k5_small_f32(const float* x, const float* w, const float* scale, const float* shift, float* y, int B,
                                       int Ci, int Co, int H, int W, int relu, void* stream) {
  if (!x || !w || !y || B <= 0 || Ci < 0 || Co < 0 || H <= 0 || W <= 0) return fail(DMB_EINVAL, "conv2d_k5_small: bad argument");
  if (Ci < 1 || Ci > K5_MAXC || Co < 1 || Co > K5_MAXC)
    return fail(DMB_EUNSUPPORTED, "conv2d_k5_small: 1 .. 16 input and output channels");
  const long long tiles = (long long)cdiv(W, K5_TW) * cdiv(H, K5_TH);
  if (B > 65535 || tiles >= 0x7fffffffLL || (long long)H * W >= 0x7fffffffLL)
    return fail(DMB_EUNSUPPORTED, "conv2d_k5_small: map too large");
  hipStream_t st = (hipStream_t)stream;
  if (Co == 1) return launch_k5<1>(x, w, scale, shift, y, B, Ci, Co, H, W, relu, st);
  if (Co <= 4) return launch_k5<4>(x, w, scale, shift, y, B, Ci, Co, H, W, relu, st);
  if (Co <= 8) return launch_k5<8>(x, w, scale, shift, y, B, Ci, Co, H, W, relu, st);
  if (Co <= 12) return launch_k5<12>(x, w, scale, shift, y, B, Ci, Co, H, W, relu, st);
  return launch_k5<16>(x, w, scale, shift, y, B, Ci, Co, H, W, relu, st);
}
