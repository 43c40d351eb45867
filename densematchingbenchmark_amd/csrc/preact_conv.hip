// AnyNet's small-channel convolutions and its stage arithmetic (include/dmb_hip.h, "AnyNet").
//
// preact_conv_kernel: one direct 3x3 (2-D) / 3x3x3 (3-D) convolution, padding 1, on the FP32 VALU.  AnyNet's layers have
// 1 .. 24 output channels, so MFMA tiles of 32 channels would stay mostly empty.  A workgroup of 256 threads owns a tile of
// 8 x 32 output pixels of one depth slice of one batch item and COT output channels; each thread computes one pixel for those
// COT channels.  The input tile plus its halo is staged in LDS, CK input channels at a time, with the prologue (2x2/2 max-pool,
// per-channel scale / shift, ReLU) applied once per staged element and only to in-bounds elements (padding stays 0).
// Each output is ONE ascending (ci, kz, ky, kx) fmaf chain from 0, whatever COT, the tile or the launch size: pair i of a batch
// equals the same pair run alone, bit for bit.
#include "dmb_common.h"

namespace dmb {
namespace {

constexpr int TW = 32, TH = 8, NT = TW * TH;
constexpr int CK = 8;                                       // input channels staged per round
constexpr int HALO_MAX = ((TH - 1) * 2 + 3) * ((TW - 1) * 2 + 3);   // 2-D stride 2: 17 x 65; 3-D stride 1 needs 3 x 10 x 34
static_assert(HALO_MAX >= 3 * (TH + 2) * (TW + 2), "3-D halo must fit");

struct PreactArgs {
  const float* x0;
  const float* x1;          // items [nb0, B) come from x1 (NULL: all from x0)
  const float* w;           // [Co, Ci, KD, 3, 3]
  const float* pscale;      // prologue affine (NULL: none)
  const float* pshift;
  const float* escale;      // epilogue: escale NULL and eshift set = bias
  const float* eshift;
  const float* res;         // [B, Co, Ho, Wo]
  float* y0;
  float* y1;                // gate mode: G2, G3
  float* y2;
  int nb0, Ci, Co, P;
  int D, H, W;              // raw input sizes
  int Hc, Wc;               // conv input sizes (after pooling)
  int Ho, Wo;
  int in_ctot, in_coff, out_ctot, out_coff;
  int tiles_x, tiles_y;
};

template <int KD, int S, int COT, bool POOL, bool GATE>
__global__ __launch_bounds__(NT) void preact_conv_kernel(PreactArgs a, int flags) {
  __shared__ float tile[CK * HALO_MAX];
  constexpr int HH = (TH - 1) * S + 3, HW = (TW - 1) * S + 3, HALO = KD * HH * HW;
  const int tid = threadIdx.x;
  const int bx = blockIdx.x % a.tiles_x, by = (blockIdx.x / a.tiles_x) % a.tiles_y, oz = blockIdx.x / (a.tiles_x * a.tiles_y);
  const int g = blockIdx.y, b = blockIdx.z;
  const int tx = tid % TW, ty = tid / TW;
  const int ox = bx * TW + tx, oy = by * TH + ty;
  const int D = a.D;
  const size_t plane = (size_t)a.H * a.W, item = (size_t)a.in_ctot * D * plane;
  const float* xb = (a.x1 != nullptr && b >= a.nb0) ? a.x1 + (size_t)(b - a.nb0) * item : a.x0 + (size_t)b * item;
  xb += (size_t)a.in_coff * D * plane;
  const bool prelu = (flags & DMB_PREACT_RELU_IN) != 0;
  const int y0 = by * TH * S - 1, x0 = bx * TW * S - 1, z0 = oz - (KD / 2);

  int co[COT];
#pragma unroll
  for (int j = 0; j < COT; ++j) co[j] = GATE ? j * a.P + g : g * COT + j;
  float acc[COT];
#pragma unroll
  for (int j = 0; j < COT; ++j) acc[j] = 0.f;

  for (int c0 = 0; c0 < a.Ci; c0 += CK) {
    const int nc = min(CK, a.Ci - c0);
    __syncthreads();
    for (int i = tid; i < nc * HALO; i += NT) {
      const int c = i / HALO, r = i - c * HALO;
      const int hz = r / (HH * HW), hy = (r / HW) % HH, hx = r % HW;
      const int z = z0 + hz, yy = y0 + hy, xx = x0 + hx;
      float v = 0.f;
      if (z >= 0 && z < D && yy >= 0 && yy < a.Hc && xx >= 0 && xx < a.Wc) {
        const float* p = xb + ((size_t)(c0 + c) * D + z) * plane;
        if (POOL) {
          const float* q = p + (size_t)(2 * yy) * a.W + 2 * xx;
          v = fmaxf(fmaxf(q[0], q[1]), fmaxf(q[a.W], q[a.W + 1]));
        } else {
          v = p[(size_t)yy * a.W + xx];
        }
        if (a.pscale != nullptr) v = fmaf(v, a.pscale[c0 + c], a.pshift[c0 + c]);
        if (prelu) v = fmaxf(v, 0.f);
      }
      tile[i] = v;
    }
    __syncthreads();
    for (int c = 0; c < nc; ++c) {
      const float* t = tile + c * HALO + (ty * S) * HW + tx * S;
#pragma unroll
      for (int kz = 0; kz < KD; ++kz) {
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
#pragma unroll
          for (int kx = 0; kx < 3; ++kx) {
            const float v = t[(kz * HH + ky) * HW + kx];
            const int tap = (kz * 3 + ky) * 3 + kx;
#pragma unroll
            for (int j = 0; j < COT; ++j) {
              if (co[j] < a.Co) acc[j] = fmaf(a.w[((size_t)co[j] * a.Ci + c0 + c) * (KD * 9) + tap], v, acc[j]);
            }
          }
        }
      }
    }
  }
  if (ox >= a.Wo || oy >= a.Ho) return;
  const size_t opix = ((size_t)oz * a.Ho + oy) * a.Wo + ox, oplane = (size_t)D * a.Ho * a.Wo;
#pragma unroll
  for (int j = 0; j < COT; ++j) {
    if (co[j] >= a.Co) continue;
    float v = acc[j];
    if (a.escale != nullptr) v = fmaf(v, a.escale[co[j]], a.eshift[co[j]]);
    else if (a.eshift != nullptr) v = v + a.eshift[co[j]];
    if (flags & DMB_PREACT_RELU_OUT) v = fmaxf(v, 0.f);
    if (a.res != nullptr) v = fmaxf(v + a.res[((size_t)b * a.Co + co[j]) * oplane + opix], 0.f);
    acc[j] = v;
  }
  if (GATE) {
    // disp_refinement/AnyNet.py:75-78: sum = (|G1| + |G2|) + |G3|; G_k / (sum + 1e-8), IEEE division
    const float s = (fabsf(acc[0]) + fabsf(acc[1])) + fabsf(acc[2]);
    const float d = s + 1e-8f;
    const size_t o = ((size_t)b * a.P + g) * oplane + opix;
    a.y0[o] = acc[0] / d;
    a.y1[o] = acc[1] / d;
    a.y2[o] = acc[2] / d;
    return;
  }
#pragma unroll
  for (int j = 0; j < COT; ++j) {
    if (co[j] < a.Co) a.y0[((size_t)b * a.out_ctot + a.out_coff + co[j]) * oplane + opix] = acc[j];
  }
}

template <int KD, int S, int COT, bool POOL, bool GATE>
int launch_preact(const PreactArgs& a, int flags, int B, int tiles_z, int groups, hipStream_t st) {
  const long long nx = (long long)a.tiles_x * a.tiles_y * tiles_z;
  if (nx > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "preact_conv: grid too large");
  hipLaunchKernelGGL((preact_conv_kernel<KD, S, COT, POOL, GATE>), dim3((unsigned)nx, groups, B), dim3(NT), 0, st, a, flags);
  return launch_status("preact_conv launch failed");
}

template <int KD, int S, bool POOL>
int dispatch_cot(const PreactArgs& a, int flags, int B, int tiles_z, int cot, hipStream_t st) {
  const int groups = (a.Co + cot - 1) / cot;
  switch (cot) {
    case 8: return launch_preact<KD, S, 8, POOL, false>(a, flags, B, tiles_z, groups, st);
    case 4: return launch_preact<KD, S, 4, POOL, false>(a, flags, B, tiles_z, groups, st);
    case 2: return launch_preact<KD, S, 2, POOL, false>(a, flags, B, tiles_z, groups, st);
    default: return launch_preact<KD, S, 1, POOL, false>(a, flags, B, tiles_z, groups, st);
  }
}

// Work split (DESIGN §4b's estimate): rounds of the chip times the chain length of a thread.  A round holds 4 workgroups of
// 256 threads per CU (each workgroup stages at most 35 KiB of LDS); a thread's chain is COT * Ci * taps fmaf.  The widest
// split within 1 % of the best estimate wins (fewer re-stagings of the same input tile).
int choose_cot(long long tiles, int Co, int chain) {
  const long long slots = 4LL * num_cus();
  double t[4], t_min = 0;
  for (int k = 0; k < 4; ++k) {
    const int cot = 1 << k;
    const long long wgs = tiles * ((Co + cot - 1) / cot);
    t[k] = (double)((wgs + slots - 1) / slots) * cot * chain;
    if (k == 0 || t[k] < t_min) t_min = t[k];
  }
  int best = 1;
  for (int k = 1; k < 4 && (1 << k) < 2 * Co; ++k)
    if (t[k] <= t_min * 1.01) best = 1 << k;
  return best;
}

// --------------------------------------------------------------------------------------------------------------- stage maps
// F.interpolate(mode='bilinear', align_corners=False) of f(p) evaluated per tap, in the arithmetic of conv2d.hip's
// bilinear_hp_kernel (ATen's source index max(scale * (dst + 0.5) - 0.5, 0), scale = in / out in FP32).
template <class F>
__device__ inline float hp_bilinear(const float* p, int Hi, int Wi, int Ho, int Wo, int yo, int xo, F f) {
#pragma clang fp contract(off)
  const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
  const float sy = fmaxf(sh * ((float)yo + 0.5f) - 0.5f, 0.f), sx = fmaxf(sw * ((float)xo + 0.5f) - 0.5f, 0.f);
  int y0 = (int)sy, x0 = (int)sx;
  y0 = y0 > Hi - 1 ? Hi - 1 : y0;
  x0 = x0 > Wi - 1 ? Wi - 1 : x0;
  const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
  float ly = sy - (float)y0, lx = sx - (float)x0;
  ly = fminf(fmaxf(ly, 0.f), 1.f);
  lx = fminf(fmaxf(lx, 0.f), 1.f);
  const float a0 = fmaf(f(p[(size_t)y0 * Wi + x1]), lx, f(p[(size_t)y0 * Wi + x0]) * (1.f - lx));
  const float a1 = fmaf(f(p[(size_t)y1 * Wi + x1]), lx, f(p[(size_t)y1 * Wi + x0]) * (1.f - lx));
  return fmaf(a1, ly, a0 * (1.f - ly));
}

__global__ __launch_bounds__(256) void stage_samples_kernel(const float* __restrict__ low, const float* __restrict__ lin,
                                                            float* __restrict__ up, float* __restrict__ samples, int h, int w,
                                                            int H, int W, int D, float scale) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= H * W) return;
  const int yo = i / W, xo = i % W;
  const float u = hp_bilinear(low + (size_t)b * h * w, h, w, H, W, yo, xo, [=](float v) { return v * scale; });
  up[(size_t)b * H * W + i] = u;
  if (samples != nullptr)
    for (int k = 0; k < D; ++k) samples[((size_t)b * D + k) * H * W + i] = lin[k] + u;
}

__global__ __launch_bounds__(256) void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ c,
                                                  long long n) {
  const long long i = blockIdx.x * 256LL + threadIdx.x;
  if (i < n) c[i] = a[i] + b[i];
}

struct FinalMaps {
  const float* d[4];
  int h[4], w[4];
};

__global__ __launch_bounds__(256) void final_maps_kernel(FinalMaps m, float* __restrict__ out, int B, int H, int W) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= H * W) return;
  const int yo = i / W, xo = i % W;
  const float Wf = (float)W;
  const size_t map = (size_t)B * H * W, o = (size_t)b * H * W + i;
  float u[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float wf = (float)m.w[k];
    // models/AnyNet.py:118: F.interpolate(d * W / d.shape[-1]) -- (d * W) / w, two roundings
    u[k] = hp_bilinear(m.d[k] + (size_t)b * m.h[k] * m.w[k], m.h[k], m.w[k], H, W, yo, xo, [=](float v) { return (v * Wf) / wf; });
    out[k * map + o] = u[k];
  }
#pragma unroll
  for (int k = 1; k < 4; ++k) out[(3 + k) * map + o] = u[k - 1] - u[k];   // :137-140
}

}  // namespace
}  // namespace dmb

using namespace dmb;

extern "C" int dmb_preact_conv_f32(const float* x, const float* x2, int B2, const float* w, const float* pre_scale,
                                   const float* pre_shift, const float* post_scale, const float* post_shift,
                                   const float* residual, float* y, float* y2, float* y3, int B, int Ci, int Co, int D, int H,
                                   int W, int ndim, int stride, int flags, int in_channels_total, int in_ch_offset,
                                   int out_channels_total, int out_ch_offset, void* stream) {
  const bool pool = (flags & DMB_PREACT_POOL) != 0, gate = (flags & DMB_PREACT_GATE) != 0;
  if (!x || !w || !y || B <= 0 || B > 65535 || Ci <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0 || in_ch_offset < 0 ||
      in_ch_offset + Ci > in_channels_total || (pre_scale == nullptr) != (pre_shift == nullptr) ||
      (post_scale != nullptr && post_shift == nullptr) || (x2 != nullptr && (B2 < 0 || B2 > B)))
    return fail(DMB_EINVAL, "preact_conv: bad argument");
  if (Ci > DMB_PREACT_MAX_CI || Co > DMB_PREACT_MAX_CO || (ndim != 2 && ndim != 3) || (stride != 1 && stride != 2) ||
      (ndim == 3 && (stride != 1 || pool)) || (ndim == 2 && D != 1) || (flags & ~0xf) != 0)
    return fail(DMB_EUNSUPPORTED, "preact_conv: Ci <= 64, Co <= 32, kernel 3 / padding 1; stride 2 and pooling 2-D only");
  const int Hc = pool ? H / 2 : H, Wc = pool ? W / 2 : W;
  if (Hc <= 0 || Wc <= 0) return fail(DMB_EINVAL, "preact_conv: nothing left after pooling");
  PreactArgs a{};
  a.x0 = x;
  a.x1 = x2;
  a.nb0 = x2 ? B2 : B;
  a.w = w;
  a.pscale = pre_scale;
  a.pshift = pre_shift;
  a.escale = post_scale;
  a.eshift = post_shift;
  a.res = residual;
  a.y0 = y;
  a.y1 = y2;
  a.y2 = y3;
  a.Ci = Ci;
  a.Co = Co;
  a.D = D;
  a.H = H;
  a.W = W;
  a.Hc = Hc;
  a.Wc = Wc;
  a.Ho = (Hc - 1) / stride + 1;
  a.Wo = (Wc - 1) / stride + 1;
  a.in_ctot = in_channels_total;
  a.in_coff = in_ch_offset;
  a.out_ctot = out_channels_total;
  a.out_coff = out_ch_offset;
  a.tiles_x = (a.Wo + TW - 1) / TW;
  a.tiles_y = (a.Ho + TH - 1) / TH;
  hipStream_t st = (hipStream_t)stream;
  if (gate) {
    // the 3P-channel guidance conv (disp_refinement/AnyNet.py:68-78): group g = channel p of G1, G2 and G3; out [B, P, Ho, Wo] x 3
    if (Co % 3 != 0 || !y2 || !y3 || residual || out_ch_offset != 0 || out_channels_total != Co / 3 || ndim != 2 || pool)
      return fail(DMB_EINVAL, "preact_conv: gate normalisation takes a 2-D 3P-channel conv into three [B, P, H, W] tensors");
    a.P = Co / 3;
    if (stride == 1) return launch_preact<1, 1, 3, false, true>(a, flags, B, 1, a.P, st);
    return launch_preact<1, 2, 3, false, true>(a, flags, B, 1, a.P, st);
  }
  if (out_ch_offset < 0 || out_ch_offset + Co > out_channels_total || (residual && out_channels_total != Co))
    return fail(DMB_EINVAL, "preact_conv: output window");
  const long long tiles = (long long)a.tiles_x * a.tiles_y * D * B;
  const int cot = choose_cot(tiles, Co, Ci * (ndim == 3 ? 27 : 9));
  if (ndim == 3) return dispatch_cot<3, 1, false>(a, flags, B, D, cot, st);
  if (stride == 1) return pool ? dispatch_cot<1, 1, true>(a, flags, B, 1, cot, st) : dispatch_cot<1, 1, false>(a, flags, B, 1, cot, st);
  return pool ? dispatch_cot<1, 2, true>(a, flags, B, 1, cot, st) : dispatch_cot<1, 2, false>(a, flags, B, 1, cot, st);
}

extern "C" int dmb_anynet_stage_samples_f32(const float* low, const float* lin, float* up, float* samples, int B, int h, int w,
                                            int H, int W, int D, float scale, void* stream) {
  if (!low || !up || B <= 0 || B > 65535 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || (samples && (!lin || D <= 0)))
    return fail(DMB_EINVAL, "anynet_stage_samples: bad argument");
  hipLaunchKernelGGL(stage_samples_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, low, lin, up, samples,
                     h, w, H, W, samples ? D : 0, scale);
  return launch_status("anynet_stage_samples launch failed");
}

extern "C" int dmb_add_f32(const float* a, const float* b, float* c, long long n, void* stream) {
  if (!a || !b || !c || n <= 0) return fail(DMB_EINVAL, "add: bad argument");
  hipLaunchKernelGGL(add_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a, b, c, n);
  return launch_status("add launch failed");
}

extern "C" int dmb_anynet_final_maps_f32(const float* d0, const float* d1, const float* d2, const float* d3, const int* h_host,
                                         const int* w_host, float* out, int B, int H, int W, void* stream) {
  if (!d0 || !d1 || !d2 || !d3 || !h_host || !w_host || !out || B <= 0 || B > 65535 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "anynet_final_maps: bad argument");
  FinalMaps m;
  m.d[0] = d0;
  m.d[1] = d1;
  m.d[2] = d2;
  m.d[3] = d3;
  for (int k = 0; k < 4; ++k) {
    if (h_host[k] <= 0 || w_host[k] <= 0) return fail(DMB_EINVAL, "anynet_final_maps: bad map size");
    m.h[k] = h_host[k];
    m.w[k] = w_host[k];
  }
  hipLaunchKernelGGL(final_maps_kernel, dim3((H * W + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, m, out, B, H, W);
  return launch_status("anynet_final_maps launch failed");
}
