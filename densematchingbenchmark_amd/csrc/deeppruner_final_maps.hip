// The output tail of the DeepPruner model (models/DeepPruner.py:82-94,115) in ONE launch: every map brought to the image size and
// the two range residuals.  With up(d) = F.interpolate((d * W) / w_d, (H, W), bilinear, align_corners=False):
//   out[k]     = up(d_k), k < K          the refinement's list, better first; D = up(d_{K-1}) is the processor's own disparity
//   out[K]     = (Mn * W) / W            Mn = up(min_disparity): the reference interpolates the full-size map a second time; a
//   out[K + 1] = (Mx * W) / W            same-size half-pixel interpolation is the identity, the scaling is not
//   out[K + 2] = |D - Mn|                from the un-rescaled Mn and Mx (:115)
//   out[K + 3] = |Mx - D|
// As launches of the library this is K + 2 dmb_bilinear_scale_f32 with their K + 2 pre-scalings, two rescalings and four
// elementwise launches; here it is K + 2 gathers of four taps and K + 4 stores per pixel.
//   rounding  (d * W) / w is a multiply and an IEEE division, two FP32 roundings applied to each TAP before the blend:
//             (d * 960) / 240 is not always 4 * d, (d * W) / W not always d.  The blend is hp_tap / hp_blend of bilinear_hp.h with
//             mult = 1, the expression of dmb_bilinear_scale_f32: the maps equal the composition bit for bit.
//   layout    a workgroup of 256 threads owns 64 x 4 output pixels of one batch item, a wave one row of 64 consecutive x: every
//             store is one coalesced row segment, the low-resolution taps (a sixteenth to a quarter of the bytes) come from cache.
//             No LDS.  4-byte loads and stores only: one path for any alignment.
//   item      nothing depends on the grid: batch item i equals the same item run alone bit for bit.
#include "bilinear_hp.h"
#include "dmb_common.h"

namespace dmb {

constexpr int FM_MAXK = 3, FM_TW = 64, FM_TH = 4;

struct DeepPrunerFinalMaps {
  const float* d[FM_MAXK + 2];   // the K list maps, then min_disparity and max_disparity
  int h[FM_MAXK + 2], w[FM_MAXK + 2];
  float sh[FM_MAXK + 2], sw[FM_MAXK + 2];   // hp_scale(h, H), hp_scale(w, W)
};

template <int K>
__global__ __launch_bounds__(FM_TW * FM_TH) void deeppruner_final_maps_kernel(DeepPrunerFinalMaps m, float* __restrict__ out, int B,
                                                                             int H, int W) {
#pragma clang fp contract(off)
  const int xo = blockIdx.x * FM_TW + threadIdx.x, yo = blockIdx.y * FM_TH + threadIdx.y, b = blockIdx.z;
  if (xo >= W || yo >= H) return;
  const float Wf = (float)W;
  float u[K + 2];
#pragma unroll
  for (int k = 0; k < K + 2; ++k) {
    const int j = k < K ? k : FM_MAXK + (k - K);
    const int h = m.h[j], w = m.w[j];
    const float wf = (float)w;
    const float* p = m.d[j] + (size_t)b * h * w;
    const HpTap ty = hp_tap(yo, h, m.sh[j]), tx = hp_tap(xo, w, m.sw[j]);
    const float* r0 = p + ty.i0 * w;
    const float* r1 = p + ty.i1 * w;
    u[k] = hp_blend((r0[tx.i0] * Wf) / wf, (r0[tx.i1] * Wf) / wf, (r1[tx.i0] * Wf) / wf, (r1[tx.i1] * Wf) / wf, tx.l, ty.l, 1.f);
  }
  const size_t HW = (size_t)H * W, map = (size_t)B * HW;
  float* o = out + (size_t)b * HW + (size_t)yo * W + xo;
#pragma unroll
  for (int k = 0; k < K; ++k) o[k * map] = u[k];
  const float D = u[K - 1], Mn = u[K], Mx = u[K + 1];
  o[K * map] = (Mn * Wf) / Wf;
  o[(K + 1) * map] = (Mx * Wf) / Wf;
  o[(K + 2) * map] = fabsf(D - Mn);
  o[(K + 3) * map] = fabsf(Mx - D);
}

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_deeppruner_final_maps_f32(const float* d0, const float* d1, const float* d2, const int* h_host,
                                             const int* w_host, const float* min_disp, const float* max_disp, float* out, int K,
                                             int B, int h, int w, int H, int W, void* stream) {
  if (K < 1 || K > FM_MAXK) return fail(DMB_EUNSUPPORTED, "deeppruner_final_maps: 1 .. 3 maps in the list");
  const float* d[FM_MAXK] = {d0, d1, d2};
  if (!h_host || !w_host || !min_disp || !max_disp || !out || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "deeppruner_final_maps: bad argument");
  DeepPrunerFinalMaps m;
  for (int k = 0; k < FM_MAXK + 2; ++k) {
    m.d[k] = nullptr;
    m.h[k] = m.w[k] = 1;
  }
  for (int k = 0; k < K; ++k) {
    if (!d[k] || h_host[k] <= 0 || w_host[k] <= 0) return fail(DMB_EINVAL, "deeppruner_final_maps: bad map");
    m.d[k] = d[k];
    m.h[k] = h_host[k];
    m.w[k] = w_host[k];
  }
  m.d[FM_MAXK] = min_disp;
  m.d[FM_MAXK + 1] = max_disp;
  m.h[FM_MAXK] = m.h[FM_MAXK + 1] = h;
  m.w[FM_MAXK] = m.w[FM_MAXK + 1] = w;
  // a batch item of every map stays below 2 GiB, so that every index inside an item fits 31 bits
  for (int k = 0; k < FM_MAXK + 2; ++k)
    if (4LL * m.h[k] * m.w[k] >= 0x80000000LL) return fail(DMB_EUNSUPPORTED, "deeppruner_final_maps: map too large");
  if (4LL * H * W >= 0x80000000LL || B > 65535 || cdiv(H, FM_TH) > 65535)
    return fail(DMB_EUNSUPPORTED, "deeppruner_final_maps: map too large");
  for (int k = 0; k < FM_MAXK + 2; ++k) {
    m.sh[k] = hp_scale(m.h[k], H);
    m.sw[k] = hp_scale(m.w[k], W);
  }
  const dim3 grid(cdiv(W, FM_TW), cdiv(H, FM_TH), B), block(FM_TW, FM_TH);
  hipStream_t st = (hipStream_t)stream;
  switch (K) {
    case 1: hipLaunchKernelGGL(deeppruner_final_maps_kernel<1>, grid, block, 0, st, m, out, B, H, W); break;
    case 2: hipLaunchKernelGGL(deeppruner_final_maps_kernel<2>, grid, block, 0, st, m, out, B, H, W); break;
    default: hipLaunchKernelGGL(deeppruner_final_maps_kernel<3>, grid, block, 0, st, m, out, B, H, W); break;
  }
  return launch_status("deeppruner_final_maps launch failed");
}
