// DeepPruner's disparity sampler: differentiable PatchMatch (forward) and the range head + uniform sampler.
//
// Reference semantics: dmb/modeling/stereo/disp_samplers/utils/patch_match.py:119-174 (Propagation), :218-253 (Evaluate),
// :329-356 (the half-iterations) and disp_samplers/DeepPruner.py:48-66 (DisparitySampleRangeHead), :99-115 (UniformSampler).
//
// The reference expands both feature maps to [B, C, 3P, H, W] per half-iteration, warps one of them with a 5-D grid_sample,
// takes a channel mean and a 3-way softmax.  Here one launch is one half-iteration and one thread owns one (pair, interval,
// pixel): it reads the interval's noise at the pixel and its two neighbours (0 outside the image: the reference's zero-padded
// one-hot convolution), forms the three candidates, computes the sampler's taps once per candidate (warp_taps.h: the
// reference's FP32 arithmetic, the volume being D = 3P planes and the candidate's plane k = 3p + j), and walks the channels
// once, blending the right feature at the three candidates against one load of the left feature.  Nothing of extent C x 3P
// is ever stored.  The neighbours need the previous half-iteration finished on the whole map, which is the launch boundary.
//
// Summation order of one output: channel c adds into partial sum c % 4 in ascending c, the partial sums are added as
// (a0 + a1) + (a2 + a3).  It depends on nothing but C, so a pair computes the same bits alone or in a batch.
#include "dmb_common.h"
#include "warp_taps.h"

namespace dmb {

constexpr int PM_MAX_P = DMB_PATCH_MATCH_MAX_SAMPLES;

// No contraction in this file (build.py also compiles it with -ffp-contract=off): candidates, taps and blends round as the
// reference's FP32 operations do.
#pragma clang fp contract(off)

template <int VERTICAL>
__global__ __launch_bounds__(256) void patch_match_step_kernel(const float* __restrict__ L, const float* __restrict__ R,
                                                               const float* __restrict__ noise_in,
                                                               const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                               float cmin, float cmax, float* __restrict__ noise_out,
                                                               float* __restrict__ out, int C, int P, int H, int W,
                                                               float interval, float temperature, int out_ctot, int out_coff,
                                                               int write_ends) {
  const int HW = H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y, b = blockIdx.z;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  // propagation (patch_match.py:131-162): candidate j is the noise of the neighbour at offset j - 1, 0 outside the image
  const float* nin = noise_in + ((size_t)b * P + p) * HW;
  float n[3];
  n[1] = nin[i];
  if (VERTICAL) {
    n[0] = y > 0 ? nin[i - W] : 0.f;
    n[2] = y + 1 < H ? nin[i + W] : 0.f;
  } else {
    n[0] = x > 0 ? nin[i - 1] : 0.f;
    n[2] = x + 1 < W ? nin[i + 1] : 0.f;
  }
  const float lo = dmin ? dmin[(size_t)b * HW + i] : cmin;
  const float hi = dmax ? dmax[(size_t)b * HW + i] : cmax;
  // patch_match.py:75-81, 338-339: (max - min) * interval * noise + (min + (max - min) * index_p)
  const float range = (hi - lo);
  const float scale = (range * interval);
  const float base = (lo + (range * ((float)(p + 1) / (float)(P + 1))));
  float s[3];
  WarpTaps t[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    s[j] = ((scale * n[j]) + base);
    t[j] = warp_taps(-s[j], 3 * p + j, y, x, 3 * P, H, W);   // Evaluate: inverse_warp_3d(right, -samples)
  }
  const float* Lp = L + (size_t)b * C * HW + i;
  const float* Rp = R + (size_t)b * C * HW;
  float acc[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[j][u] = 0.f;
  for (int c0 = 0; c0 < C; c0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u;
      if (c < C) {
        const float l = Lp[(size_t)c * HW];
        const float* plane = Rp + (size_t)c * HW;
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[j][u] = (acc[j][u] + (l * warp_blend(t[j], plane)));
      }
    }
  }
  // patch_match.py:231: mean over the channels times the temperature; :246-251: softmax over the 3 candidates
  float cost[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) cost[j] = ((((acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3])) / (float)C) * temperature);
  const float m = fmaxf(fmaxf(cost[0], cost[1]), cost[2]);
  float e[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) e[j] = expf(cost[j] - m);
  const float den = ((e[0] + e[1]) + e[2]);
  float ns = 0.f, nn = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float pr = (e[j] / den);
    ns = (ns + (pr * s[j]));
    nn = (nn + (pr * n[j]));
  }
  if (noise_out) noise_out[((size_t)b * P + p) * HW + i] = nn;
  if (out) {
    float* o = out + (size_t)b * out_ctot * HW + i;
    o[(size_t)(out_coff + p) * HW] = ns;
    // patch_match.py:359: the ends of the range are samples too (channels next to the P inner ones)
    if (write_ends && p == 0) o[(size_t)(out_coff - 1) * HW] = lo;
    if (write_ends && p == P - 1) o[(size_t)(out_coff + P) * HW] = hi;
  }
}

// DeepPruner.py:48-66 (range head, optional) then :99-115 (uniform sampler): one thread per (pair, pixel)
__global__ __launch_bounds__(256) void deeppruner_uniform_kernel(const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                                 float* __restrict__ out, int HW, int N, int range_head,
                                                                 float limit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= HW) return;
  float lo = dmin[(size_t)b * HW + i], hi = dmax[(size_t)b * HW + i];
  if (range_head) {
    const bool nan = lo != lo || hi != hi;     // torch.min / torch.max propagate NaN
    const float gmin = nan ? (lo + hi) : (lo < hi ? lo : hi);
    const float gmax = nan ? (lo + hi) : (lo > hi ? lo : hi);
    float over = ((gmin + (float)N) - gmax);
    over = over < 0.f ? 0.f : over;
    lo = ((gmin - over) / 2.f);
    hi = ((gmax + over) / 2.f);
    lo = lo < 0.f ? 0.f : (lo > limit ? limit : lo);
    hi = hi < 0.f ? 0.f : (hi > limit ? limit : hi);
  }
  float* o = out + (size_t)b * N * HW + i;
  o[0] = lo;
  const float range = (hi - lo);
  for (int k = 1; k < N - 1; ++k) o[(size_t)k * HW] = (lo + (range * ((float)k / (float)(N - 1))));
  o[(size_t)(N - 1) * HW] = hi;
}

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_patch_match_step_f32(const float* L, const float* R, const float* noise_in, const float* min_disp,
                                        const float* max_disp, float min_const, float max_const, float* noise_out, float* out,
                                        int B, int C, int P, int H, int W, int vertical, float temperature,
                                        int out_channels_total, int out_ch_offset, int write_ends, void* stream) {
  if (!L || !R || !noise_in || (!noise_out && !out) || B <= 0 || C <= 0 || P <= 0 || H <= 0 || W <= 0 || noise_out == noise_in ||
      (min_disp == nullptr) != (max_disp == nullptr))
    return fail(DMB_EINVAL, "patch_match_step: bad argument");
  if (H < 2 || W < 2) return fail(DMB_EUNSUPPORTED, "patch_match_step: the reference divides by (size - 1); H, W must be >= 2");
  if (P > PM_MAX_P) return fail(DMB_EUNSUPPORTED, "patch_match_step: more than DMB_PATCH_MATCH_MAX_SAMPLES intervals");
  if ((long long)C * H * W >= 0x7fffffffLL || B > 65535) return fail(DMB_EUNSUPPORTED, "patch_match_step: feature map too large");
  if (out) {
    const int first = out_ch_offset - (write_ends ? 1 : 0), last = out_ch_offset + P + (write_ends ? 1 : 0);
    if (first < 0 || last > out_channels_total || (long long)out_channels_total * H * W >= 0x7fffffffLL)
      return fail(DMB_EINVAL, "patch_match_step: the samples do not fit the output's channels");
  }
  const float interval = (float)(1.0 / (double)(P + 1));   // patch_match.py:65: a Python double, rounded when it meets the FP32 tensor
  const dim3 grid(cdiv(H * W, 256), P, B);
  hipStream_t st = (hipStream_t)stream;
  if (vertical)
    hipLaunchKernelGGL((patch_match_step_kernel<1>), grid, dim3(256), 0, st, L, R, noise_in, min_disp, max_disp, min_const,
                       max_const, noise_out, out, C, P, H, W, interval, temperature, out_channels_total, out_ch_offset, write_ends);
  else
    hipLaunchKernelGGL((patch_match_step_kernel<0>), grid, dim3(256), 0, st, L, R, noise_in, min_disp, max_disp, min_const,
                       max_const, noise_out, out, C, P, H, W, interval, temperature, out_channels_total, out_ch_offset, write_ends);
  return launch_status("patch_match_step launch failed");
}

extern "C" int dmb_deeppruner_uniform_samples_f32(const float* min_disp, const float* max_disp, float* out, int B, int H, int W,
                                                  int N, int range_head, float max_disp_limit, void* stream) {
  if (!min_disp || !max_disp || !out || B <= 0 || H <= 0 || W <= 0) return fail(DMB_EINVAL, "deeppruner_uniform_samples: bad argument");
  if (N < 2 || N > DMB_MAX_DISP_SAMPLES) return fail(DMB_EUNSUPPORTED, "deeppruner_uniform_samples: 2 .. DMB_MAX_DISP_SAMPLES samples");
  if ((long long)N * H * W >= 0x7fffffffLL || B > 65535) return fail(DMB_EUNSUPPORTED, "deeppruner_uniform_samples: map too large");
  hipLaunchKernelGGL(deeppruner_uniform_kernel, dim3(cdiv(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, min_disp, max_disp,
                     out, H * W, N, range_head, max_disp_limit);
  return launch_status("deeppruner_uniform_samples launch failed");
}
