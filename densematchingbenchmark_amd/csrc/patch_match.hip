// DeepPruner's disparity sampler: differentiable PatchMatch and the range head + uniform sampler, forward and backward.
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

// ---------------------------------------------------------------------------------------------------------------------
// What one thread recomputes of a half-iteration: shared by the forward kernel and by both phases of the backward, so that a
// candidate, its taps (and with them the cell floor(ix) it falls into) and its cost are the forward's own bits.
// ---------------------------------------------------------------------------------------------------------------------
// propagation (patch_match.py:131-162): candidate j is the noise of the neighbour at offset j - 1, 0 outside the image
template <int VERTICAL>
__device__ inline float pm_noise(const float* __restrict__ nin, int j, int i, int y, int x, int H, int W) {
  if (j == 1) return nin[i];
  if (VERTICAL) return j == 0 ? (y > 0 ? nin[i - W] : 0.f) : (y + 1 < H ? nin[i + W] : 0.f);
  return j == 0 ? (x > 0 ? nin[i - 1] : 0.f) : (x + 1 < W ? nin[i + 1] : 0.f);
}

struct PmRange {
  float lo, hi, scale, base;
};

// patch_match.py:75-81, 338-339: (max - min) * interval * noise + (min + (max - min) * index_p)
__device__ inline PmRange pm_range(const float* __restrict__ dmin, const float* __restrict__ dmax, float cmin, float cmax, int b,
                                   int p, int i, int P, int HW, float interval) {
  PmRange r;
  r.lo = dmin ? dmin[(size_t)b * HW + i] : cmin;
  r.hi = dmax ? dmax[(size_t)b * HW + i] : cmax;
  const float range = (r.hi - r.lo);
  r.scale = (range * interval);
  r.base = (r.lo + (range * ((float)(p + 1) / (float)(P + 1))));
  return r;
}

__device__ inline float pm_sample(const PmRange& r, float n) { return ((r.scale * n) + r.base); }

// Evaluate: inverse_warp_3d(right, -samples) on plane 3p + j of 3P planes
__device__ inline WarpTaps pm_taps(float s, int p, int j, int y, int x, int P, int H, int W) {
  return warp_taps(-s, 3 * p + j, y, x, 3 * P, H, W);
}

struct PmCand {
  float n[3], s[3];
  WarpTaps t[3];
  PmRange r;
};

template <int VERTICAL>
__device__ inline void pm_candidates(PmCand& cd, const float* __restrict__ nin, const float* __restrict__ dmin,
                                     const float* __restrict__ dmax, float cmin, float cmax, int b, int p, int i, int y, int x,
                                     int P, int H, int W, float interval) {
  cd.r = pm_range(dmin, dmax, cmin, cmax, b, p, i, P, H * W, interval);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    cd.n[j] = pm_noise<VERTICAL>(nin, j, i, y, x, H, W);
    cd.s[j] = pm_sample(cd.r, cd.n[j]);
    cd.t[j] = pm_taps(cd.s[j], p, j, y, x, P, H, W);
  }
}

// d w_tap / d ix of the four image taps (both plane taps of an image point added up), as warp_volume.hip's sample gradient
// takes it: w = wx * wy * wz with wx = (x1 - ix) west, (ix - x0) east, so the derivative is -/+ (row weight * plane weight).
// Taps outside the volume count 0.
__device__ inline void pm_dtaps(const WarpTaps& t, int k, int y, int D, int H, float dq[4]) {
  const float gd = ((((float)k / (float)(D - 1)) * 2.f) - 1.f), gh = ((((float)y / (float)(H - 1)) * 2.f) - 1.f);
  const float iy = ((((gh + 1.f) * (float)H) - 1.f) / 2.f), iz = ((((gd + 1.f) * (float)D) - 1.f) / 2.f);
  const float wy1 = iy - floorf(iy), wy0 = (floorf(iy) + 1.f) - iy, wz1 = iz - floorf(iz), wz0 = (floorf(iz) + 1.f) - iz;
  const float wyq[4] = {wy0, wy0, wy1, wy1};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float wz = ((t.valid >> q & 1u) ? wz0 : 0.f) + ((t.valid >> (q + 4) & 1u) ? wz1 : 0.f);
    dq[q] = (q & 1 ? wyq[q] : -wyq[q]) * wz;
  }
}

// The channel walk: acc[j][c % 4] += L[c] * T_j[c] in ascending c; DERIV: dacc[j][c % 4] += L[c] * dT_j[c] / d ix likewise.
template <int DERIV>
__device__ inline void pm_channel_sums(const PmCand& cd, const float (*dq)[4], const float* __restrict__ Lp,
                                       const float* __restrict__ Rp, int C, int HW, float acc[3][4], float dacc[3][4]) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      acc[j][u] = 0.f;
      if (DERIV) dacc[j][u] = 0.f;
    }
  for (int c0 = 0; c0 < C; c0 += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int c = c0 + u;
      if (c < C) {
        const float l = Lp[(size_t)c * HW];
        const float* plane = Rp + (size_t)c * HW;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          acc[j][u] = (acc[j][u] + (l * warp_blend(cd.t[j], plane)));
          if (DERIV) {
            const unsigned any = cd.t[j].valid | (cd.t[j].valid >> 4);
            float gx = 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q)
              if (any >> q & 1u) gx += plane[cd.t[j].off[q]] * dq[j][q];
            dacc[j][u] += l * gx;
          }
        }
      }
    }
  }
}

// patch_match.py:231: mean over the channels times the temperature; :246-251: softmax over the 3 candidates
__device__ inline void pm_softmax(const float acc[3][4], int C, float temperature, float pr[3]) {
  float cost[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) cost[j] = ((((acc[j][0] + acc[j][1]) + (acc[j][2] + acc[j][3])) / (float)C) * temperature);
  const float m = fmaxf(fmaxf(cost[0], cost[1]), cost[2]);
  float e[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) e[j] = expf(cost[j] - m);
  const float den = ((e[0] + e[1]) + e[2]);
#pragma unroll
  for (int j = 0; j < 3; ++j) pr[j] = (e[j] / den);
}

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
  PmCand cd;
  pm_candidates<VERTICAL>(cd, noise_in + ((size_t)b * P + p) * HW, dmin, dmax, cmin, cmax, b, p, i, y, x, P, H, W, interval);
  float acc[3][4], pr[3];
  pm_channel_sums<0>(cd, nullptr, L + (size_t)b * C * HW + i, R + (size_t)b * C * HW, C, HW, acc, nullptr);
  pm_softmax(acc, C, temperature, pr);
  float ns = 0.f, nn = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    ns = (ns + (pr[j] * cd.s[j]));
    nn = (nn + (pr[j] * cd.n[j]));
  }
  if (noise_out) noise_out[((size_t)b * P + p) * HW + i] = nn;
  if (out) {
    float* o = out + (size_t)b * out_ctot * HW + i;
    o[(size_t)(out_coff + p) * HW] = ns;
    // patch_match.py:359: the ends of the range are samples too (channels next to the P inner ones)
    if (write_ends && p == 0) o[(size_t)(out_coff - 1) * HW] = cd.r.lo;
    if (write_ends && p == P - 1) o[(size_t)(out_coff + P) * HW] = cd.r.hi;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Backward of one half-iteration (docs/design/14, "Backward").  With pi the softmax, gS / gN the gradients of the step's samples
// and noise (absent = 0), tc = temperature / C:
//     a_j = gS s_j + gN n_j,   gc_j = pi_j (a_j - sum_j pi_j a_j)                      (softmax backward)
//     dL[c, i] += tc sum_j gc_j T_j[c],    dR += sampler adjoint of tc gc_j L[c, i] on plane 3p + j
//     gs_j = pi_j gS + tc gc_j sum_c L[c, i] dT_j[c] / ds,   gn_j = pi_j gN + scale gs_j
//     d_noise_in[neighbour j of i] += gn_j                                              (adjoint of the propagation)
// Phase one (one thread per pair, interval, pixel: the forward's grid) recomputes the three candidates and their costs with the
// forward's functions, walks the channels once for the costs AND the column derivatives, and leaves tc * gc_j and gn_j as
// [B, 3P, H, W] each.  Phase two owns one output row and eight channels (warp_volume.hip's adjoint): it recomputes each
// candidate's taps with the same functions, adds tc gc_k T_k[c] into one register per column in ascending k -- dL needs no
// scatter and has a fixed order -- and scatters tc gc_k L[c, i] times the tap's column and plane weight into ONE LDS row per
// channel (the row weights depend on y only), left as two partial rows [B, C, H, 2, W]: the sums times the north / south row weight.  The finishing launches add, per source row, the partial rows that point at it in ascending y,
// and gather d_noise_in from the three gn that name a pixel, in a fixed order.  Nothing of extent C x 3P exists.
// ---------------------------------------------------------------------------------------------------------------------
template <int VERTICAL>
__global__ __launch_bounds__(256) void patch_match_bwd_pixel_kernel(const float* __restrict__ L, const float* __restrict__ R,
                                                                    const float* __restrict__ noise_in,
                                                                    const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                                    float cmin, float cmax, const float* __restrict__ gS,
                                                                    const float* __restrict__ gN, float* __restrict__ gc,
                                                                    float* __restrict__ gn, int C, int P, int H, int W,
                                                                    float interval, float temperature, int gs_ctot, int gs_coff) {
  const int HW = H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y, b = blockIdx.z;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  PmCand cd;
  pm_candidates<VERTICAL>(cd, noise_in + ((size_t)b * P + p) * HW, dmin, dmax, cmin, cmax, b, p, i, y, x, P, H, W, interval);
  float dq[3][4];
#pragma unroll
  for (int j = 0; j < 3; ++j) pm_dtaps(cd.t[j], 3 * p + j, y, 3 * P, H, dq[j]);
  float acc[3][4], dacc[3][4], pr[3];
  pm_channel_sums<1>(cd, dq, L + (size_t)b * C * HW + i, R + (size_t)b * C * HW, C, HW, acc, dacc);
  pm_softmax(acc, C, temperature, pr);
  const float gs_up = gS ? gS[((size_t)b * gs_ctot + gs_coff + p) * HW + i] : 0.f;
  const float gn_up = gN ? gN[((size_t)b * P + p) * HW + i] : 0.f;
  float a[3], abar = 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    a[j] = gs_up * cd.s[j] + gn_up * cd.n[j];
    abar += pr[j] * a[j];
  }
  const float tc = temperature / (float)C;
  const float dsdix = -(((0.5f * (float)W)) * 2.f / (float)(W - 1));   // d ix / d sample: grid_sample's and inverse_warp_3d's scaling
  const size_t o = ((size_t)b * 3 * P + 3 * p) * HW + i;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float g = (pr[j] * (a[j] - abar)) * tc;
    const float dcol = (dacc[j][0] + dacc[j][1]) + (dacc[j][2] + dacc[j][3]);
    const float gs = pr[j] * gs_up + g * (dcol * dsdix);
    gc[o + (size_t)j * HW] = g;
    gn[o + (size_t)j * HW] = pr[j] * gn_up + cd.r.scale * gs;
  }
}

constexpr int PMB_CG = 8;   // channels per workgroup of phase two

template <int VERTICAL>
__global__ __launch_bounds__(256) void patch_match_bwd_rows_kernel(const float* __restrict__ L, const float* __restrict__ R,
                                                                   const float* __restrict__ noise_in,
                                                                   const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                                   float cmin, float cmax, const float* __restrict__ gc,
                                                                   const float* dL_acc, float* dL,   /* may be one tensor */
                                                                   float* __restrict__ part, int C, int P, int H, int W,
                                                                   float interval) {
  // One LDS row per channel, not one per source row: a tap's weight is (wx * wy) * wz and the row weights wy depend on y only,
  // i.e. are the same for the whole workgroup.  The row collects sum wx * (wy0 + wy1) * wz * g * L per SOURCE COLUMN (wy0 + wy1
  // = 1 up to rounding) and the two partial rows are that sum times wy0 (north) and wy1 (south): half the LDS adds.
  extern __shared__ float rows[];   // [PMB_CG][W]
  const int y = blockIdx.x, c0 = blockIdx.y * PMB_CG, b = blockIdx.z;
  const int HW = H * W;
  const int nc = min(PMB_CG, C - c0);   // channels of this group
  for (int i = threadIdx.x; i < PMB_CG * W; i += blockDim.x) rows[i] = 0.f;
  __syncthreads();
  const float* Rb = R + ((size_t)b * C + c0) * HW;
  // one thread owns one column and all channels of the group: a candidate's taps are computed once, and the gathers of the
  // channels are independent of each other
  for (int x = threadIdx.x; x < W; x += blockDim.x) {
    const int i = y * W + x;
    float dl[PMB_CG], lv[PMB_CG];
#pragma unroll
    for (int cl = 0; cl < PMB_CG; ++cl) {
      dl[cl] = 0.f;
      lv[cl] = cl < nc ? L[((size_t)b * C + c0 + cl) * HW + i] : 0.f;
    }
    for (int p = 0; p < P; ++p) {
      const PmRange r = pm_range(dmin, dmax, cmin, cmax, b, p, i, P, HW, interval);
      const float* nin = noise_in + ((size_t)b * P + p) * HW;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float s = pm_sample(r, pm_noise<VERTICAL>(nin, j, i, y, x, H, W));
        const WarpTaps t = pm_taps(s, p, j, y, x, P, H, W);
        const float g = gc[((size_t)b * 3 * P + 3 * p + j) * HW + i];
        // weight of the west | east source column: both row taps and the plane taps inside the volume add up
        const bool vz0 = (t.valid & 0x0fu) != 0u, vz1 = (t.valid & 0xf0u) != 0u;
        float cw[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const bool vx = ((t.valid | (t.valid >> 4)) & (0x5u << e)) != 0u;    // the column is inside the image
          cw[e] = (vx && vz0 ? t.w[e] + t.w[e + 2] : 0.f) + (vx && vz1 ? t.w[e + 4] + t.w[e + 6] : 0.f);
        }
        // the gathers of all channels first, unconditionally (an out-of-range tap reads offset 0 and is not used; a channel
        // past the group's last reads the last one's): none of them waits for another
        float v[PMB_CG][4];
#pragma unroll
        for (int cl = 0; cl < PMB_CG; ++cl)
#pragma unroll
          for (int q = 0; q < 4; ++q) v[cl][q] = Rb[(size_t)min(cl, nc - 1) * HW + t.off[q]];
#pragma unroll
        for (int cl = 0; cl < PMB_CG; ++cl) {
          if (cl >= nc) continue;
          dl[cl] += g * warp_blend_loaded(t, v[cl]);
          const float gt = g * lv[cl];
          float* row = rows + (size_t)cl * W;
          if (cw[0] != 0.f) atomicAdd(row + t.xi[0], cw[0] * gt);
          if (cw[1] != 0.f) atomicAdd(row + t.xi[1], cw[1] * gt);
        }
      }
    }
#pragma unroll
    for (int cl = 0; cl < PMB_CG; ++cl)
      if (cl < nc) {
        const size_t o = ((size_t)b * C + c0 + cl) * HW + i;
        dL[o] = dL_acc ? dL_acc[o] + dl[cl] : dl[cl];
      }
  }
  __syncthreads();
  // partial rows: part[b][c][y][ns][W] = the row's sums times the weight of the north | south source row (warp_taps.h's
  // arithmetic for the row coordinate; 0 where that row is outside the image)
  const float gh = ((((float)y / (float)(H - 1)) * 2.f) - 1.f);
  const float iy = ((((gh + 1.f) * (float)H) - 1.f) / 2.f);
  const float y0 = floorf(iy), y1 = (y0 + 1.f);
  const float wy[2] = {y0 >= 0.f && y0 < (float)H ? (y1 - iy) : 0.f, y1 >= 0.f && y1 < (float)H ? (iy - y0) : 0.f};
  for (int i = threadIdx.x; i < PMB_CG * W; i += blockDim.x) {
    const int cl = i / W, x = i - cl * W;
    if (c0 + cl < C) {
      float* o = part + (((size_t)b * C + c0 + cl) * H + y) * 2 * W + x;
      o[0] = rows[i] * wy[0];
      o[W] = rows[i] * wy[1];
    }
  }
}

// dR[b, c, yn, x] = dR_acc + the sum, in ascending y, of the partial rows of the output rows y whose north (south) source row
// is yn (warp_volume.hip's finishing kernel, restated: the row taps are warp_taps.h's)
__global__ __launch_bounds__(256) void patch_match_bwd_dr_kernel(const float* __restrict__ part, const float* dR_acc,   /* may be dR */
                                                                 float* dR, int H, int W) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int bc = blockIdx.y;
  if (i >= H * W) return;
  const int yn = i / W, x = i - yn * W;
  float acc = 0.f;
  for (int y = max(0, yn - 2); y <= min(H - 1, yn + 2); ++y) {
    const float gh = ((((float)y / (float)(H - 1)) * 2.f) - 1.f);
    const float iy = ((((gh + 1.f) * (float)H) - 1.f) / 2.f);
    const float y0 = floorf(iy), y1 = y0 + 1.f;
    const float* p = part + (((size_t)bc * H + y) * 2) * W + x;
    if (y0 >= 0.f && y0 < (float)H && (int)y0 == yn) acc += p[0];
    if (y1 >= 0.f && y1 < (float)H && (int)y1 == yn) acc += p[W];
  }
  const size_t o = (size_t)bc * H * W + i;
  dR[o] = dR_acc ? dR_acc[o] + acc : acc;
}

// d_noise_in[b, p, i] = gn_1[i] + gn_0[the pixel after i] + gn_2[the pixel before i]: the three candidates that read noise_in at i
template <int VERTICAL>
__global__ __launch_bounds__(256) void patch_match_bwd_noise_kernel(const float* __restrict__ gn, float* __restrict__ d_noise,
                                                                    int P, int H, int W) {
  const int HW = H * W;
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int p = blockIdx.y, b = blockIdx.z;
  if (i >= HW) return;
  const int y = i / W, x = i - y * W;
  const float* g = gn + ((size_t)b * 3 * P + 3 * p) * HW;
  const int step = VERTICAL ? W : 1;
  const bool after = VERTICAL ? y + 1 < H : x + 1 < W, before = VERTICAL ? y > 0 : x > 0;
  float acc = g[(size_t)HW + i];
  if (after) acc += g[i + step];
  if (before) acc += g[(size_t)2 * HW + i - step];
  d_noise[((size_t)b * P + p) * HW + i] = acc;
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

// Backward of the launch above: one thread per (pair, pixel), every element of d_min and d_max written once.  The subgradients
// are torch's: minimum / maximum split a tie in halves, clamp passes the gradient at its bounds (and at 0 for the shortfall).
__global__ __launch_bounds__(256) void deeppruner_uniform_bwd_kernel(const float* __restrict__ dmin, const float* __restrict__ dmax,
                                                                     const float* __restrict__ dout, float* __restrict__ gmin_out,
                                                                     float* __restrict__ gmax_out, int HW, int N, int range_head,
                                                                     float limit) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= HW) return;
  const float* g = dout + (size_t)b * N * HW + i;
  // out_k = lo + (hi - lo) * f_k: d lo = sum_k g_k (1 - f_k), d hi = sum_k g_k f_k, in ascending k
  float glo = g[0], ghi = g[(size_t)(N - 1) * HW];
  for (int k = 1; k < N - 1; ++k) {
    const float f = ((float)k / (float)(N - 1)), gk = g[(size_t)k * HW];
    glo += gk - gk * f;
    ghi += gk * f;
  }
  if (range_head) {
    const float lo = dmin[(size_t)b * HW + i], hi = dmax[(size_t)b * HW + i];
    const float gmin = lo < hi ? lo : hi, gmax = lo > hi ? lo : hi;
    const float v = ((gmin + (float)N) - gmax);
    const float over = v < 0.f ? 0.f : v;
    const float a = ((gmin - over) / 2.f), c = ((gmax + over) / 2.f);
    const float ga = (a >= 0.f && a <= limit) ? glo / 2.f : 0.f;    // through the clamp and the halving
    const float gb = (c >= 0.f && c <= limit) ? ghi / 2.f : 0.f;
    const float gv = v >= 0.f ? gb - ga : 0.f;                       // over enters a with -1, c with +1
    const float g_min = ga + gv, g_max = gb - gv;                    // d gmin, d gmax (v = gmin + N - gmax)
    if (lo == hi) {
      glo = g_min / 2.f + g_max / 2.f;
      ghi = glo;
    } else if (lo < hi) {
      glo = g_min;
      ghi = g_max;
    } else {
      glo = g_max;
      ghi = g_min;
    }
  }
  gmin_out[(size_t)b * HW + i] = glo;
  gmax_out[(size_t)b * HW + i] = ghi;
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

extern "C" int dmb_patch_match_step_bwd_f32(const float* L, const float* R, const float* noise_in, const float* min_disp,
                                            const float* max_disp, float min_const, float max_const, const float* g_samples,
                                            const float* g_noise, const float* dL_acc, const float* dR_acc, float* dL, float* dR,
                                            float* d_noise_in, float* workspace, int B, int C, int P, int H, int W, int vertical,
                                            float temperature, int gs_channels_total, int gs_ch_offset, void* stream) {
  if (!L || !R || !noise_in || (!g_samples && !g_noise) || !dL || !dR || !d_noise_in || !workspace || B <= 0 || C <= 0 || P <= 0 ||
      H <= 0 || W <= 0 || (min_disp == nullptr) != (max_disp == nullptr))
    return fail(DMB_EINVAL, "patch_match_step_bwd: bad argument");
  if (H < 2 || W < 2) return fail(DMB_EUNSUPPORTED, "patch_match_step_bwd: the reference divides by (size - 1); H, W must be >= 2");
  if (P > PM_MAX_P) return fail(DMB_EUNSUPPORTED, "patch_match_step_bwd: more than DMB_PATCH_MATCH_MAX_SAMPLES intervals");
  if (W > DMB_PATCH_MATCH_BWD_MAX_W)
    return fail(DMB_EUNSUPPORTED, "patch_match_step_bwd: more than DMB_PATCH_MATCH_BWD_MAX_W columns (eight channel rows in LDS)");
  if ((long long)C * H * W >= 0x7fffffffLL || (long long)3 * P * H * W >= 0x7fffffffLL || B > 65535 || H > 65535 ||
      (long long)B * C > 65535)
    return fail(DMB_EUNSUPPORTED, "patch_match_step_bwd: feature map too large");
  if (g_samples && (gs_ch_offset < 0 || gs_ch_offset + P > gs_channels_total || (long long)gs_channels_total * H * W >= 0x7fffffffLL))
    return fail(DMB_EINVAL, "patch_match_step_bwd: the samples' gradient does not fit its channels");
  const float interval = (float)(1.0 / (double)(P + 1));   // as the forward
  const size_t planes = (size_t)B * 3 * P * H * W;
  float* gc = workspace;                 // [B, 3P, H, W]  tc * gc_j
  float* gn = workspace + planes;        // [B, 3P, H, W]  gn_j
  float* part = workspace + 2 * planes;  // [B, C, H, 2, W]
  const dim3 pgrid(cdiv(H * W, 256), P, B), rgrid(H, cdiv(C, PMB_CG), B);
  const size_t lds = (size_t)PMB_CG * W * sizeof(float);
  const int rthreads = W >= 256 ? 256 : cdiv(W, 64) * 64;   // one thread per column, whole waves
  hipStream_t st = (hipStream_t)stream;
#define DMB_PM_BWD(V)                                                                                                              \
  do {                                                                                                                            \
    hipLaunchKernelGGL((patch_match_bwd_pixel_kernel<V>), pgrid, dim3(256), 0, st, L, R, noise_in, min_disp, max_disp, min_const, \
                       max_const, g_samples, g_noise, gc, gn, C, P, H, W, interval, temperature, gs_channels_total, gs_ch_offset); \
    hipLaunchKernelGGL((patch_match_bwd_rows_kernel<V>), rgrid, dim3(rthreads), lds, st, L, R, noise_in, min_disp, max_disp, min_const, \
                       max_const, gc, dL_acc, dL, part, C, P, H, W, interval);                                                    \
    hipLaunchKernelGGL((patch_match_bwd_noise_kernel<V>), pgrid, dim3(256), 0, st, gn, d_noise_in, P, H, W);                      \
  } while (0)
  if (vertical) DMB_PM_BWD(1);
  else DMB_PM_BWD(0);
#undef DMB_PM_BWD
  hipLaunchKernelGGL(patch_match_bwd_dr_kernel, dim3(cdiv(H * W, 256), B * C), dim3(256), 0, st, part, dR_acc, dR, H, W);
  return launch_status("patch_match_step_bwd launch failed");
}

extern "C" int dmb_deeppruner_uniform_samples_bwd_f32(const float* min_disp, const float* max_disp, const float* d_out,
                                                      float* d_min, float* d_max, int B, int H, int W, int N, int range_head,
                                                      float max_disp_limit, void* stream) {
  if (!d_out || !d_min || !d_max || (range_head && (!min_disp || !max_disp)) || B <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "deeppruner_uniform_samples_bwd: bad argument");
  if (N < 2 || N > DMB_MAX_DISP_SAMPLES) return fail(DMB_EUNSUPPORTED, "deeppruner_uniform_samples_bwd: 2 .. DMB_MAX_DISP_SAMPLES samples");
  if ((long long)N * H * W >= 0x7fffffffLL || B > 65535) return fail(DMB_EUNSUPPORTED, "deeppruner_uniform_samples_bwd: map too large");
  hipLaunchKernelGGL(deeppruner_uniform_bwd_kernel, dim3(cdiv(H * W, 256), B), dim3(256), 0, (hipStream_t)stream, min_disp, max_disp,
                     d_out, d_min, d_max, H * W, N, range_head, max_disp_limit);
  return launch_status("deeppruner_uniform_samples_bwd launch failed");
}
