// The training losses of the DeepPruner model (models/DeepPruner.py:82-108, losses/smooth_l1_loss.py:35-58,
// losses/utils/quantile_loss.py:25-37) on the low-resolution maps the model holds: ONE forward launch (plus the finalising block)
// and ONE backward launch; no full-size tensor is written or allocated.  With up(d) = F.interpolate((d * W) / w_d, (H, W), bilinear,
// align_corners=False), Mn = up(min), Mx = up(max), Rn = (Mn * W) / W, Rx = (Mx * W) / W -- bit for bit the maps of
// deeppruner_final_maps.hip (hp_tap / hp_blend of bilinear_hp.h, per-tap multiply then IEEE divide) -- the K + 4 means are
//   out[k]     = mean smooth_l1(up(d_k) - gt), k < K       under l1_lower < gt < l1_upper; 0 when no pixel is valid
//   out[K]     = mean smooth_l1(Rn - gt),  out[K + 1] = mean smooth_l1(Rx - gt)
//   out[K + 2] = mean (gt - Mn) * (theta - [gt - Mn < 0])  under q_lower < gt < q_upper; NaN when no pixel is valid
//   out[K + 3] = mean (gt - Mx) * ((1 - theta) - [gt - Mx < 0])
//   arithmetic  per-pixel terms FP32 (smooth_l1_term of loss_terms.h, the statement of map_loss_fwd_kernel); sums FP64, per thread
//               over its tiles, per block (block_sum), then one finalising block; the two counts are FP64 sums of ones: exact.
//               No floating-point atomics: results are identical from run to run.
//   forward     a block of 256 threads owns 64 x 4 full-size pixels at a time, a wave one row of 64 consecutive x (the layout of
//               deeppruner_final_maps.hip: gt is one coalesced row segment, the taps come from cache) and strides over the tiles
//               with at most DL_MAX_BLOCKS blocks, so the workspace has a fixed size.
//   backward    a gather: 2^lg lanes own one low-resolution pixel and visit the full-size pixels whose taps include it, lanes
//               along x (consecutive lanes read consecutive gt), a loop along y; membership is decided by hp_tap itself over a
//               conservative range.  Each visit recomputes the up-sampled value, takes the term's derivative and accumulates
//               derivative x blend weight in FP64, ascending (x, y) per lane, then a fixed butterfly over the 2^lg lanes.  The
//               tap scale W / w is applied to the sum once.  min and max share size, taps and gt: one item gathers both.
//               The K + 1 items have different sizes: a table of them, with their first block, is passed by value.
// 4-byte loads and stores only: one path for any alignment.
#include "bilinear_hp.h"
#include "dmb_common.h"
#include "loss_terms.h"

namespace dmb {

constexpr int DL_MAXK = 3, DL_TW = 64, DL_TH = 4, DL_MAX_BLOCKS = 1024, DL_NSUM = DL_MAXK + 6;
static_assert(DL_TW * DL_TH == LOSS_BLOCK, "block_sum is written for LOSS_BLOCK threads");
static_assert(DL_NSUM * DL_MAX_BLOCKS == DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES, "the header states the workspace");

struct DeepPrunerLossMaps {
  const float* d[DL_MAXK + 2];   // the K list maps, then min_disparity and max_disparity (slots K and K + 1)
  int h[DL_MAXK + 2], w[DL_MAXK + 2];
  float sh[DL_MAXK + 2], sw[DL_MAXK + 2];   // hp_scale(h, H), hp_scale(w, W)
};

// (gt - M) * (c - [gt - M < 0]), c = theta or 1 - theta (quantile_loss.py:28-30,34-36)
__device__ __forceinline__ float quantile_term(float g, float m, float c) {
#pragma clang fp contract(off)
  const float x = g - m;
  return x * (c - (x < 0.f ? 1.f : 0.f));
}

// partial[j * gridDim.x + block]: j < K + 2 the smooth-L1 sums, K + 2 and K + 3 the quantile sums, K + 4 and K + 5 the two counts
template <int K>
__global__ __launch_bounds__(LOSS_BLOCK) void deeppruner_loss_fwd_kernel(DeepPrunerLossMaps m, const float* __restrict__ gt,
                                                                         double* __restrict__ partial, int B, int H, int W,
                                                                         int tiles_x, int tiles_y, float l1_lo, float l1_hi,
                                                                         float q_lo, float q_hi, float th, float th1) {
#pragma clang fp contract(off)
  __shared__ double sm[4];
  double acc[K + 6];
#pragma unroll
  for (int j = 0; j < K + 6; ++j) acc[j] = 0.0;
  const int lx = threadIdx.x & (DL_TW - 1), ly = threadIdx.x / DL_TW;
  const float Wf = (float)W;
  const size_t HW = (size_t)H * W;
  const long long ntiles = (long long)B * tiles_y * tiles_x;
  for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int tx_i = (int)(t % tiles_x);
    const long long r = t / tiles_x;
    const int ty_i = (int)(r % tiles_y), b = (int)(r / tiles_y);
    const int xo = tx_i * DL_TW + lx, yo = ty_i * DL_TH + ly;
    if (xo >= W || yo >= H) continue;
    const float g = gt[(size_t)b * HW + (size_t)yo * W + xo];
    const bool l1 = g > l1_lo && g < l1_hi, q = g > q_lo && g < q_hi;
    if (!l1 && !q) continue;
    float u[K + 2];
#pragma unroll
    for (int k = 0; k < K + 2; ++k) {
      const int h = m.h[k], w = m.w[k];
      const float wf = (float)w;
      const float* p = m.d[k] + (size_t)b * h * w;
      const HpTap ty = hp_tap(yo, h, m.sh[k]), tx = hp_tap(xo, w, m.sw[k]);
      const float* r0 = p + ty.i0 * w;
      const float* r1 = p + ty.i1 * w;
      u[k] = hp_blend((r0[tx.i0] * Wf) / wf, (r0[tx.i1] * Wf) / wf, (r1[tx.i0] * Wf) / wf, (r1[tx.i1] * Wf) / wf, tx.l, ty.l, 1.f);
    }
    const float Mn = u[K], Mx = u[K + 1];
    if (l1) {
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] += (double)smooth_l1_term(fabsf(u[k] - g));
      acc[K] += (double)smooth_l1_term(fabsf((Mn * Wf) / Wf - g));
      acc[K + 1] += (double)smooth_l1_term(fabsf((Mx * Wf) / Wf - g));
      acc[K + 4] += 1.0;
    }
    if (q) {
      acc[K + 2] += (double)quantile_term(g, Mn, th);
      acc[K + 3] += (double)quantile_term(g, Mx, th1);
      acc[K + 5] += 1.0;
    }
  }
#pragma unroll
  for (int j = 0; j < K + 6; ++j) {
    const double s = block_sum(acc[j], sm);
    if (threadIdx.x == 0) partial[(size_t)j * gridDim.x + blockIdx.x] = s;
  }
}

// The two quantile terms on maps already at the ground truth's size: partial[j * gridDim.x + block], j = 0, 1 the sums, 2 the count.
__global__ __launch_bounds__(LOSS_BLOCK) void quantile_loss_fwd_kernel(const float* __restrict__ mn, const float* __restrict__ mx,
                                                                       const float* __restrict__ gt, double* __restrict__ partial,
                                                                       long long n, float q_lo, float q_hi, float th, float th1) {
  __shared__ double sm[4];
  double a0 = 0.0, a1 = 0.0, cnt = 0.0;
  for (long long i = blockIdx.x * (long long)LOSS_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * LOSS_BLOCK) {
    const float g = gt[i];
    if (g > q_lo && g < q_hi) {
      a0 += (double)quantile_term(g, mn[i], th);
      a1 += (double)quantile_term(g, mx[i], th1);
      cnt += 1.0;
    }
  }
  const double s0 = block_sum(a0, sm), s1 = block_sum(a1, sm), sc = block_sum(cnt, sm);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = s0;
    partial[(size_t)gridDim.x + blockIdx.x] = s1;
    partial[2 * (size_t)gridDim.x + blockIdx.x] = sc;
  }
}

// nl1 smooth-L1 sums, two quantile sums, then (nl1 > 0) the smooth-L1 count and the quantile count.
// out[j] = sum / count: an empty smooth-L1 level is 0 (smooth_l1_loss.py:49-53), an empty quantile term 0 / 0 = NaN (the mean of an
// empty tensor).  stats = (smooth-L1 count, quantile count), FP64: exact at any size.
__global__ __launch_bounds__(LOSS_BLOCK) void deeppruner_loss_finalize_kernel(const double* __restrict__ partial, int nblk, int nl1,
                                                                              float* __restrict__ out, double* __restrict__ stats) {
  __shared__ double tot[DL_NSUM];
  const int nsum = nl1 + 2 + (nl1 > 0 ? 2 : 1);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int j = wave; j < nsum; j += LOSS_BLOCK / 64) {   // a wave per sum: its lanes stride over the blocks, then a fixed tree
    double s = 0.0;
    for (int i = lane; i < nblk; i += 64) s += partial[(size_t)j * nblk + i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if (lane == 0) tot[j] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double n1 = nl1 > 0 ? tot[nsum - 2] : 0.0, nq = tot[nsum - 1];
    for (int j = 0; j < nl1; ++j) out[j] = n1 > 0.0 ? (float)(tot[j] / n1) : 0.f;
    out[nl1] = (float)(tot[nl1] / nq);
    out[nl1 + 1] = (float)(tot[nl1 + 1] / nq);
    stats[0] = n1;
    stats[1] = nq;
  }
}

struct DeepPrunerLossItem {
  const float* a;     // a list map, or min_disparity
  const float* b;     // max_disparity (the range item), else nullptr
  float* ga;
  float* gb;
  int h, w;
  float sh, sw;       // hp_scale(h, H), hp_scale(w, W)
  int lg;             // 2^lg lanes per low-resolution pixel
  int tiles_x;        // blocks per row of tiles: a block owns (64 >> lg) columns x 4 rows of the map
  int tiles_y;
  int first_block;
  int slot;           // grad_out[slot] weighs this map's smooth-L1 term (the range item: slot for min, slot + 1 for max)
};
struct DeepPrunerLossTable {
  DeepPrunerLossItem it[DL_MAXK + 1];
  int n;
};

// Destination indices whose taps can include source index i: src = scale * (dst + 0.5) - 0.5 lies in [i - 1, i + 1) for
// dst + 0.5 in [(i - 0.5) / scale, (i + 1.5) / scale); one more on either side for the FP32 roundings.  hp_tap decides.  (Where
// src is clamped to 0, index 1 is named as a tap of weight 0 outside this range: it carries nothing.)
__device__ __forceinline__ void footprint(int i, int in, int out, int& lo, int& hi) {
  const float f = (float)out / (float)in;
  lo = (int)floorf(((float)i - 0.5f) * f - 0.5f) - 1;
  hi = (int)ceilf(((float)i + 1.5f) * f - 0.5f) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}

__device__ __forceinline__ float tap_weight(const HpTap& t, int i) { return (t.i0 == i ? 1.f - t.l : 0.f) + (t.i1 == i ? t.l : 0.f); }

__global__ __launch_bounds__(LOSS_BLOCK) void deeppruner_loss_bwd_kernel(DeepPrunerLossTable tb, const float* __restrict__ gt,
                                                                         const double* __restrict__ stats,
                                                                         const float* __restrict__ grad_out, int K, int H, int W,
                                                                         float l1_lo, float l1_hi, float q_lo, float q_hi, float th,
                                                                         float th1) {
#pragma clang fp contract(off)
  DeepPrunerLossItem it = tb.it[0];
#pragma unroll
  for (int k = 1; k < DL_MAXK + 1; ++k)
    if (k < tb.n && (int)blockIdx.x >= tb.it[k].first_block) it = tb.it[k];
  const int local = (int)blockIdx.x - it.first_block;
  const int tx_i = local % it.tiles_x, r = local / it.tiles_x;
  const int ty_i = r % it.tiles_y, b = r / it.tiles_y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int G = 1 << it.lg, sub = lane >> it.lg, g_lane = lane & (G - 1);
  const int h = it.h, w = it.w;
  const int i = ty_i * 4 + wave, j = tx_i * (64 >> it.lg) + sub;
  const bool valid = i < h && j < w, range = it.b != nullptr;
  // d loss / d term: grad_out over the count; nothing flows from an empty mask
  const double n1 = stats[0], nq = stats[1];
  const double c1a = n1 > 0.0 ? (double)grad_out[it.slot] / n1 : 0.0;
  const double c1b = range && n1 > 0.0 ? (double)grad_out[it.slot + 1] / n1 : 0.0;
  const double cqa = range && nq > 0.0 ? (double)grad_out[K + 2] / nq : 0.0;
  const double cqb = range && nq > 0.0 ? (double)grad_out[K + 3] / nq : 0.0;
  const float Wf = (float)W, wf = (float)w;
  double acc_a = 0.0, acc_b = 0.0;
  if (valid) {
    int y0, y1, x0, x1;
    footprint(i, h, H, y0, y1);
    footprint(j, w, W, x0, x1);
    const size_t item = (size_t)b * h * w;
    const float* pa = it.a + item;
    const float* pb = range ? it.b + item : nullptr;
    const float* gb = gt + (size_t)b * H * W;
    for (int x = x0 + g_lane; x <= x1; x += G) {
      const HpTap tx = hp_tap(x, w, it.sw);
      if (tx.i0 != j && tx.i1 != j) continue;
      const float wx = tap_weight(tx, j);
      // A row that includes i has its taps on rows i - 1 and i, or i and i + 1 (clamped): the scaled taps of these three rows at
      // this column's two taps are formed once, by the forward's statement, and chosen per row below.
      const int rm = (i > 0 ? i - 1 : 0) * w, rc = i * w, rp = (i < h - 1 ? i + 1 : i) * w;
      const float am0 = (pa[rm + tx.i0] * Wf) / wf, am1 = (pa[rm + tx.i1] * Wf) / wf, ac0 = (pa[rc + tx.i0] * Wf) / wf,
                  ac1 = (pa[rc + tx.i1] * Wf) / wf, ap0 = (pa[rp + tx.i0] * Wf) / wf, ap1 = (pa[rp + tx.i1] * Wf) / wf;
      float bm0 = 0.f, bm1 = 0.f, bc0 = 0.f, bc1 = 0.f, bp0 = 0.f, bp1 = 0.f;
      if (range) {
        bm0 = (pb[rm + tx.i0] * Wf) / wf, bm1 = (pb[rm + tx.i1] * Wf) / wf, bc0 = (pb[rc + tx.i0] * Wf) / wf;
        bc1 = (pb[rc + tx.i1] * Wf) / wf, bp0 = (pb[rp + tx.i0] * Wf) / wf, bp1 = (pb[rp + tx.i1] * Wf) / wf;
      }
      for (int y = y0; y <= y1; ++y) {
        const HpTap ty = hp_tap(y, h, it.sh);
        if (ty.i0 != i && ty.i1 != i) continue;
        const float g = gb[y * W + x];
        const bool l1 = g > l1_lo && g < l1_hi, q = range && g > q_lo && g < q_hi;
        if (!l1 && !q) continue;
        const double wgt = (double)tap_weight(ty, i) * (double)wx;
        const bool top_c = ty.i0 == i, bot_c = ty.i1 == i;      // top: row i or i - 1; bottom: row i or i + 1
        const float va = hp_blend(top_c ? ac0 : am0, top_c ? ac1 : am1, bot_c ? ac0 : ap0, bot_c ? ac1 : ap1, tx.l, ty.l, 1.f);
        if (!range) {
          acc_a += c1a * (double)fminf(fmaxf(va - g, -1.f), 1.f) * wgt;
        } else {
          const float vb = hp_blend(top_c ? bc0 : bm0, top_c ? bc1 : bm1, bot_c ? bc0 : bp0, bot_c ? bc1 : bp1, tx.l, ty.l, 1.f);
          double da = 0.0, db = 0.0;
          if (l1) {   // the second scaling (M * W) / W differentiates to 1
            da = c1a * (double)fminf(fmaxf((va * Wf) / Wf - g, -1.f), 1.f);
            db = c1b * (double)fminf(fmaxf((vb * Wf) / Wf - g, -1.f), 1.f);
          }
          if (q) {
            da -= cqa * (double)(th - (g - va < 0.f ? 1.f : 0.f));
            db -= cqb * (double)(th1 - (g - vb < 0.f ? 1.f : 0.f));
          }
          acc_a += da * wgt;
          acc_b += db * wgt;
        }
      }
    }
  }
  for (int o = G >> 1; o > 0; o >>= 1) {   // a fixed butterfly inside the pixel's 2^lg lanes
    acc_a += __shfl_xor(acc_a, o, 64);
    if (range) acc_b += __shfl_xor(acc_b, o, 64);
  }
  if (valid && g_lane == 0) {
    const double scale = (double)W / (double)w;
    const size_t at = (size_t)b * h * w + (size_t)i * w + j;
    it.ga[at] = (float)(acc_a * scale);
    if (range) it.gb[at] = (float)(acc_b * scale);
  }
}

__global__ __launch_bounds__(LOSS_BLOCK) void quantile_loss_bwd_kernel(const float* __restrict__ mn, const float* __restrict__ mx,
                                                                       const float* __restrict__ gt, const double* __restrict__ stats,
                                                                       const float* __restrict__ grad_out, float* __restrict__ gmn,
                                                                       float* __restrict__ gmx, long long n, float q_lo, float q_hi,
                                                                       float th, float th1) {
#pragma clang fp contract(off)
  const long long i = blockIdx.x * (long long)LOSS_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double nq = stats[1];
  const float g = gt[i];
  float a = 0.f, b = 0.f;
  if (g > q_lo && g < q_hi && nq > 0.0) {
    a = (float)(-(double)grad_out[0] / nq * (double)(th - (g - mn[i] < 0.f ? 1.f : 0.f)));
    b = (float)(-(double)grad_out[1] / nq * (double)(th1 - (g - mx[i] < 0.f ? 1.f : 0.f)));
  }
  gmn[i] = a;
  gmx[i] = b;
}

static int lanes_log2(int in, int out) {   // the smallest power of two that covers the footprint's width in one step, at most a wave
  const int width = 2 * cdiv(out, in) + 4;   // (footprint() below: 2 * out / in, rounded outwards, and one more on either side)
  int lg = 0;
  while ((1 << lg) < width && lg < 6) ++lg;
  return lg;
}

// Shared validation: the K list maps, the range maps, the extents.  Fills the maps; returns DMB_OK or the failure.
// ``msgs``: the entry point's own messages (the last error keeps the pointer, so they are literals).
struct DeepPrunerLossMsgs {
  const char *list, *argument, *map, *large;
};
static int fill_maps(const DeepPrunerLossMsgs& msgs, const float* const* d, const int* h_host, const int* w_host,
                     const float* min_disp, const float* max_disp, int K, int B, int h, int w, int H, int W, DeepPrunerLossMaps& m) {
  if (K < 1 || K > DL_MAXK) return fail(DMB_EUNSUPPORTED, msgs.list);
  if (!h_host || !w_host || !min_disp || !max_disp || B <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, msgs.argument);
  for (int k = 0; k < DL_MAXK + 2; ++k) {
    m.d[k] = nullptr;
    m.h[k] = m.w[k] = 1;
  }
  for (int k = 0; k < K; ++k) {
    if (!d[k] || h_host[k] <= 0 || w_host[k] <= 0) return fail(DMB_EINVAL, msgs.map);
    m.d[k] = d[k];
    m.h[k] = h_host[k];
    m.w[k] = w_host[k];
  }
  m.d[K] = min_disp;
  m.d[K + 1] = max_disp;
  m.h[K] = m.h[K + 1] = h;
  m.w[K] = m.w[K + 1] = w;
  // a batch item of every map stays below 2 GiB, so that every index inside an item fits 31 bits
  for (int k = 0; k < K + 2; ++k)
    if (4LL * m.h[k] * m.w[k] >= 0x80000000LL) return fail(DMB_EUNSUPPORTED, msgs.large);
  if (4LL * H * W >= 0x80000000LL) return fail(DMB_EUNSUPPORTED, msgs.large);
  for (int k = 0; k < DL_MAXK + 2; ++k) {
    m.sh[k] = hp_scale(m.h[k], H);
    m.sw[k] = hp_scale(m.w[k], W);
  }
  return DMB_OK;
}
static const DeepPrunerLossMsgs FWD_MSGS = {"deeppruner_loss_fwd: 1 .. 3 maps in the list", "deeppruner_loss_fwd: bad argument",
                                            "deeppruner_loss_fwd: bad map", "deeppruner_loss_fwd: map too large"};
static const DeepPrunerLossMsgs BWD_MSGS = {"deeppruner_loss_bwd: 1 .. 3 maps in the list", "deeppruner_loss_bwd: bad argument",
                                            "deeppruner_loss_bwd: bad map", "deeppruner_loss_bwd: map too large"};

static bool theta_ok(double theta) { return theta > 0.0 && theta < 1.0; }   // (false for a NaN)

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_deeppruner_loss_fwd_f32(const float* d0, const float* d1, const float* d2, const int* h_host, const int* w_host,
                                           const float* min_disp, const float* max_disp, const float* gt, double* workspace,
                                           float* loss_out, double* stats, int K, int B, int h, int w, int H, int W, float l1_lower,
                                           float l1_upper, float q_lower, float q_upper, double theta, void* stream) {
  const float* d[DL_MAXK] = {d0, d1, d2};
  DeepPrunerLossMaps m;
  if (int e = fill_maps(FWD_MSGS, d, h_host, w_host, min_disp, max_disp, K, B, h, w, H, W, m)) return e;
  if (!gt || !workspace || !loss_out || !stats || !theta_ok(theta)) return fail(DMB_EINVAL, "deeppruner_loss_fwd: bad argument");
  const int tiles_x = cdiv(W, DL_TW), tiles_y = cdiv(H, DL_TH);
  const long long ntiles = (long long)B * tiles_y * tiles_x;
  const int nblk = (int)(ntiles < DL_MAX_BLOCKS ? ntiles : DL_MAX_BLOCKS);
  const float th = (float)theta, th1 = (float)(1.0 - theta);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(nblk), block(LOSS_BLOCK);
  switch (K) {
    case 1:
      hipLaunchKernelGGL(deeppruner_loss_fwd_kernel<1>, grid, block, 0, st, m, gt, workspace, B, H, W, tiles_x, tiles_y, l1_lower,
                         l1_upper, q_lower, q_upper, th, th1);
      break;
    case 2:
      hipLaunchKernelGGL(deeppruner_loss_fwd_kernel<2>, grid, block, 0, st, m, gt, workspace, B, H, W, tiles_x, tiles_y, l1_lower,
                         l1_upper, q_lower, q_upper, th, th1);
      break;
    default:
      hipLaunchKernelGGL(deeppruner_loss_fwd_kernel<3>, grid, block, 0, st, m, gt, workspace, B, H, W, tiles_x, tiles_y, l1_lower,
                         l1_upper, q_lower, q_upper, th, th1);
      break;
  }
  hipLaunchKernelGGL(deeppruner_loss_finalize_kernel, dim3(1), block, 0, st, workspace, nblk, K + 2, loss_out, stats);
  return launch_status("deeppruner_loss_fwd launch failed");
}

extern "C" int dmb_deeppruner_loss_bwd_f32(const float* d0, const float* d1, const float* d2, const int* h_host, const int* w_host,
                                           const float* min_disp, const float* max_disp, const float* gt, const double* stats,
                                           const float* grad_out, float* grad_d0, float* grad_d1, float* grad_d2, float* grad_min,
                                           float* grad_max, int K, int B, int h, int w, int H, int W, float l1_lower, float l1_upper,
                                           float q_lower, float q_upper, double theta, void* stream) {
  const float* d[DL_MAXK] = {d0, d1, d2};
  float* gd[DL_MAXK] = {grad_d0, grad_d1, grad_d2};
  DeepPrunerLossMaps m;
  if (int e = fill_maps(BWD_MSGS, d, h_host, w_host, min_disp, max_disp, K, B, h, w, H, W, m)) return e;
  if (!gt || !stats || !grad_out || !grad_min || !grad_max || !theta_ok(theta))
    return fail(DMB_EINVAL, "deeppruner_loss_bwd: bad argument");
  for (int k = 0; k < K; ++k)
    if (!gd[k]) return fail(DMB_EINVAL, "deeppruner_loss_bwd: bad gradient map");
  DeepPrunerLossTable tb;
  tb.n = K + 1;
  long long blocks = 0;
  for (int k = 0; k < DL_MAXK + 1; ++k) {
    DeepPrunerLossItem& it = tb.it[k];
    const int s = k < K ? k : K;          // the unused entries repeat the range item and are never selected
    it.a = m.d[s];
    it.b = k < K ? nullptr : m.d[K + 1];
    it.ga = k < K ? gd[k] : grad_min;
    it.gb = k < K ? nullptr : grad_max;
    it.h = m.h[s];
    it.w = m.w[s];
    it.sh = m.sh[s];
    it.sw = m.sw[s];
    it.lg = lanes_log2(it.w, W);
    it.tiles_x = cdiv(it.w, 64 >> it.lg);
    it.tiles_y = cdiv(it.h, 4);
    it.slot = s;
    it.first_block = (int)blocks;
    if (k <= K) blocks += (long long)B * it.tiles_y * it.tiles_x;
    if (blocks > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "deeppruner_loss_bwd: grid too large");
  }
  hipLaunchKernelGGL(deeppruner_loss_bwd_kernel, dim3((unsigned)blocks), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, tb, gt, stats,
                     grad_out, K, H, W, l1_lower, l1_upper, q_lower, q_upper, (float)theta, (float)(1.0 - theta));
  return launch_status("deeppruner_loss_bwd launch failed");
}

extern "C" int dmb_quantile_loss_fwd_f32(const float* min_disp, const float* max_disp, const float* gt, double* workspace,
                                         float* loss_out, double* stats, int B, int H, int W, float q_lower, float q_upper,
                                         double theta, void* stream) {
  if (!min_disp || !max_disp || !gt || !workspace || !loss_out || !stats || B <= 0 || H <= 0 || W <= 0 || !theta_ok(theta))
    return fail(DMB_EINVAL, "quantile_loss_fwd: bad argument");
  if (4LL * H * W >= 0x80000000LL) return fail(DMB_EUNSUPPORTED, "quantile_loss_fwd: map too large");
  const long long n = (long long)B * H * W, want = (n + LOSS_BLOCK - 1) / LOSS_BLOCK;
  const int nblk = (int)(want < DL_MAX_BLOCKS ? want : DL_MAX_BLOCKS);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(quantile_loss_fwd_kernel, dim3(nblk), dim3(LOSS_BLOCK), 0, st, min_disp, max_disp, gt, workspace, n, q_lower,
                     q_upper, (float)theta, (float)(1.0 - theta));
  hipLaunchKernelGGL(deeppruner_loss_finalize_kernel, dim3(1), dim3(LOSS_BLOCK), 0, st, workspace, nblk, 0, loss_out, stats);
  return launch_status("quantile_loss_fwd launch failed");
}

extern "C" int dmb_quantile_loss_bwd_f32(const float* min_disp, const float* max_disp, const float* gt, const double* stats,
                                         const float* grad_out, float* grad_min, float* grad_max, int B, int H, int W,
                                         float q_lower, float q_upper, double theta, void* stream) {
  if (!min_disp || !max_disp || !gt || !stats || !grad_out || !grad_min || !grad_max || B <= 0 || H <= 0 || W <= 0 || !theta_ok(theta))
    return fail(DMB_EINVAL, "quantile_loss_bwd: bad argument");
  if (4LL * H * W >= 0x80000000LL) return fail(DMB_EUNSUPPORTED, "quantile_loss_bwd: map too large");
  const long long n = (long long)B * H * W, nblk = (n + LOSS_BLOCK - 1) / LOSS_BLOCK;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "quantile_loss_bwd: grid too large");
  hipLaunchKernelGGL(quantile_loss_bwd_kernel, dim3((unsigned)nblk), dim3(LOSS_BLOCK), 0, (hipStream_t)stream, min_disp, max_disp, gt,
                     stats, grad_out, grad_min, grad_max, n, q_lower, q_upper, (float)theta, (float)(1.0 - theta));
  return launch_status("quantile_loss_bwd launch failed");
}
