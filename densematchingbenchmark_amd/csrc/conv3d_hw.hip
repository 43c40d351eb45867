// 3-D convolutions that stride the (y, x) plane only: the layers of DeepPruner's HWHourglass
// (reference cost_processors/utils/hw_hourglass.py:31-74, aggregators/DeepPruner.py:34-37) as FP32 implicit GEMMs.
//
//   MODE 0   Conv3d k3 p1 stride 1                                  Co = 16 (the widths 32 / 64 / 128 stay on conv3d_s1s2.hip)
//   MODE 1   Conv3d k3 p1 stride (1, 2, 2)                          Co = 16, 32, 64, 128
//   MODE 2   ConvTranspose3d k3 p1 stride (1, 2, 2) out_pad (0,1,1) Co = 16, 32, 64
//
// Same roles as conv3d.hip: v_mfma_f32_32x32x2_f32 (exact FP32, an fmaf chain in k order), A = packed weights (row = output
// channel, the stream of dmb_conv3d_pack_weights_f32 / dmb_deconv3d_pack_weights_f32 read as it is), B = input voxels (column =
// voxel).  Co = 16 is the 32-row stream with 16 zero rows: half of that tile's arithmetic is spent on zeros, none of its stores.
//
// These launches are small (the deepest level of one 544 x 960 pair is 9 x 17 x 30 = 4590 voxels at 128 channels), so the unit of
// work is as small as the instruction allows: ONE 32-voxel column tile x ONE 32-channel row tile per wave, every wave running the
// whole K chain of its tile (one chain per output voxel: pair of channels ascending, tap ascending, the two channels of the pair --
// the order of the packed stream and of the stride-1 / stride-2 kernels of conv3d_s1s2.hip, so a (1, 2, 2) result equals the stride-1
// result sampled at even (y, x) bit for bit, and a batch item equals the item run alone).  There is no split-K form here.
//
// Workgroup = 4 waves = WN row tiles x TZ = 4 / WN consecutive z-slices of one (y, x) patch of G columns x 32 / G rows (G = 32, 16
// or 8, whichever computes the fewest discarded voxels for the launch's width).  With stride 1 along z the TZ slices share their
// halo planes: TZ + 2 staged planes per channel.  Per chunk of 8 input channels the haloed patch is staged through registers into
// LDS with zero padding materialised (plain 4-byte loads: any alignment, any extent), then every wave runs 4 x 27 k-steps, each
// one 256-byte weight-fragment load (L2 resident; the fragments of the NEXT channel pair are in flight during the 27 MFMAs of the
// current one), one ds_read_b32 and one MFMA.
//
// LDS addressing makes a tap a compile-time offset for every lane:
//   MODE 0  plane [IY][P] in input order:                           tap (kd, ky, kx) = kd * PLANE + ky * P + kx
//   MODE 1  rows and columns de-interleaved by parity, [py][yy][px][xx]: input (2 oy + ky, 2 ox + kx) relative to the patch
//           origin lies at parity (ky & 1, kx & 1), index (oy + (ky >> 1), ox + (kx >> 1)) -- 32 lanes read 32 consecutive floats
//   MODE 2  a column is a position (gy, gx) of the INPUT grid and owns the four outputs (2 gy + qy, 2 gx + qx): tap ky = 1 feeds
//           the even rows from input row gy, ky = 2 the odd rows from gy, ky = 0 the odd rows from gy + 1 (x alike); along z the
//           layer is a stride-1 convolution with mirrored taps (id = od + 1 - kd).  Each of the 27 taps of a channel pair is one
//           MFMA into the accumulator of its parity class: 3 / 6 / 6 / 12 taps per class, four independent chains per wave.
#include "dmb_common.h"

namespace dmb {

template <int MODE_, int G_, int WN_>
struct HwCfg {
  static constexpr int MODE = MODE_, G = G_, WN = WN_;
  static constexpr int RY = 32 / G;        // rows of a column tile
  static constexpr int TZ = 4 / WN;        // z-slices per workgroup, one per wave
  static constexpr int ZS = TZ + 2;        // staged planes per channel
  static constexpr int CK = 8;             // input channels per chunk (the packed stream pads Ci to a multiple of 8)
  // staged patch of one (channel, z) plane in input coordinates
  static constexpr int IY = MODE == 0 ? RY + 2 : (MODE == 1 ? 2 * RY + 1 : RY + 1);
  static constexpr int IX = MODE == 0 ? G + 2 : (MODE == 1 ? 2 * G + 1 : G + 1);
  static constexpr int P = MODE == 1 ? G + 1 : IX;
  static constexpr int PLANE = MODE == 1 ? 4 * (RY + 1) * P : IY * P;
  static constexpr int CHS = ZS * PLANE;
  static constexpr int LDS_FLOATS = CK * CHS;
  static constexpr int NACC = MODE == 2 ? 4 : 1;
  static constexpr int EPP = (IY * IX + 63) / 64;   // staging instructions per plane
  static constexpr int PPW = CK * ZS / 4;           // planes per wave
  static_assert(LDS_FLOATS * 4 <= 64 * 1024, "static LDS");
  __host__ __device__ static constexpr int lds_pos(int ly, int lx) {
    return MODE == 1 ? (((ly & 1) * (RY + 1) + (ly >> 1)) * 2 + (lx & 1)) * P + (lx >> 1) : ly * P + lx;
  }
  __host__ __device__ static constexpr int lane_base(int ry, int rx) { return MODE == 1 ? 2 * ry * P + rx : ry * P + rx; }
  __host__ __device__ static constexpr int tap_off(int kd, int ky, int kx) {
    return MODE == 2 ? (2 - kd) * PLANE + (ky == 0 ? P : 0) + (kx == 0 ? 1 : 0) : kd * PLANE + lds_pos(ky, kx);
  }
  __host__ __device__ static constexpr int tap_acc(int ky, int kx) { return MODE == 2 ? (ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0) : 0; }
};

// Ho, Wo: extent of the plane the columns walk -- the output plane (MODE 0 / 1) or the input grid (MODE 2).
template <class C>
__global__ __launch_bounds__(256) void conv3d_hw_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        const float* __restrict__ res, float* __restrict__ y, int Ci, int Co,
                                                        int D, int H, int W, int Ho, int Wo, int ntx, int nty, int ntz, int relu) {
  __shared__ float lds[C::LDS_FLOATS];
  int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz;
  const int b = t / ntz;
  const int ox0 = tx * C::G, oy0 = ty * C::RY, z0 = tz * C::TZ;
  const int ix0 = C::MODE == 0 ? ox0 - 1 : (C::MODE == 1 ? 2 * ox0 - 1 : ox0);
  const int iy0 = C::MODE == 0 ? oy0 - 1 : (C::MODE == 1 ? 2 * oy0 - 1 : oy0);

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j = lane & 31, h = lane >> 5;
  const int nt = wave % C::WN, wz = wave / C::WN;
  const int ry = j / C::G, rx = j % C::G;
  const size_t HW = (size_t)H * W;
  const float* xb = x + (size_t)b * Ci * D * HW;

  const int nkp = (Ci + 7) / 8 * 4;   // channel pairs of the packed stream
  const float* wl = wp + (size_t)nt * 64 + lane;
  const size_t wtap = (size_t)C::WN * 64;   // floats between the fragments of two taps (WN = row tiles of the layer)

  f32x16 acc[C::NACC];
#pragma unroll
  for (int q = 0; q < C::NACC; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;

  float an[27];   // weight fragments of the next channel pair
#pragma unroll
  for (int tp = 0; tp < 27; ++tp) an[tp] = wl[tp * wtap];

  const bool zactive = z0 + wz < D;   // a wave beyond the volume still stages and meets the barriers
  const int bbase = h * C::CHS + wz * C::PLANE + C::lane_base(ry, rx);

  for (int c0 = 0, kp = 0; c0 < Ci; c0 += C::CK) {
    if (c0) __syncthreads();
    // ---- stage [CK][ZS] planes, dealt to the waves; a plane = IY rows of IX floats in memory order (coalesced), zeros outside
#pragma unroll
    for (int q = 0; q < C::PPW; ++q) {
      const int pl = wave * C::PPW + q, cl = pl / C::ZS, lz = pl - cl * C::ZS;
      const int gz = z0 - 1 + lz;
      const bool zok = c0 + cl < Ci && gz >= 0 && gz < D;
      const float* src = xb + ((size_t)(zok ? c0 + cl : 0) * D + (zok ? gz : 0)) * HW;
      float* dst = lds + cl * C::CHS + lz * C::PLANE;
#pragma unroll
      for (int e = 0; e < C::EPP; ++e) {
        const int i = e * 64 + lane;
        const int ly = i / C::IX, lx = i - ly * C::IX;
        const int gy = iy0 + ly, gx = ix0 + lx;
        const bool ok = zok && i < C::IY * C::IX && gy >= 0 && gy < H && gx >= 0 && gx < W;
        const float v = ok ? src[(size_t)gy * W + gx] : 0.f;
        if (i < C::IY * C::IX) dst[C::lds_pos(ly, lx)] = v;
      }
    }
    __syncthreads();
    // ---- 4 channel pairs x 27 taps
    for (int kl = 0; kl < C::CK / 2; ++kl, ++kp) {
      float a[27];
#pragma unroll
      for (int tp = 0; tp < 27; ++tp) a[tp] = an[tp];
      const int kn = kp + 1 < nkp ? kp + 1 : kp;
      const float* wn = wl + (size_t)kn * 27 * wtap;
#pragma unroll
      for (int tp = 0; tp < 27; ++tp) an[tp] = wn[tp * wtap];
      if (zactive) {
        const float* bp = lds + bbase + 2 * kl * C::CHS;
#pragma unroll
        for (int tp = 0; tp < 27; ++tp) {
          const int kd = tp / 9, ky = (tp / 3) % 3, kx = tp % 3;
          const float bv = bp[C::tap_off(kd, ky, kx)];
          acc[C::tap_acc(ky, kx)] = DMB_MFMA(a[tp], bv, acc[C::tap_acc(ky, kx)]);
        }
      }
    }
  }

  // ---- epilogue: affine, ReLU mode 2, residual, ReLU mode 1 (include/dmb_hip.h)
  const int od = z0 + wz, py = oy0 + ry, px = ox0 + rx;
  if (!zactive || py >= Ho || px >= Wo) return;
  const int OH = C::MODE == 2 ? 2 * Ho : Ho, OW = C::MODE == 2 ? 2 * Wo : Wo;
  const size_t cstride = (size_t)D * OH * OW;
  const size_t o0 = (size_t)b * Co * cstride + (size_t)od * OH * OW +
                    (C::MODE == 2 ? (size_t)(2 * py) * OW + 2 * px : (size_t)py * OW + px);
  // MODE 2: the two x-parities of a lane are neighbours in memory, at an even float offset of y (2 px, even rows, even planes):
  // one 8-byte store (and residual load) per pair when the bases are 8-byte aligned, 4-byte ones otherwise
  const bool vec2 = C::MODE == 2 && ((reinterpret_cast<size_t>(y) | reinterpret_cast<size_t>(res)) & 7) == 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = nt * 32 + cd_row(r, h);
    if (co >= Co) continue;
    const float sc = scale ? scale[co] : 1.f, sh = shift ? shift[co] : 0.f;
    const size_t oc = o0 + (size_t)co * cstride;
    float v[C::NACC];
#pragma unroll
    for (int q = 0; q < C::NACC; ++q) {
      v[q] = fmaf(acc[q][r], sc, sh);
      if (relu == 2) v[q] = fmaxf(v[q], 0.f);
    }
    if constexpr (C::MODE == 2) {
#pragma unroll
      for (int qy = 0; qy < 2; ++qy) {
        const size_t o = oc + (size_t)qy * OW;
        float a = v[2 * qy], b = v[2 * qy + 1];
        if (res) {
          if (vec2) {
            const float2 t2 = *reinterpret_cast<const float2*>(res + o);
            a += t2.x;
            b += t2.y;
          } else {
            a += res[o];
            b += res[o + 1];
          }
        }
        if (relu == 1) a = fmaxf(a, 0.f), b = fmaxf(b, 0.f);
        if (vec2) {
          *reinterpret_cast<float2*>(y + o) = make_float2(a, b);
        } else {
          y[o] = a;
          y[o + 1] = b;
        }
      }
    } else {
      float a = v[0];
      if (res) a += res[oc];
      if (relu == 1) a = fmaxf(a, 0.f);
      y[oc] = a;
    }
  }
}

template <int MODE, int G, int WN>
static int launch_hw(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B,
                     int Ci, int Co, int D, int H, int W, int Ho, int Wo, int relu, hipStream_t st) {
  using C = HwCfg<MODE, G, WN>;
  const int ntx = cdiv(Wo, C::G), nty = cdiv(Ho, C::RY), ntz = cdiv(D, C::TZ);
  const long long nblk = (long long)B * ntx * nty * ntz;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d_hw: grid too large");
  hipLaunchKernelGGL(conv3d_hw_kernel<C>, dim3((unsigned)nblk), dim3(256), 0, st, x, wp, scale, shift, res, y, Ci, Co, D, H, W, Ho,
                     Wo, ntx, nty, ntz, relu);
  return launch_status("conv3d_hw launch failed");
}

// Columns per tile row: the G whose tiles cover the (Ho, Wo) plane with the fewest computed voxels (ties: the wider rows, longer
// store runs).  Selected by the launch's extents only.
static int pick_g(int Ho, int Wo) {
  int best = 32;
  long long bc = -1;
  for (int g = 32; g >= 8; g >>= 1) {
    const long long c = (long long)cdiv(Wo, g) * cdiv(Ho, 32 / g);
    if (bc < 0 || c < bc) best = g, bc = c;
  }
  return best;
}

template <int MODE>
static int dispatch_hw(const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y, int B,
                       int Ci, int Co, int D, int H, int W, int Ho, int Wo, int relu, hipStream_t st) {
  const int g = pick_g(Ho, Wo), wn = cdiv(Co, 32);
#define DMB_HW(G, WN) \
  if (g == G && wn == WN) return launch_hw<MODE, G, WN>(x, wp, scale, shift, res, y, B, Ci, Co, D, H, W, Ho, Wo, relu, st)
  DMB_HW(32, 1);
  DMB_HW(16, 1);
  DMB_HW(8, 1);
  if constexpr (MODE != 0) {
    DMB_HW(32, 2);
    DMB_HW(16, 2);
    DMB_HW(8, 2);
  }
  if constexpr (MODE == 1) {
    DMB_HW(32, 4);
    DMB_HW(16, 4);
    DMB_HW(8, 4);
  }
#undef DMB_HW
  return fail(DMB_EUNSUPPORTED, "conv3d_hw: no kernel for this channel count");
}

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_conv3d_k3_hw_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                    const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int stride_hw,
                                    int relu, void* stream) {
  if (!x || !wpack || !y || B <= 0 || Ci <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "conv3d_hw: bad argument");
  const bool co_ok = stride_hw == 2 ? (Co == 16 || Co == 32 || Co == 64 || Co == 128) : (stride_hw == 1 && Co == 16);
  if (!co_ok)
    return fail(DMB_EUNSUPPORTED, "conv3d_hw: stride (1, 2, 2) with 16, 32, 64 or 128 output channels, or stride 1 with 16");
  relu &= 0xff;   // DMB_CONV_SINGLE_CHAIN: every launch of this family is one chain per voxel
  if (relu > 2) return fail(DMB_EINVAL, "conv3d_hw: relu must be 0, 1 or 2");
  hipStream_t st = (hipStream_t)stream;
  if (stride_hw == 1) return dispatch_hw<0>(x, wpack, scale, shift, residual, y, B, Ci, Co, D, H, W, H, W, relu, st);
  return dispatch_hw<1>(x, wpack, scale, shift, residual, y, B, Ci, Co, D, H, W, (H - 1) / 2 + 1, (W - 1) / 2 + 1, relu, st);
}

extern "C" int dmb_deconv3d_k3_hw_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                      const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int relu,
                                      void* stream) {
  if (!x || !wpack || !y || B <= 0 || Ci <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "deconv3d_hw: bad argument");
  if (Co != 16 && Co != 32 && Co != 64) return fail(DMB_EUNSUPPORTED, "deconv3d_hw: 16, 32 or 64 output channels");
  relu &= 0xff;
  if (relu > 2) return fail(DMB_EINVAL, "deconv3d_hw: relu must be 0, 1 or 2");
  return dispatch_hw<2>(x, wpack, scale, shift, residual, y, B, Ci, Co, D, H, W, H, W, relu, (hipStream_t)stream);
}
