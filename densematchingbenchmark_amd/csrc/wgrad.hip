// Weight gradients of the 3x3x3 convolutions (training side) as FP32 implicit GEMMs on the matrix cores.
//
//   dW[co, ci, tap] = sum_{b, v} dc[b, co, v] * x[b, ci, S v + tap - 1]      (S = 1 here; M = co, N = ci, K = voxels)
//
// (dc = gradient with respect to the raw convolution output: torch.nn.grad.conv3d_weight.)  The GEMM is K-dominated --
// 25 M voxels against a 32 x 32 x 27 result -- so the result lives in registers for the whole launch and the two input
// tensors stream through LDS exactly once:
//   * a workgroup owns one (32 output channels x 32 input channels) block and walks (4 rows x 24 columns) columns of
//     the volume along z; wave w owns taps 7w .. 7w+6 (112 accumulator registers), every wave reads the same dc
//     fragment (A) and its taps' shifted x fragments (B) -- 8 ds_read_b32 per 7 MFMAs;
//   * x planes sit in a ring of four LDS slots (z - 1, z, z + 1 in use, z + 2 landing by LDS-DMA), so every plane is
//     staged once per column and not three times; dc planes are double buffered;
//   * an MFMA k-step multiplies two x-adjacent voxels (lanes 0-31: even column, lanes 32-63: odd); channel pitches
//     (196 / 100 floats) are = 4 mod 64 so that the 2 x 32 lanes of a fragment read fall 2-way on the banks;
//   * persistent launch (one workgroup per CU): partial results go to a workspace [slot][tap][32][32] and a second
//     kernel adds the slots in a fixed order -- no atomics, bit-reproducible.
//
// Reference semantics: autograd of nn.Conv3d in dmb/modeling/stereo/layers/basic_layers.py:68-83,160-177.
#include <tuple>
#include <utility>

#include "wgrad_plan.h"

namespace dmb {

template <int TX_>
struct WgCfg {
  static constexpr int TY = 4, TX = TX_, ROWS = TY + 2, XOFF = 3;
  static constexpr int P = (4 + TX + 1 + 3) / 4 * 4;            // staged row: aligned column x0 - 4 .. x0 + TX + 3
  static constexpr int SX = ROWS * P + 4, SD = TY * TX + 4;     // channel pitches (floats), = 4 mod 64
  static constexpr int XPLANE = 32 * SX, DPLANE = 32 * SD;
  static constexpr int NRING = 4;
  static constexpr int LDS_FLOATS = NRING * XPLANE + 2 * DPLANE;
  static constexpr int UX = ROWS * P / 4, UD = TY * TX / 4;     // 16-byte units per channel plane
  static constexpr int KSTEPS = TY * TX / 2;
  static constexpr int NTAPW = 7;                               // taps per wave (4 x 7 = 28 >= 27; the last one is a dummy)
  static_assert(SX % 8 == 4 && SD % 8 == 4 && UX <= 64 && UD <= 64 && LDS_FLOATS * 4 <= 160 * 1024, "tile");
};

// workspace layout: ws[((blk * nslots + slot) * 27 + tap) * 1024 + m * 32 + n], blk = cob * ncib + cib
template <bool V16, int TX_>
__global__ __launch_bounds__(256, 1) void conv3d_wgrad_s1_kernel(const float* __restrict__ x, const float* __restrict__ dc,
                                                                 float* __restrict__ ws, int B, int Ci, int Co, int D, int H,
                                                                 int W, int ntx, int nty, int nzs, int zseg) {
  typedef WgCfg<TX_> C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xring = lds;
  float* dbuf = lds + C::NRING * C::XPLANE;
  const int ncib = cdiv(Ci, 32);
  const int cib = blockIdx.y % ncib, cob = blockIdx.y / ncib;
  const int slot = xcd_remap(blockIdx.x, gridDim.x), nslots = gridDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = lane & 31, kk = lane >> 5;
  const unsigned HW = (unsigned)H * W, DHW = (unsigned)D * HW;
  const int items = B * nzs * nty * ntx;
  const int nci = min(32, Ci - cib * 32), nco = min(32, Co - cob * 32);   // real channels of this block

  f32x16 acc[C::NTAPW];
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  // this wave's taps: B-fragment offsets inside a plane and the plane (dz) they read
  int tapoff[C::NTAPW], tapdz[C::NTAPW];
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i) {
    const int t = min(wave * C::NTAPW + i, 26);
    tapdz[i] = t / 9;
    tapoff[i] = n * C::SX + kk + C::XOFF + ((t / 3) % 3) * C::P + (t % 3);
  }
  const int aoff = n * C::SD + kk;

  for (int it = slot; it < items; it += nslots) {
    int t = it;
    const int tx = t % ntx;
    t /= ntx;
    const int ty = t % nty;
    t /= nty;
    const int zs = t % nzs;
    const int b = t / nzs;
    const int x0 = tx * C::TX, y0 = ty * C::TY, za = zs * zseg, zb = min(D, za + zseg);
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(x + ((size_t)b * Ci + cib * 32) * DHW, (unsigned)nci * DHW * 4u);
    const __amdgpu_buffer_rsrc_t drs = make_rsrc(dc + ((size_t)b * Co + cob * 32) * DHW, (unsigned)nco * DHW * 4u);
    // per-lane (row, unit) of the two staging patterns; the plane and the channel are wave-uniform scalar offsets
    unsigned xvo, dvo;
    {
      const int row = lane / (C::P / 4), un = lane % (C::P / 4);
      const int gy = y0 - 1 + row, gx = x0 - 4 + 4 * un;
      xvo = (lane < C::UX && gy >= 0 && gy < H && gx >= 0 && gx < W) ? ((unsigned)gy * W + (unsigned)gx) * 4u : DMA_OOB;
      const int drow = lane / (C::TX / 4), dun = lane % (C::TX / 4);
      const int dgy = y0 + drow, dgx = x0 + 4 * dun;
      dvo = (lane < C::UD && dgy < H && dgx < W) ? ((unsigned)dgy * W + (unsigned)dgx) * 4u : DMA_OOB;
    }
    // (channels >= nci / nco fall outside the resource and read zeros; a plane outside the volume is written as zeros)
    // One staging step = one channel plane of x or dc (one 16-byte LDS-DMA instruction, or one per row with dword
    // copies).  Steps are dealt out between the k-steps of the multiply loop: a wave that issues its 16 copies in one go
    // sits in the address queue for thousands of cycles while its SIMD's matrix core idles (one wave per SIMD here).
    auto stage_x1 = [&](int gz, int ring, int i) {
      const bool zok = gz >= 0 && gz < D;
      const int c = wave * 8 + i;
      float* dst = xring + ring * C::XPLANE + c * C::SX;
      if constexpr (V16) {
        if (lane < C::UX) dma16(xrs, zok ? xvo : DMA_OOB, zok ? ((unsigned)c * DHW + (unsigned)gz * HW) * 4u : 0u, dst);
      } else {
        const int gxs = x0 - 4 + lane;
        if (lane < C::P) {
#pragma unroll
          for (int row = 0; row < C::ROWS; ++row) {
            const int gy = y0 - 1 + row;
            const bool ok = zok && gy >= 0 && gy < H && gxs >= 0 && gxs < W;
            dma4(xrs, ok ? ((unsigned)gy * W + (unsigned)gxs) * 4u : DMA_OOB, ok ? ((unsigned)c * DHW + (unsigned)gz * HW) * 4u : 0u,
                 dst + row * C::P);
          }
        }
      }
    };
    auto stage_d1 = [&](int gz, int buf, int i) {
      const bool zok = gz >= 0 && gz < zb;
      const int c = wave * 8 + i;
      float* dst = dbuf + buf * C::DPLANE + c * C::SD;
      if constexpr (V16) {
        if (lane < C::UD) dma16(drs, zok ? dvo : DMA_OOB, zok ? ((unsigned)c * DHW + (unsigned)gz * HW) * 4u : 0u, dst);
      } else {
        const int gxs = x0 + lane;
        if (lane < C::TX) {
#pragma unroll
          for (int row = 0; row < C::TY; ++row) {
            const int gy = y0 + row;
            const bool ok = zok && gy < H && gxs < W;
            dma4(drs, ok ? ((unsigned)gy * W + (unsigned)gxs) * 4u : DMA_OOB, ok ? ((unsigned)c * DHW + (unsigned)gz * HW) * 4u : 0u,
                 dst + row * C::TX);
          }
        }
      }
    };
    auto stage_x = [&](int gz, int ring) {
#pragma unroll
      for (int i = 0; i < 8; ++i) stage_x1(gz, ring, i);
    };
    auto stage_d = [&](int gz, int buf) {
#pragma unroll
      for (int i = 0; i < 8; ++i) stage_d1(gz, buf, i);
    };

    // prologue: planes za - 1, za, za + 1 -> ring slots 0, 1, 2; dc plane za -> buffer 0
    __syncthreads();   // the previous column's last plane is still being read by slower waves
    stage_x(za - 1, 0);
    stage_x(za, 1);
    stage_x(za + 1, 2);
    stage_d(za, 0);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
    __syncthreads();
    for (int z = za; z < zb; ++z) {
      const int rel = z - za;   // plane z + dz - 1 sits in ring slot (rel + dz) % 4
      const bool more = z + 1 < zb;
      const float* ap = dbuf + (rel & 1) * C::DPLANE + aoff;
      const float* bp[C::NTAPW];
#pragma unroll
      for (int i = 0; i < C::NTAPW; ++i) bp[i] = xring + ((rel + tapdz[i]) & 3) * C::XPLANE + tapoff[i];
      float af[2], bf[2][C::NTAPW];
      auto load_frag = [&](int q, float& a, float (&bq)[C::NTAPW]) {
        const int r = q / (C::TX / 2), c2 = 2 * (q % (C::TX / 2));
        a = ap[r * C::TX + c2];
#pragma unroll
        for (int i = 0; i < C::NTAPW; ++i) bq[i] = bp[i][r * C::P + c2];
      };
      load_frag(0, af[0], bf[0]);
#pragma unroll
      for (int q = 0; q < C::KSTEPS; ++q) {
        if (q + 1 < C::KSTEPS) load_frag(q + 1, af[(q + 1) & 1], bf[(q + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < C::NTAPW; ++i) acc[i] = DMB_MFMA(af[q & 1], bf[q & 1][i], acc[i]);
        if (q % 2 == 0 && q / 2 < 16 && more) {   // the next planes, one copy every other k-step (KSTEPS >= 32)
          if (q / 2 < 8)
            stage_x1(z + 2, (rel + 3) & 3, q / 2);
          else
            stage_d1(z + 1, (rel + 1) & 1, q / 2 - 8);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      __builtin_amdgcn_s_waitcnt(0x0F70);   // the next planes have landed
      __syncthreads();                      // ... and everyone is done with the oldest ones
    }
  }

  // partial result of this slot
  float* wsb = ws + ((size_t)blockIdx.y * nslots + slot) * 27 * 1024;
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i) {
    const int t = wave * C::NTAPW + i;
    if (t < 27) {
#pragma unroll
      for (int r = 0; r < 16; ++r) wsb[t * 1024 + cd_row(r, kk) * 32 + n] = acc[i][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// Stride 2: out[cs, cb, tap] = sum_{b, o} small[b, cs, o] * big[b, cb, 2 o + tap - 1], the weight gradient of both
//   nn.Conv3d(stride 2):      small = dc [Co], big = x [Ci]   -> out = dW  [Co, Ci, 27]
//   nn.ConvTranspose3d(s 2):  small = x [Ci],  big = dy [Co]  -> out = dWt [Ci, Co, 27]
// Same structure as the stride-1 kernel; a small plane z needs big planes 2z - 1, 2z, 2z + 1 (ring of five slots, two
// landing per step); the tile is 2 rows x 12 columns of the small tensor (5 x 28 staged floats of the big one per
// channel); fragment reads of the big tile step 2 floats per k lane (bank pattern 12 n + 2 kk: still 2-way).
// Staging units are linear in LDS across channels (the unit count per channel is made odd: pitch = 4 mod 8 floats), so one LDS-DMA
// instruction moves 64 units whatever the plane size.
// ------------------------------------------------------------------------------------------------------------------
// Stride (1, 2, 2) (Db == Ds >= 2): out[cs, cb, kz, ky, kx] = sum small[b, cs, z, y, x] * big[b, cb, z + kz - 1, 2y + ky - 1,
// 2x + kx - 1] is the same kernel on WgHwCfg (ZS = 1): the staged tile, the pitches and the fragment reads are those of stride 2
// (the plane is strided the same way); only the ring (four slots, one landing) and the plane numbers of the walk differ.
// (round 6) The tile is a parameter: 2 x 12 (84 MFMAs per wave between two barriers) or 4 x 8 (112; and 64-column rows -- the
// training crops -- tile exactly where 12-column tiles compute 72); wgrad_plan picks per launch.
// ZS: the stride along z.  2 = the stride-2 units (Wg2Cfg).  1 = the units that stride only height and width (DeepPruner's
// hourglass, stride (1, 2, 2): WgHwCfg): the plane of the tile is the same, the walk along z is the stride-1 kernel's -- a small plane
// z needs big planes z - 1, z, z + 1: a ring of four slots with one landing per step.
template <int TY_, int TX_, int ZS_>
struct Wg2Tile {
  static constexpr int TY = TY_, TX = TX_, ZS = ZS_, ROWS = 2 * TY + 1, XOFF = 3;
  static constexpr int P = (4 + 2 * TX + 3) / 4 * 4;            // staged row of the big tile: aligned column 2 x0 - 4 ..
  static constexpr int UBU = ROWS * P / 4, USU = TY * TX / 4;   // 16-byte units per channel plane ...
  static constexpr int UB = UBU | 1, US = USU | 1;              // ... padded to an odd count (pitch = 4 mod 8 floats)
  static constexpr int SB = UB * 4, SS = US * 4;                // channel pitches (floats)
  static constexpr int BPLANE = 32 * SB, SPLANE = 32 * SS;
  static constexpr int NRING = 3 + ZS;                          // three big planes in use, ZS landing
  static constexpr int LDS_FLOATS = NRING * BPLANE + 2 * SPLANE;
  static constexpr int KSTEPS = TY * TX / 2;
  static constexpr int NTAPW = 7;
  static constexpr int IB = (32 * UB + 255) / 256, IS = (32 * US + 255) / 256;   // copy instructions per wave and plane
  static_assert(SB % 8 == 4 && SS % 8 == 4 && LDS_FLOATS * 4 <= 160 * 1024 && ZS * IB + IS <= KSTEPS && TX % 4 == 0 && (ZS == 1 || ZS == 2), "tile");
};

template <int TY_, int TX_>
struct Wg2Cfg : Wg2Tile<TY_, TX_, 2> {};
// Stride (1, 2, 2) has ONE tile, 4 x 8: the training shapes (small planes of 8 x 16, 16 x 32 and 32 x 64) tile exactly, and a wave
// issues 112 MFMAs between two barriers (2 x 12 would compute 24 columns for 16, 36 for 32, 72 for 64).
struct WgHwCfg : Wg2Tile<4, 8, 1> {};

template <class C, bool V16>
__global__ __launch_bounds__(256, 1) void conv3d_wgrad_s2_kernel(const float* __restrict__ sm, const float* __restrict__ bg,
                                                                 float* __restrict__ ws, int B, int Cs, int Cb, int Ds, int Hs,
                                                                 int Ws, int Db, int Hb, int Wb, int ntx, int nty, int nzs,
                                                                 int zseg) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* ring = lds;
  float* sbuf = lds + C::NRING * C::BPLANE;
  const int ncbb = cdiv(Cb, 32);
  const int cbb = blockIdx.y % ncbb, csb = blockIdx.y / ncbb;
  const int slot = xcd_remap(blockIdx.x, gridDim.x), nslots = gridDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = lane & 31, kk = lane >> 5;
  const unsigned HWs = (unsigned)Hs * Ws, DHWs = (unsigned)Ds * HWs, HWb = (unsigned)Hb * Wb, DHWb = (unsigned)Db * HWb;
  const int items = B * nzs * nty * ntx;
  const int ncs = min(32, Cs - csb * 32), ncb = min(32, Cb - cbb * 32);

  f32x16 acc[C::NTAPW];
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  int tapoff[C::NTAPW], tapdz[C::NTAPW];
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i) {
    const int t = min(wave * C::NTAPW + i, 26);
    tapdz[i] = t / 9;
    tapoff[i] = n * C::SB + 2 * kk + C::XOFF + ((t / 3) % 3) * C::P + (t % 3);
  }
  const int aoff = n * C::SS + kk;

  for (int it = slot; it < items; it += nslots) {
    int t = it;
    const int tx = t % ntx;
    t /= ntx;
    const int ty = t % nty;
    t /= nty;
    const int zs = t % nzs;
    const int b = t / nzs;
    const int x0 = tx * C::TX, y0 = ty * C::TY, za = zs * zseg, zb = min(Ds, za + zseg);
    const __amdgpu_buffer_rsrc_t brs = make_rsrc(bg + ((size_t)b * Cb + cbb * 32) * DHWb, (unsigned)ncb * DHWb * 4u);
    const __amdgpu_buffer_rsrc_t srs = make_rsrc(sm + ((size_t)b * Cs + csb * 32) * DHWs, (unsigned)ncs * DHWs * 4u);
    // per-lane source offsets (channel + in-plane part) of this wave's copy instructions; the plane is a scalar offset
    unsigned bvo[C::IB], svo[C::IS];
#pragma unroll
    for (int j = 0; j < C::IB; ++j) {
      const int u = (j * 4 + wave) * 64 + lane, ch = u / C::UB, un = u - ch * C::UB;
      const int row = un / (C::P / 4), cu = un - row * (C::P / 4);
      const int gy = 2 * y0 - 1 + row, gx = 2 * x0 - 4 + 4 * cu;
      const bool ok = ch < 32 && un < C::UBU && gy >= 0 && gy < Hb && gx >= 0 && gx < Wb;
      bvo[j] = ok ? ((unsigned)ch * DHWb + (unsigned)gy * Wb + (unsigned)gx) * 4u : DMA_OOB;
    }
#pragma unroll
    for (int j = 0; j < C::IS; ++j) {
      const int u = (j * 4 + wave) * 64 + lane, ch = u / C::US, un = u - ch * C::US;
      const int row = un / (C::TX / 4), cu = un - row * (C::TX / 4);
      const int gy = y0 + row, gx = x0 + 4 * cu;
      const bool ok = ch < 32 && un < C::USU && gy < Hs && gx < Ws;
      svo[j] = ok ? ((unsigned)ch * DHWs + (unsigned)gy * Ws + (unsigned)gx) * 4u : DMA_OOB;
    }
    auto stage_b1 = [&](int gz, int rslot, int j) {   // copy instruction j of this wave for big plane gz
      const bool zok = gz >= 0 && gz < Db;
      const int first = (j * 4 + wave) * 64;
      if (first + lane < 32 * C::UB) dma16(brs, zok ? bvo[j] : DMA_OOB, zok ? (unsigned)gz * HWb * 4u : 0u, ring + rslot * C::BPLANE + first * 4);
    };
    auto stage_s1 = [&](int gz, int buf, int j) {
      const bool zok = gz >= 0 && gz < zb;
      const int first = (j * 4 + wave) * 64;
      if (first + lane < 32 * C::US) dma16(srs, zok ? svo[j] : DMA_OOB, zok ? (unsigned)gz * HWs * 4u : 0u, sbuf + buf * C::SPLANE + first * 4);
    };
    // widths that are not multiples of 4: whole planes with dword copies, one staged row per instruction (slow path)
    auto stage_b_rows = [&](int gz, int rslot) {
      const bool zok = gz >= 0 && gz < Db;
      const int gx = 2 * x0 - 4 + lane;
      if (lane < C::P) {
        for (int i = 0; i < 8; ++i) {
          const int c = wave * 8 + i;
#pragma unroll
          for (int row = 0; row < C::ROWS; ++row) {
            const int gy = 2 * y0 - 1 + row;
            const bool ok = zok && gy >= 0 && gy < Hb && gx >= 0 && gx < Wb;
            dma4(brs, ok ? ((unsigned)gy * Wb + (unsigned)gx) * 4u : DMA_OOB, ok ? ((unsigned)c * DHWb + (unsigned)gz * HWb) * 4u : 0u,
                 ring + rslot * C::BPLANE + c * C::SB + row * C::P);
          }
        }
      }
    };
    auto stage_s_rows = [&](int gz, int buf) {
      const bool zok = gz >= 0 && gz < zb;
      const int gx = x0 + lane;
      if (lane < C::TX) {
        for (int i = 0; i < 8; ++i) {
          const int c = wave * 8 + i;
#pragma unroll
          for (int row = 0; row < C::TY; ++row) {
            const int gy = y0 + row;
            const bool ok = zok && gy < Hs && gx < Ws;
            dma4(srs, ok ? ((unsigned)gy * Ws + (unsigned)gx) * 4u : DMA_OOB, ok ? ((unsigned)c * DHWs + (unsigned)gz * HWs) * 4u : 0u,
                 sbuf + buf * C::SPLANE + c * C::SS + row * C::TX);
          }
        }
      }
    };
    // ring slot of big plane p: (p - (ZS za - 1)) % NRING
    __syncthreads();
    if constexpr (V16) {
#pragma unroll
      for (int q = 0; q < 3; ++q)
#pragma unroll
        for (int j = 0; j < C::IB; ++j) stage_b1(C::ZS * za - 1 + q, q, j);
#pragma unroll
      for (int j = 0; j < C::IS; ++j) stage_s1(za, 0, j);
    } else {
      for (int q = 0; q < 3; ++q) stage_b_rows(C::ZS * za - 1 + q, q);
      stage_s_rows(za, 0);
    }
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int q0 = 0;   // ring index of plane ZS z - 1
    for (int z = za; z < zb; ++z) {
      const int rel = z - za;
      const bool more = z + 1 < zb;
      const float* ap = sbuf + (rel & 1) * C::SPLANE + aoff;
      const float* bp[C::NTAPW];
#pragma unroll
      for (int i = 0; i < C::NTAPW; ++i) bp[i] = ring + ((q0 + tapdz[i]) % C::NRING) * C::BPLANE + tapoff[i];
      const int s3 = (q0 + 3) % C::NRING, s4 = (q0 + 4) % C::NRING;
      if constexpr (!V16) {
        if (more) {   // the planes the next step adds: ZS (z + 1) + 1 and, with a z stride, the one before it
          stage_b_rows(C::ZS * z + 2, s3);
          if constexpr (C::ZS == 2) stage_b_rows(2 * z + 3, s4);
          stage_s_rows(z + 1, (rel + 1) & 1);
        }
      }
      float af[2], bf[2][C::NTAPW];
      auto load_frag = [&](int q, float& a, float (&bq)[C::NTAPW]) {
        const int r = q / (C::TX / 2), c = q % (C::TX / 2);
        a = ap[r * C::TX + 2 * c];
#pragma unroll
        for (int i = 0; i < C::NTAPW; ++i) bq[i] = bp[i][2 * r * C::P + 4 * c];
      };
      load_frag(0, af[0], bf[0]);
#pragma unroll
      for (int q = 0; q < C::KSTEPS; ++q) {
        if (q + 1 < C::KSTEPS) load_frag(q + 1, af[(q + 1) & 1], bf[(q + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < C::NTAPW; ++i) acc[i] = DMB_MFMA(af[q & 1], bf[q & 1][i], acc[i]);
        if (V16 && more) {   // the next planes, one copy per k-step
          if (q < C::IB)
            stage_b1(C::ZS * z + 2, s3, q);
          else if (C::ZS == 2 && q < 2 * C::IB)
            stage_b1(2 * z + 3, s4, q - C::IB);
          else if (q >= C::ZS * C::IB && q < C::ZS * C::IB + C::IS)
            stage_s1(z + 1, (rel + 1) & 1, q - C::ZS * C::IB);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      q0 = (q0 + C::ZS) % C::NRING;
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
  }

  float* wsb = ws + ((size_t)blockIdx.y * nslots + slot) * 27 * 1024;
#pragma unroll
  for (int i = 0; i < C::NTAPW; ++i) {
    const int t = wave * C::NTAPW + i;
    if (t < 27) {
#pragma unroll
      for (int r = 0; r < 16; ++r) wsb[t * 1024 + cd_row(r, kk) * 32 + n] = acc[i][r];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------------
// One output channel (the classifier heads, nn.Conv3d(C, 1, 3, 1, 1)): dw[ci, tap] = sum_u x[ci, u] * dy[u - tap + 1].
// Round 5: on the matrix cores.  It is a GEMM with M = 32 input channels, N = 27 taps (one 32 x 32 tile) and K = the voxels:
// A[ci][u] = x[ci][u], B[u][tap] = dy[u - tap + 1] -- the 27 shifted views of ONE small dy neighbourhood.  A workgroup walks
// tiles of 4 rows x 64 columns of one (b, z) plane, one row per wave: the x tile (32 channels x 4 x 64, read coalesced, 256 B per
// channel row) and the dy neighbourhood (3 planes x 6 rows x 66 columns) are fetched into registers one tile AHEAD, committed to
// LDS between two barriers, and a wave then issues 32 MFMAs (two voxels per k-step) whose A / B operands are single LDS dwords
// (x pitch 65: conflict-free; taps 27 .. 31 read a zero row).  The round-1 form -- a VALU kernel, 27 address computations and
// cached loads per voxel and channel group -- ran at 0.11 of the HBM rate (0.30 ms per head at the training shape; rocprofv3,
// profiles/r05_train_pmc.csv): 10x the time of its one pass over x.  Partials per workgroup ([ci][tap], the four waves added in
// a fixed order) go to the workspace and are added in a fixed order in FP64 by the reduce kernel: bit-reproducible, no atomics.
// ------------------------------------------------------------------------------------------------------------------
constexpr int C1M_XT = 64, C1M_ROWS = 4, C1M_XP = C1M_XT + 1;        // tile columns, rows (= waves), LDS pitch of an x row
constexpr int C1M_DYP = 68, C1M_DYROWS = 3 * (C1M_ROWS + 2) + 1;     // dy neighbourhood: pitch, rows (+ 1 zero row)
constexpr int C1M_XS = C1M_ROWS * 32 * C1M_XP, C1M_DYS = C1M_DYROWS * C1M_DYP;
constexpr int C1M_XPT = C1M_ROWS * 32 * C1M_XT / 256;                // x words per thread and tile (32)
constexpr int C1M_DYN = 3 * (C1M_ROWS + 2) * (C1M_XT + 2);           // dy words per tile (1188)
constexpr int C1M_DPT = (C1M_DYN + 255) / 256;                       // ... per thread (5)
static_assert(C1M_XS >= 4 * 32 * 33, "the wave reduction reuses the x tile");

__global__ __launch_bounds__(256, 4) void conv3d_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                 float* __restrict__ ws, int B, int Ci, int D, int H, int W,
                                                                 int ntx, int nty, int ntiles) {
  __shared__ float xs[C1M_XS];
  __shared__ float dys[C1M_DYS];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int c0 = blockIdx.y * 32;
  const long long HW = (long long)H * W, DHW = (long long)D * HW;
  for (int i = tid; i < C1M_DYP; i += 256) dys[(C1M_DYROWS - 1) * C1M_DYP + i] = 0.f;   // the zero row (never overwritten)

  float xr[C1M_XPT], dr[C1M_DPT];
  auto fetch = [&](int t) {
    const int tx = t % ntx;
    int r = t / ntx;
    const int ty = r % nty;
    r /= nty;
    const int z = r % D, b = r / D;
    const int x0 = tx * C1M_XT, y0 = ty * C1M_ROWS;
    const float* xb = x + ((long long)b * Ci + c0) * DHW + (long long)z * HW;
#pragma unroll
    for (int q = 0; q < C1M_XPT; ++q) {
      const int idx = q * 256 + tid;                  // (row, channel, column): 64 consecutive lanes = one 256-byte run
      const int xx = idx & 63, ci = (idx >> 6) & 31, rr = idx >> 11;
      const int gy = y0 + rr, gx = x0 + xx;
      xr[q] = (c0 + ci < Ci && gy < H && gx < W) ? xb[(long long)ci * DHW + (long long)gy * W + gx] : 0.f;
    }
    const float* db = dy + (long long)b * DHW;
#pragma unroll
    for (int q = 0; q < C1M_DPT; ++q) {
      const int idx = q * 256 + tid;
      const int cc = idx % (C1M_XT + 2), r2 = idx / (C1M_XT + 2), rr = r2 % (C1M_ROWS + 2), zz = r2 / (C1M_ROWS + 2);
      const int gz = z - 1 + zz, gy = y0 - 1 + rr, gx = x0 - 1 + cc;
      dr[q] = (idx < C1M_DYN && gz >= 0 && gz < D && gy >= 0 && gy < H && gx >= 0 && gx < W) ? db[(long long)gz * HW + (long long)gy * W + gx] : 0.f;
    }
  };
  auto commit = [&]() {
#pragma unroll
    for (int q = 0; q < C1M_XPT; ++q) {
      const int idx = q * 256 + tid;
      xs[(idx >> 6) * C1M_XP + (idx & 63)] = xr[q];   // row index (rr * 32 + ci) = idx >> 6
    }
#pragma unroll
    for (int q = 0; q < C1M_DPT; ++q) {
      const int idx = q * 256 + tid;
      if (idx < C1M_DYN) dys[(idx / (C1M_XT + 2)) * C1M_DYP + idx % (C1M_XT + 2)] = dr[q];
    }
  };

  // operand addresses of this lane: A = x[channel i][voxel 2 s + k] of the wave's row, B = dy[voxel 2 s + k - tap j + 1]
  const int i = lane & 31, k = lane >> 5;
  const int tz = i / 9, tyy = (i / 3) % 3, txx = i % 3;
  const float* ap = xs + (wave * 32 + i) * C1M_XP + k;
  const float* bp = (i < 27) ? dys + ((2 - tz) * (C1M_ROWS + 2) + wave + 2 - tyy) * C1M_DYP + 2 - txx + k
                             : dys + (C1M_DYROWS - 1) * C1M_DYP + k;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  int t = blockIdx.x;
  if (t < ntiles) fetch(t);
  for (; t < ntiles; t += gridDim.x) {
    __syncthreads();          // every wave is done with the previous tile
    commit();
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) fetch(t + gridDim.x);   // lands while this tile is multiplied
#pragma unroll 8
    for (int s = 0; s < C1M_XT / 2; ++s) acc = DMB_MFMA(ap[2 * s], bp[2 * s], acc);
  }
  // the four waves' tiles, added in a fixed order (the x tile's LDS is free now)
  __syncthreads();
  float* red = xs;
#pragma unroll
  for (int r = 0; r < 16; ++r) red[(wave * 32 + cd_row(r, k)) * 33 + i] = acc[r];
  __syncthreads();
  for (int e = tid; e < 32 * 27; e += 256) {
    const int ci = e / 27, tp = e - ci * 27;
    if (c0 + ci < Ci)
      ws[((size_t)blockIdx.x * Ci + c0 + ci) * 27 + tp] =
          (red[ci * 33 + tp] + red[(32 + ci) * 33 + tp]) + (red[(64 + ci) * 33 + tp] + red[(96 + ci) * 33 + tp]);
  }
}

// One wave per number of the result ((channel, tap)): the lanes walk the workgroups' partials 64 apart (independent loads; one thread walking all of
// them alone was a chain of 256 .. 1024 dependent-latency loads, 63 us for 864 numbers), each in FP64, then a fixed butterfly.
// (n = Ci x 27 numbers per workgroup; the 5x5 form below: Co x Ci x 25 per slot; the 2-D one-channel form: Ci x 9)
__global__ __launch_bounds__(256) void wgrad_reduce_flat_kernel(const float* __restrict__ ws, float* __restrict__ dw, int n, int nchunk) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= n) return;
  double s = 0.0;
  for (int c = lane; c < nchunk; c += 64) s += (double)ws[(size_t)c * n + i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) dw[i] = (float)s;
}

// dw[co][ci][tap] = sum over slots in FP64, fixed order.  A workgroup owns 64 consecutive elements of one (block, tap) plane and
// its four waves a quarter of the slots each (eight interleaved partial sums per thread: independent loads), combined through LDS
// as (q0 + q1) + (q2 + q3).  (Rounds 1-5: one thread per element walked all 256 slots -- 32 dependent rounds of 8 loads, 9.2 us for
// 28 MB, 25 times per training step; more threads per element, not more bytes, is what it lacked.)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Co, int Ci, int nslots) {
  __shared__ double sm[4][64];
  const int ncib = cdiv(Ci, 32);
  const int e = threadIdx.x & 63, q = threadIdx.x >> 6;
  long long r = blockIdx.x;
  const int grp = (int)(r & 15);
  r >>= 4;
  const int t = (int)(r % 27);
  const int blk = (int)(r / 27);
  const int m = grp * 2 + (e >> 5), nn = e & 31;
  const int cib = blk % ncib, cob = blk / ncib;
  const int co = cob * 32 + m, ci = cib * 32 + nn;
  const float* p = ws + (size_t)blk * nslots * 27 * 1024 + t * 1024 + m * 32 + nn;
  const int per = (nslots + 3) / 4;
  const int s0 = q * per, s1 = s0 + per < nslots ? s0 + per : nslots;
  double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int sl = s0;
  for (; sl + 8 <= s1; sl += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) part[u] += (double)p[(size_t)(sl + u) * 27 * 1024];
  }
  for (int u = 0; sl < s1; ++sl, ++u) part[u] += (double)p[(size_t)sl * 27 * 1024];
  sm[q][e] = ((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7]));
  __syncthreads();
  if (q != 0 || co >= Co || ci >= Ci) return;
  const double s = (sm[0][e] + sm[1][e]) + (sm[2][e] + sm[3][e]);
  dw[((size_t)co * Ci + ci) * 27 + t] = (float)s;
}

// ------------------------------------------------------------------------------------------------------------------
// 2-D: dW[co, ci, tap] = sum_{b, p} dc[b, co, p] * x[b, ci, p + tap - 1] for nn.Conv2d(k 3, s 1, p 1) -- AcfNet's confidence
// heads (cmn/cmn.py:21-36: 192 -> 64 over the full-resolution cost volume).  Same idea as the 3-D kernel, one dimension down:
// a workgroup owns a (32 x 32) channel block and walks strips of 64 columns along y (in steps of the dilation: the image is
// `dilation` interleaved row classes, so a tap's rows are neighbours inside the class); x rows sit in a ring of four LDS slots,
// dc rows are double buffered; the four waves split the strip's columns (16 each) and each holds all nine taps (144
// accumulator registers); their partial results are added through LDS at the end, the slots' by the reduction kernel.
// ------------------------------------------------------------------------------------------------------------------
template <int KS_, int DIL_>
struct Wg2dCfg {
  static constexpr int KS = KS_, DIL = DIL_, NTAP = KS * KS;
  static constexpr int HALO = DIL * (KS / 2);                  // columns either side
  static constexpr int PAD = HALO <= 4 ? 4 : 8;                // the staged row starts at the aligned column x0 - PAD
  static constexpr int TX = 64, XOFF = PAD - HALO;
  // Rows are walked in steps of DIL (the image is DIL interleaved row classes; taps reach rows y - DIL, y, y + DIL = the
  // neighbours INSIDE the class), so the ring is four slots whatever the dilation: three in use, one landing.
  static constexpr int NR = KS == 1 ? 2 : 4;
  static constexpr int P = (PAD + TX + HALO + 3) / 4 * 4;
  static constexpr int UXU = P / 4, UDU = TX / 4;              // 16-byte units per channel row
  static constexpr int UX = UXU | 1, UD = UDU | 1;             // ... made odd: pitch = 4 mod 8 floats
  static constexpr int SX = UX * 4, SD = UD * 4;
  static constexpr int XROW = 32 * SX, DROW = 32 * SD;
  static constexpr int LDS_FLOATS = NR * XROW + 2 * DROW;
  static constexpr int IX = (32 * UX + 255) / 256, ID = (32 * UD + 255) / 256;   // copy instructions per wave and row
  static constexpr int KSTEPS = TX / 4 / 2;                    // per wave: 16 columns = 8 k-steps
  static_assert(HALO <= 8 && SX % 8 == 4 && SD % 8 == 4 && IX + ID <= KSTEPS && LDS_FLOATS * 4 * 2 <= 160 * 1024, "tile");
};

// nys: segments per row class; yseg: class rows per segment.  An item = (batch item, column strip, row class, segment).
template <int KS_, int DIL_>
__global__ __launch_bounds__(256, 2) void conv2d_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dc,
                                                              float* __restrict__ ws, int B, int Ci, int Co, int H, int W, int ntx,
                                                              int nys, int yseg) {
  typedef Wg2dCfg<KS_, DIL_> C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xring = lds;
  float* dbuf = lds + C::NR * C::XROW;
  const int ncib = cdiv(Ci, 32);
  const int cib = blockIdx.y % ncib, cob = blockIdx.y / ncib;
  const int slot = xcd_remap(blockIdx.x, gridDim.x), nslots = gridDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int n = lane & 31, kk = lane >> 5;
  const unsigned HW = (unsigned)H * W;
  const int items = B * nys * C::DIL * ntx;
  const int nci = min(32, Ci - cib * 32), nco = min(32, Co - cob * 32);
  constexpr int RH = C::KS / 2;   // class rows either side (0 or 1)

  f32x16 acc[C::NTAP];
#pragma unroll
  for (int i = 0; i < C::NTAP; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  const int aoff = n * C::SD + wave * 16 + kk;
  const int boff = n * C::SX + wave * 16 + kk + C::XOFF;

  for (int it = slot; it < items; it += nslots) {
    int t = it;
    const int tx = t % ntx;
    t /= ntx;
    const int rc = t % C::DIL;        // row class: image rows rc, rc + DIL, rc + 2 DIL, ...
    t /= C::DIL;
    const int ys = t % nys;
    const int b = t / nys;
    const int x0 = tx * C::TX, ia = ys * yseg, ib = ia + yseg;   // class-row range [ia, ib); rows past H read as zeros
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(x + ((size_t)b * Ci + cib * 32) * HW, (unsigned)nci * HW * 4u);
    const __amdgpu_buffer_rsrc_t drs = make_rsrc(dc + ((size_t)b * Co + cob * 32) * HW, (unsigned)nco * HW * 4u);
    unsigned xvo[C::IX], dvo[C::ID];   // channel + column part of this wave's copy instructions; the row is a scalar offset
#pragma unroll
    for (int j = 0; j < C::IX; ++j) {
      const int u = (j * 4 + wave) * 64 + lane, ch = u / C::UX, un = u - ch * C::UX;
      const int gx = x0 - C::PAD + 4 * un;
      xvo[j] = (ch < 32 && un < C::UXU && gx >= 0 && gx < W) ? ((unsigned)ch * HW + (unsigned)gx) * 4u : DMA_OOB;
    }
#pragma unroll
    for (int j = 0; j < C::ID; ++j) {
      const int u = (j * 4 + wave) * 64 + lane, ch = u / C::UD, un = u - ch * C::UD;
      const int gx = x0 + 4 * un;
      dvo[j] = (ch < 32 && un < C::UDU && gx < W) ? ((unsigned)ch * HW + (unsigned)gx) * 4u : DMA_OOB;
    }
    auto stage_x1 = [&](int ci_row, int rslot, int j) {   // class row -> image row rc + DIL * ci_row
      const int gy = rc + C::DIL * ci_row;
      const bool ok = ci_row >= 0 && gy < H;
      const int first = (j * 4 + wave) * 64;
      if (first + lane < 32 * C::UX) dma16(xrs, ok ? xvo[j] : DMA_OOB, ok ? (unsigned)gy * W * 4u : 0u, xring + rslot * C::XROW + first * 4);
    };
    auto stage_d1 = [&](int ci_row, int buf, int j) {
      const int gy = rc + C::DIL * ci_row;
      const bool ok = ci_row < ib && gy < H;
      const int first = (j * 4 + wave) * 64;
      if (first + lane < 32 * C::UD) dma16(drs, ok ? dvo[j] : DMA_OOB, ok ? (unsigned)gy * W * 4u : 0u, dbuf + buf * C::DROW + first * 4);
    };
    // ring slot of class row j: (j - (ia - RH)) % NR
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2 * RH + 1; ++q)
#pragma unroll
      for (int j = 0; j < C::IX; ++j) stage_x1(ia - RH + q, q, j);
#pragma unroll
    for (int j = 0; j < C::ID; ++j) stage_d1(ia, 0, j);
    __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    int r0 = 0;   // ring index of class row i - RH
    for (int i = ia; i < ib; ++i) {
      const int rel = i - ia;
      const bool more = i + 1 < ib;
      const float* ap = dbuf + (rel & 1) * C::DROW + aoff;
      const float* bp[C::KS];
#pragma unroll
      for (int ty = 0; ty < C::KS; ++ty) bp[ty] = xring + ((r0 + ty) % C::NR) * C::XROW + boff;
      const int rnew = (r0 + 2 * RH + 1) % C::NR;
      float af[2], bf[2][C::NTAP];
      auto load_frag = [&](int q, float& a, float (&bq)[C::NTAP]) {
        a = ap[2 * q];
#pragma unroll
        for (int tt = 0; tt < C::NTAP; ++tt) bq[tt] = bp[tt / C::KS][2 * q + (tt % C::KS) * C::DIL];
      };
      load_frag(0, af[0], bf[0]);
#pragma unroll
      for (int q = 0; q < C::KSTEPS; ++q) {
        if (q + 1 < C::KSTEPS) load_frag(q + 1, af[(q + 1) & 1], bf[(q + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int tt = 0; tt < C::NTAP; ++tt) acc[tt] = DMB_MFMA(af[q & 1], bf[q & 1][tt], acc[tt]);
        if (more) {
          if (q < C::IX)
            stage_x1(i + RH + 1, rnew, q);
          else if (q < C::IX + C::ID)
            stage_d1(i + 1, (rel + 1) & 1, q - C::IX);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      r0 = (r0 + 1) % C::NR;
      __builtin_amdgcn_s_waitcnt(0x0F70);
      __syncthreads();
    }
  }
  // the four waves' partial results are added through LDS (wave 0 stores, the others add in turn) before one copy per
  // workgroup goes to the workspace
  __syncthreads();
  float* red = lds;   // NTAP x 1024 floats <= the ring
  static_assert(C::NTAP * 1024 <= C::LDS_FLOATS, "reduction scratch");
#pragma unroll
  for (int wv = 0; wv < 4; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int tt = 0; tt < C::NTAP; ++tt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float* q = red + tt * 1024 + cd_row(r, kk) * 32 + n;
          *q = wv == 0 ? acc[tt][r] : *q + acc[tt][r];
        }
    }
    __syncthreads();
  }
  float* wsb = ws + ((size_t)blockIdx.y * nslots + slot) * C::NTAP * 1024;
  for (int i = threadIdx.x; i < C::NTAP * 1024; i += 256) wsb[i] = red[i];
}

__global__ void conv2d_wgrad_reduce_kernel(const float* __restrict__ ws, float* __restrict__ dw, int Co, int Ci, int nparts, int ntap) {
  const int ncib = cdiv(Ci, 32);
  const long long total = (long long)cdiv(Co, 32) * ncib * ntap * 1024;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int nn = (int)(i & 31), m = (int)((i >> 5) & 31);
    long long r = i >> 10;
    const int t = (int)(r % ntap);
    const int blk = (int)(r / ntap);
    const int cib = blk % ncib, cob = blk / ncib;
    const int co = cob * 32 + m, ci = cib * 32 + nn;
    if (co >= Co || ci >= Ci) continue;
    const float* p = ws + (size_t)blk * nparts * ntap * 1024 + t * 1024 + m * 32 + nn;
    double part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int sl = 0;
    for (; sl + 8 <= nparts; sl += 8) {
#pragma unroll
      for (int u = 0; u < 8; ++u) part[u] += (double)p[(size_t)(sl + u) * ntap * 1024];
    }
    for (; sl < nparts; ++sl) part[sl & 7] += (double)p[(size_t)sl * ntap * 1024];
    dw[((size_t)co * Ci + ci) * ntap + t] = (float)(((part[0] + part[1]) + (part[2] + part[3])) + ((part[4] + part[5]) + (part[6] + part[7])));
  }
}

// ------------------------------------------------------------------------------------------------------------------
// 2-D, kernel 5 on 1 .. DMB_CONV2D_K5_MAX_C channels (plan form 6): dW[co, ci, ky, kx] = sum_{b, y, x} dc[b, co, y, x] *
// x[b, ci, y + ky - 2, x + kx - 2] for nn.Conv2d(k 5, s 1, p 2) -- DeepPruner's range heads and its disparity refinement tail
// (SmallConv5x5).  M = Co <= 16 and N = Ci x 25 <= 400 against K = B x H x W: a 32 x 32 MFMA tile would be three quarters zeros at
// 14 -> 14 and all but one row at 1 -> 1, so this is a VALU kernel.  A workgroup walks tiles of 8 rows x 32 columns: the haloed x
// tile (12 x 36 per channel) and the dc tile go to LDS with plain loads (any width, any alignment, zeros outside the image); a
// thread owns ONE (co, ci) pair and its 25 taps in registers for the whole launch, and per tile row reads the dc row (32 floats)
// and five x rows (36 floats each) into registers: 212 LDS reads per 800 FMAs.  Where Co x Ci <= 128 the tile's rows are dealt
// out to 256 / (Co x Ci) groups of threads (at most 8), added in ascending group order through LDS at the end.  Channel pitches
// are odd: the lanes of a wave differ in ci (and read the same dc word).  Partial results per slot [Co][Ci][25] go to the workspace
// and are added over the slots in FP64 in a fixed order: no atomics, bit-reproducible.
// ------------------------------------------------------------------------------------------------------------------
struct Wg5Cfg {
  static constexpr int MAXC = DMB_CONV2D_K5_MAX_C, KS = 5, NTAP = KS * KS, HALO = KS / 2;
  static constexpr int TY = 8, TX = 32;
  static constexpr int XR = TY + 2 * HALO, XP = TX + 2 * HALO;   // rows and row pitch of the haloed x tile
  static constexpr int XC = XR * XP + 1, DC = TY * TX + 1;       // channel pitches (floats), odd
  static constexpr int PER_CU = 2;
  // row groups of a launch, and its LDS: the two tiles, or the groups' partial results at the end
  static constexpr int groups(int Co, int Ci) { return 256 / (Co * Ci) < TY ? 256 / (Co * Ci) : TY; }
  static constexpr int lds_floats(int Co, int Ci) {
    const int tiles = Ci * XC + Co * DC, red = groups(Co, Ci) * Co * Ci * NTAP;
    return tiles > red ? tiles : red;
  }
  static_assert(MAXC * MAXC <= 256 && MAXC * MAXC * NTAP <= 9 * 1024, "one thread per pair; a slot's partial result fits the 2-D workspace");
  static_assert(MAXC * (XC + DC) * 4 * PER_CU <= 160 * 1024 && 256 * NTAP * 4 * PER_CU <= 160 * 1024, "tile");
};

// An item = (batch item, tile row, tile column); nty tile rows.  workspace: ws[slot][co][ci][tap]
__global__ __launch_bounds__(256, Wg5Cfg::PER_CU) void conv2d_k5_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dc,
                                                                             float* __restrict__ ws, int B, int Ci, int Co, int H, int W,
                                                                             int ntx, int nty) {
  typedef Wg5Cfg C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* ds = lds + Ci * C::XC;
  const int slot = xcd_remap(blockIdx.x, gridDim.x), nslots = gridDim.x;
  const int tid = threadIdx.x;
  const int np = Co * Ci, G = C::groups(Co, Ci);
  const bool active = tid < G * np;
  const int pair = tid % np, grp = tid / np;
  const int co = pair / Ci, ci = pair - co * Ci;
  const size_t HW = (size_t)H * W;
  const int items = B * nty * ntx;

  float acc[C::NTAP];
#pragma unroll
  for (int t = 0; t < C::NTAP; ++t) acc[t] = 0.f;

  for (int it = slot; it < items; it += nslots) {
    const int tx = it % ntx;
    const int r = it / ntx;
    const int ty = r % nty, b = r / nty;
    const int x0 = tx * C::TX, y0 = ty * C::TY;
    const float* xb = x + (size_t)b * Ci * HW;
    const float* db = dc + (size_t)b * Co * HW;
    __syncthreads();   // the previous tile is still being read by slower waves
    for (int i = tid; i < Ci * C::XR * C::XP; i += 256) {
      const int ch = i / (C::XR * C::XP), q = i - ch * (C::XR * C::XP);
      const int row = q / C::XP, col = q - row * C::XP;
      const int gy = y0 - C::HALO + row, gx = x0 - C::HALO + col;
      xs[ch * C::XC + row * C::XP + col] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[ch * HW + (size_t)gy * W + gx] : 0.f;
    }
    for (int i = tid; i < Co * C::TY * C::TX; i += 256) {
      const int ch = i / (C::TY * C::TX), q = i - ch * (C::TY * C::TX);
      const int row = q / C::TX, col = q - row * C::TX;
      const int gy = y0 + row, gx = x0 + col;
      ds[ch * C::DC + row * C::TX + col] = (gy < H && gx < W) ? db[ch * HW + (size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    if (active) {
      const int rows = min(C::TY, H - y0);   // (rows past the image hold zeros of dc)
      for (int row = grp; row < rows; row += G) {
        float dr[C::TX];
        const float* dp = ds + co * C::DC + row * C::TX;
#pragma unroll
        for (int j = 0; j < C::TX; ++j) dr[j] = dp[j];
#pragma unroll
        for (int ky = 0; ky < C::KS; ++ky) {
          float xr[C::XP];
          const float* xp = xs + ci * C::XC + (row + ky) * C::XP;
#pragma unroll
          for (int j = 0; j < C::XP; ++j) xr[j] = xp[j];
#pragma unroll
          for (int j = 0; j < C::TX; ++j)
#pragma unroll
            for (int kx = 0; kx < C::KS; ++kx) acc[ky * C::KS + kx] = fmaf(dr[j], xr[j + kx], acc[ky * C::KS + kx]);
        }
      }
    }
  }
  // the row groups' results, added in ascending group order (the tiles' LDS is free now)
  __syncthreads();
  float* red = lds;
  if (active) {
#pragma unroll
    for (int t = 0; t < C::NTAP; ++t) red[(grp * np + pair) * C::NTAP + t] = acc[t];
  }
  __syncthreads();
  float* wsb = ws + (size_t)slot * np * C::NTAP;
  for (int e = tid; e < np * C::NTAP; e += 256) {
    float s = red[e];
    for (int g = 1; g < G; ++g) s += red[g * np * C::NTAP + e];
    wsb[e] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// 2-D, kernel 3 with ONE output channel on 1 .. DMB_REFINE_HEAD_MAX_C input channels (plan form 7): dW[0, ci, ky, kx] =
// sum_{b, y, x} dc[b, 0, y, x] * x[b, ci, y + ky - 1, x + kx - 1] for nn.Conv2d(Ci, 1, 3, 1, 1) -- the classifier of DeepPruner's
// refinement head (16 -> 1).  M = 1 against N = Ci x 9 <= 144: the 32 x 32 MFMA tile of form 4 is 31 rows of zeros, and FP32 MFMA
// runs at the vector FP32 rate anyway, so this is a VALU kernel in the manner of the 5x5 one above.  A workgroup walks tiles of
// 8 rows x 32 columns: the haloed x tile (10 x 34 per channel) and the dc tile go to LDS with plain loads (any width, any
// alignment, zeros outside the image).  A tile is 32 units of (row, 8 columns); a thread owns ONE channel's 9 taps in registers for
// the whole launch and belongs to one of min(256 / Ci, 32) groups, which takes units grp, grp + groups, ...: per unit 8 dc words
// and 3 x 10 x words from LDS for 72 FMAs.  At 16 channels the 32 lanes that share an LDS access are 16 channels x 2 rows of one
// column segment: the channel pitch is 2 mod 32 and the row pitches are odd, so they meet 32 different banks (x) or two words
// that 16 lanes each share (dc).  (Other channel counts are correct, not conflict-free.)  The groups' sums are added in
// ascending group order through LDS at the end; partial results per slot [Ci][9] go to the workspace and are added over the
// slots in FP64 in a fixed order: no atomics, bit-reproducible.
// ------------------------------------------------------------------------------------------------------------------
struct WgC1x2dCfg {
  static constexpr int MAXC = DMB_REFINE_HEAD_MAX_C, KS = 3, NTAP = KS * KS;
  static constexpr int TY = 8, TX = 32, SEG = 8, UNITS = TY * (TX / SEG);
  static constexpr int XR = TY + 2, XW = TX + 2;                     // rows and used columns of the haloed x tile
  static constexpr int XP = XW + 1, XC = XR * XP + 4, DP = TX + 1;   // pitches (floats): x row, x channel, dc row
  static constexpr int PER_CU = 4;
  static constexpr int groups(int Ci) { return 256 / Ci < UNITS ? 256 / Ci : UNITS; }
  static constexpr int lds_floats(int Ci) {
    const int tiles = Ci * XC + TY * DP, red = groups(Ci) * Ci * NTAP;
    return tiles > red ? tiles : red;
  }
  static_assert(XP % 2 == 1 && DP % 2 == 1 && XC % 32 == 2 && XC >= XR * XP, "bank-conflict-free pitches at 16 channels");
  static_assert(MAXC * PER_CU * NTAP <= 2 * 9 * 1024, "the slots' partial results fit the 2-D workspace");
  static_assert((MAXC * XC + TY * DP) * 4 * PER_CU <= 160 * 1024 && 256 * NTAP * 4 * PER_CU <= 160 * 1024, "tile");
};

// An item = (batch item, tile row, tile column); nty tile rows.  workspace: ws[slot][ci][tap]
__global__ __launch_bounds__(256, WgC1x2dCfg::PER_CU) void conv2d_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dc,
                                                                                 float* __restrict__ ws, int B, int Ci, int H, int W, int ntx,
                                                                                 int nty) {
  typedef WgC1x2dCfg C;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  float* ds = lds + Ci * C::XC;
  const int slot = xcd_remap(blockIdx.x, gridDim.x), nslots = gridDim.x;
  const int tid = threadIdx.x;
  const int G = C::groups(Ci);
  const bool active = tid < G * Ci;
  const int grp = tid / Ci, ci = tid - grp * Ci;
  const size_t HW = (size_t)H * W;
  const int items = B * nty * ntx;

  float acc[C::NTAP];
#pragma unroll
  for (int t = 0; t < C::NTAP; ++t) acc[t] = 0.f;

  for (int it = slot; it < items; it += nslots) {
    const int tx = it % ntx;
    const int r = it / ntx;
    const int ty = r % nty, b = r / nty;
    const int x0 = tx * C::TX, y0 = ty * C::TY;
    const float* xb = x + (size_t)b * Ci * HW;
    const float* db = dc + (size_t)b * HW;
    __syncthreads();   // the previous tile is still being read by slower waves
    for (int i = tid; i < Ci * C::XR * C::XW; i += 256) {
      const int ch = i / (C::XR * C::XW), q = i - ch * (C::XR * C::XW);
      const int row = q / C::XW, col = q - row * C::XW;
      const int gy = y0 - 1 + row, gx = x0 - 1 + col;
      xs[ch * C::XC + row * C::XP + col] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? xb[ch * HW + (size_t)gy * W + gx] : 0.f;
    }
    {
      const int row = tid / C::TX, col = tid - row * C::TX;   // TY x TX = 256: one word per thread
      const int gy = y0 + row, gx = x0 + col;
      ds[row * C::DP + col] = (gy < H && gx < W) ? db[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    if (active) {
      for (int u = grp; u < C::UNITS; u += G) {
        const int row = u % C::TY, c0 = (u / C::TY) * C::SEG;
        if (y0 + row >= H || x0 + c0 >= W) continue;   // (dc is zero there)
        float dr[C::SEG];
        const float* dp = ds + row * C::DP + c0;
#pragma unroll
        for (int j = 0; j < C::SEG; ++j) dr[j] = dp[j];
#pragma unroll
        for (int ky = 0; ky < C::KS; ++ky) {
          float xr[C::SEG + 2];
          const float* xp = xs + ci * C::XC + (row + ky) * C::XP + c0;
#pragma unroll
          for (int j = 0; j < C::SEG + 2; ++j) xr[j] = xp[j];
#pragma unroll
          for (int j = 0; j < C::SEG; ++j)
#pragma unroll
            for (int kx = 0; kx < C::KS; ++kx) acc[ky * C::KS + kx] = fmaf(dr[j], xr[j + kx], acc[ky * C::KS + kx]);
        }
      }
    }
  }
  // the groups' results, added in ascending group order (the tiles' LDS is free now)
  __syncthreads();
  float* red = lds;
  if (active) {
#pragma unroll
    for (int t = 0; t < C::NTAP; ++t) red[(grp * Ci + ci) * C::NTAP + t] = acc[t];
  }
  __syncthreads();
  float* wsb = ws + (size_t)slot * Ci * C::NTAP;
  for (int e = tid; e < Ci * C::NTAP; e += 256) {
    float s = red[e];
    for (int g = 1; g < G; ++g) s += red[g * Ci * C::NTAP + e];
    wsb[e] = s;
  }
}

// ------------------------------------------------------------------------------------------------------------------
// The instantiations a launch can run: ONE list per form.  Bits 0-7 of a plan code are the position in the form's list
// (include/dmb_hip.h numbers them); wgrad_plan names a position and wg_visit is the only place where one becomes a type.
// ------------------------------------------------------------------------------------------------------------------
template <bool V16_, int TX_>
struct WgS1Form {
  typedef WgCfg<TX_> C;
  static constexpr bool V16 = V16_;   // 16-byte staging, else dword copies
};
template <class C_, bool V16_>
struct WgS2Form {
  typedef C_ C;
  static constexpr bool V16 = V16_;
};
using WgS1Forms = std::tuple<WgS1Form<true, 24>, WgS1Form<true, 32>, WgS1Form<false, 24>>;
using WgS2Forms = std::tuple<WgS2Form<Wg2Cfg<2, 12>, true>, WgS2Form<Wg2Cfg<2, 12>, false>, WgS2Form<Wg2Cfg<4, 8>, true>, WgS2Form<Wg2Cfg<4, 8>, false>>;
using WgHwForms = std::tuple<WgS2Form<WgHwCfg, true>, WgS2Form<WgHwCfg, false>>;   // stride (1, 2, 2)
using Wg2dForms = std::tuple<Wg2dCfg<3, 1>, Wg2dCfg<3, 2>, Wg2dCfg<3, 4>, Wg2dCfg<3, 8>, Wg2dCfg<1, 1>>;

template <class L, class F, size_t... I>
static int wg_visit(int k, F&& f, std::index_sequence<I...>) {
  int rc = DMB_EUNSUPPORTED;
  const bool hit = ((k == (int)I && ((rc = f(std::tuple_element_t<I, L>{})), true)) || ...);
  return hit ? rc : fail(DMB_EUNSUPPORTED, "wgrad: the plan names an instantiation this build does not hold");
}
// f(Form{}) for the type a plan code names in the list L of its form
template <class L, class F>
static int wg_visit(int code, F&& f) { return wg_visit<L>(code & 0xff, f, std::make_index_sequence<std::tuple_size_v<L>>{}); }

// The planned instantiation on the planned grid, its LDS cap raised first (*seen: one static per instantiation, see ensure_dynamic_lds)
template <class... P, class... A>
static int wg_launch(void (*kernel)(P...), int lds_bytes, unsigned long long* seen, const WgradPlan& p, hipStream_t st, const char* what, A... args) {
  const int rc = ensure_dynamic_lds(reinterpret_cast<const void*>(kernel), (size_t)lds_bytes, seen);
  if (rc != DMB_OK) return rc;
  hipLaunchKernelGGL(kernel, dim3((unsigned)p.slots, (unsigned)p.blocks), dim3(256), lds_bytes, st, args...);
  return launch_status(what);
}

// floats of workspace: one partial result [ntap][32][32] per slot and channel block
static long long wgrad_ws_floats(int Co, int Ci, int per_cu, int ntap, int ncu) {
  return (long long)cdiv(Co, 32) * cdiv(Ci, 32) * wgrad_slots_per_block(Co, Ci, per_cu, ncu) * ntap * 1024;
}

// The plan of a launch: every refusal and every choice of the three entry points (wgrad_plan.h)
int wgrad_plan(const WgradDesc& d, WgradPlan* p, const char** why) {
  const int B = d.B, Co = d.Co, Ci = d.Ci, D = d.D, H = d.H, W = d.W, ncu = d.ncu;
  auto refuse = [&](int err, const char* msg) { return *why = msg, err; };
  // segments of `seg` along an axis of `extent`; no more slots than items (small layers: no idle slots to write and add zeros for)
  auto planned = [&](int form, int index, int ntx, int nty, int extent, int seg, long long items_per_segment_count, int nslots) {
    const int nseg = cdiv(extent, seg);
    const long long items = items_per_segment_count * nseg;
    *p = {(form << 8) | index, ntx, nty, seg, nseg, (int)(items < nslots ? items : nslots), cdiv(Co, 32) * cdiv(Ci, 32)};
    return DMB_OK;
  };
  const bool aligned = d.align >= 16;
  const long long LIM = 0x7fffffffLL;   // 32-bit buffer offsets

  if (d.kind == DMB_WGRAD_S1) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || D <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "conv3d_wgrad: bad argument");
    if ((long long)32 * D * H * W * 4 >= LIM) return refuse(DMB_EUNSUPPORTED, "conv3d_wgrad: 32 channels of one batch item must stay below 2 GiB");
    if (Co == 1) {   // classifier heads: the single-output-channel form (M = channels, N = taps, K = voxels on the matrix cores)
      const int ntx = cdiv(W, C1M_XT), nty = cdiv(H, C1M_ROWS);
      const long long nt = (long long)B * D * ntx * nty;
      if (nt > LIM) return refuse(DMB_EUNSUPPORTED, "conv3d_wgrad (1 channel): too many tiles");
      // persistent grid: four workgroups per CU, bounded by the tiles and by the caller's workspace ([workgroup][Ci][27] partials)
      long long g = 4LL * ncu;
      const long long cap = wgrad_ws_floats(Co, Ci, 1, 27, ncu) / ((long long)Ci * 27);
      if (g > nt) g = nt;
      if (g > cap) g = cap;
      if (g < 1) g = 1;
      *p = {WGRAD_C1 << 8, ntx, nty, 1, D, (int)g, cdiv(Ci, 32)};
      return DMB_OK;
    }
    // 24- or 32-column tiles: whichever covers W with fewer computed columns (W = 128 of the training crops: 128 against 144)
    const bool wide = cdiv(W, 32) * 32 < cdiv(W, 24) * 24;
    const bool v16 = W % 4 == 0 && aligned;
    const int nty = cdiv(H, WgCfg<24>::TY);
    // z segments.  Rows that cannot take 16-byte copies run the 24-column dword form on the segments and slots of their width
    // class's tile (as ever: the split decides the order of the sums, so it stays).
    const long long per_seg = (long long)B * cdiv(W, wide ? 32 : 24) * nty;
    const int nslots = wgrad_slots_per_block(Co, Ci, 1, ncu);
    int zseg = segment_search(D, per_seg, nslots, WG_SEG_S1);
    if (DMB_OPT(5) > 0) zseg = cdiv(D, DMB_OPT(5));   // (development option 5: number of z segments)
    return planned(WGRAD_S1, v16 ? (wide ? 1 : 0) : 2, cdiv(W, v16 && wide ? 32 : 24), nty, D, zseg, per_seg, nslots);
  }

  if (d.kind == DMB_WGRAD_S2) {   // Co / D, H, W: the small operand's; Ci / Db, Hb, Wb: the big one's
    const int Db = d.Db, Hb = d.Hb, Wb = d.Wb;
    if (B <= 0 || Co <= 0 || Ci <= 0 || D <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "conv3d_s2_wgrad: bad argument");
    // only height and width strided (stride (1, 2, 2)): the same depth, two planes or more.  (One plane of either reading is the
    // same sum and stays on the stride-2 kernels.)
    const bool hw = Db == D && D >= 2;
    if ((!hw && Db != 2 * D && Db != 2 * D - 1) || (Hb != 2 * H && Hb != 2 * H - 1) || (Wb != 2 * W && Wb != 2 * W - 1))
      return refuse(DMB_EINVAL, "conv3d_s2_wgrad: the big tensor must be 2n or 2n - 1 per axis");
    if ((long long)32 * Db * Hb * Wb * 4 >= LIM) return refuse(DMB_EUNSUPPORTED, "conv3d_s2_wgrad: 32 channels of one batch item must stay below 2 GiB");
    const bool v16 = W % 4 == 0 && Wb % 4 == 0 && aligned;
    const int nslots = wgrad_slots_per_block(Co, Ci, 1, ncu);
    if (hw) {   // one tile; the segments are what fills the CUs from the few tiles of these layers
      typedef std::tuple_element_t<0, WgHwForms>::C C;
      const int ntx = cdiv(W, C::TX), nty = cdiv(H, C::TY);
      const long long per_seg = (long long)B * ntx * nty;
      int zseg = segment_search(D, per_seg, nslots, WG_SEG_HW);
      if (DMB_OPT(5) > 0) zseg = cdiv(D, DMB_OPT(5));   // (development option 5: number of z segments)
      return planned(WGRAD_HW, v16 ? 0 : 1, ntx, nty, D, zseg, per_seg, nslots);
    }
    // z segments and the launch's cost for a tile shape: rounds of items on the slots x (planes per item + prologue) x the tile's
    // k-steps, over what the tile reaches between its barriers (4 x 8: 112 MFMAs per wave and barrier against 84; measured at the
    // training crop, profiles/r06_wgrad_s2_tiles.log)
    struct { int ty, tx; double eff; int zseg; double cost; } t[2] = {{2, 12, 1.0, 0, 0}, {4, 8, WG2_EFF_4x8, 0, 0}};
    for (auto& c : t) {
      c.zseg = segment_search(D, (long long)B * cdiv(W, c.tx) * cdiv(H, c.ty), nslots, WG_SEG_S2, &c.cost);
      c.cost = c.cost * (c.ty * c.tx) / c.eff;
    }
    int wide = t[1].cost < t[0].cost;     // the 4 x 8 tile
    if (DMB_OPT(27) == 1) wide = 0;       // (development option 27: 1 = always 2 x 12, 2 = always 4 x 8)
    if (DMB_OPT(27) == 2) wide = 1;
    const auto& c = t[wide];
    return planned(WGRAD_S2, 2 * wide + (v16 ? 0 : 1), cdiv(W, c.tx), cdiv(H, c.ty), D, c.zseg, (long long)B * cdiv(W, c.tx) * cdiv(H, c.ty), nslots);
  }

  if (d.kind == DMB_WGRAD_2D) {
    if (B <= 0 || Ci <= 0 || Co <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "conv2d_wgrad: bad argument");
    if ((long long)32 * H * W * 4 >= LIM) return refuse(DMB_EUNSUPPORTED, "conv2d_wgrad: 32 channels of one image must stay below 2 GiB");
    if (d.ksize == 5 && d.dilation == 1 && Co <= Wg5Cfg::MAXC && Ci <= Wg5Cfg::MAXC) {   // small-channel 5x5: any width, any alignment
      typedef Wg5Cfg C;
      const int ntx = cdiv(W, C::TX);
      if ((long long)B * ntx * cdiv(H, C::TY) > LIM) return refuse(DMB_EUNSUPPORTED, "conv2d_wgrad (kernel 5): too many tiles");
      // one row class; a "segment" is a tile's rows: items = B x tiles, accumulated in registers by the slot that walks them
      return planned(WGRAD_K5, 0, ntx, 1, H, C::TY, (long long)B * ntx, wgrad_slots_per_block(Co, Ci, C::PER_CU, ncu));
    }
    if (d.ksize == 3 && d.dilation == 1 && Co == 1 && Ci <= WgC1x2dCfg::MAXC) {   // one output channel: any width, any alignment
      typedef WgC1x2dCfg C;
      const int ntx = cdiv(W, C::TX);
      if ((long long)B * ntx * cdiv(H, C::TY) > LIM) return refuse(DMB_EUNSUPPORTED, "conv2d_wgrad (1 channel): too many tiles");
      // as kernel 5: one row class, a "segment" is a tile's rows; [slot][Ci][9] partials, four slots per CU (asserted to fit)
      return planned(WGRAD_C1_2D, 0, ntx, 1, H, C::TY, (long long)B * ntx, wgrad_slots_per_block(Co, Ci, C::PER_CU, ncu));
    }
    if (W % 4 != 0 || !aligned) return refuse(DMB_EUNSUPPORTED, "conv2d_wgrad: the width must be a multiple of 4 and the tensors 16-byte aligned");
    const int dil = d.ksize == 1 ? 1 : d.dilation;   // (a 1x1 layer has no dilation)
    const int index = d.ksize == 1 ? 4 : (d.ksize != 3 ? -1 : (dil == 1 ? 0 : (dil == 2 ? 1 : (dil == 4 ? 2 : (dil == 8 ? 3 : -1)))));
    if (index < 0) return refuse(DMB_EUNSUPPORTED, "conv2d_wgrad: kernel 1, or kernel 3 with dilation 1, 2, 4 or 8 (stride 1)");
    // y segments of a row class (rows y, y + dil, ...: cdiv(H, dil) of them); two workgroups per CU
    const int ntx = cdiv(W, Wg2dCfg<3, 1>::TX), HC = cdiv(H, dil), nslots = wgrad_slots_per_block(Co, Ci, 2, ncu);
    const long long per_seg = (long long)B * ntx * dil;
    return planned(WGRAD_2D, index, ntx, dil, HC, segment_search(HC, per_seg, nslots, WG_SEG_2D), per_seg, nslots);
  }
  return refuse(DMB_EINVAL, "conv_wgrad_plan: kind must be DMB_WGRAD_S1, DMB_WGRAD_S2 or DMB_WGRAD_2D");
}

}  // namespace dmb

using namespace dmb;

extern "C" long long dmb_conv3d_wgrad_workspace_floats(int Co, int Ci) { return Co <= 0 || Ci <= 0 ? 0 : wgrad_ws_floats(Co, Ci, 1, 27, num_cus()); }
extern "C" long long dmb_conv2d_wgrad_workspace_floats(int Co, int Ci) { return Co <= 0 || Ci <= 0 ? 0 : wgrad_ws_floats(Co, Ci, 2, 9, num_cus()); }

extern "C" int dmb_conv_wgrad_plan(int kind, int B, int Co, int Ci, int D, int H, int W, int Db, int Hb, int Wb, int ksize, int dilation,
                                   int align, int ncu, int* detail_host) {
  WgradPlan p = {};
  const char* why = "";
  const int rc = wgrad_plan({kind, B, Co, Ci, D, H, W, Db, Hb, Wb, ksize, dilation, align, ncu > 0 ? ncu : num_cus()}, &p, &why);
  set_last_error(why);
  if (rc != DMB_OK) return -rc;
  if (detail_host) {
    const int v[6] = {p.ntx, p.nty, p.seg, p.nseg, p.slots, p.blocks};
    for (int i = 0; i < 6; ++i) detail_host[i] = v[i];
  }
  return p.code;
}

// the two operands' alignment together
static int align_of_both(const void* a, const void* b) { return align_of(reinterpret_cast<const void*>((uintptr_t)a | (uintptr_t)b)); }

extern "C" int dmb_conv3d_k3_wgrad_f32(const float* x, const float* dc, float* dw, float* workspace, int B, int Ci, int Co,
                                       int D, int H, int W, void* stream) {
  if (!x || !dc || !dw || !workspace) return fail(DMB_EINVAL, "conv3d_wgrad: bad argument");
  WgradPlan p;
  const char* why = "";
  int rc = wgrad_plan({DMB_WGRAD_S1, B, Co, Ci, D, H, W, 0, 0, 0, 3, 1, align_of_both(x, dc), num_cus()}, &p, &why);
  if (rc != DMB_OK) return fail(rc, why);
  hipStream_t st = (hipStream_t)stream;
  if (p.code >> 8 == WGRAD_C1) {
    hipLaunchKernelGGL(conv3d_c1_wgrad_kernel, dim3((unsigned)p.slots, (unsigned)p.blocks), dim3(256), 0, st, x, dc, workspace, B, Ci, D, H, W, p.ntx,
                       p.nty, B * p.nseg * p.ntx * p.nty);
    hipLaunchKernelGGL(wgrad_reduce_flat_kernel, dim3(cdiv(Ci * 27, 4)), dim3(256), 0, st, workspace, dw, Ci * 27, p.slots);
    return launch_status("conv3d_wgrad (1 channel) launch failed");
  }
  rc = wg_visit<WgS1Forms>(p.code, [&](auto f) {
    typedef decltype(f) F;
    static unsigned long long seen = 0;
    return wg_launch(&conv3d_wgrad_s1_kernel<F::V16, F::C::TX>, F::C::LDS_FLOATS * 4, &seen, p, st, "conv3d_wgrad launch failed", x, dc, workspace,
                     B, Ci, Co, D, H, W, p.ntx, p.nty, p.nseg, p.seg);
  });
  if (rc != DMB_OK) return rc;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(p.blocks * 27 * 16), dim3(256), 0, st, workspace, dw, Co, Ci, p.slots);
  return launch_status("conv3d_wgrad reduce launch failed");
}

extern "C" int dmb_conv3d_k3s2_wgrad_f32(const float* small, const float* big, float* dw, float* workspace, int B, int Cs, int Cb,
                                         int Ds, int Hs, int Ws, int Db, int Hb, int Wb, void* stream) {
  if (!small || !big || !dw || !workspace) return fail(DMB_EINVAL, "conv3d_s2_wgrad: bad argument");
  WgradPlan p;
  const char* why = "";
  int rc = wgrad_plan({DMB_WGRAD_S2, B, Cs, Cb, Ds, Hs, Ws, Db, Hb, Wb, 3, 1, align_of_both(small, big), num_cus()}, &p, &why);
  if (rc != DMB_OK) return fail(rc, why);
  hipStream_t st = (hipStream_t)stream;
  auto run = [&](auto f) {
    typedef decltype(f) F;
    static unsigned long long seen = 0;
    return wg_launch(&conv3d_wgrad_s2_kernel<typename F::C, F::V16>, F::C::LDS_FLOATS * 4, &seen, p, st, "conv3d_s2_wgrad launch failed", small, big,
                     workspace, B, Cs, Cb, Ds, Hs, Ws, Db, Hb, Wb, p.ntx, p.nty, p.nseg, p.seg);
  };
  rc = p.code >> 8 == WGRAD_HW ? wg_visit<WgHwForms>(p.code, run) : wg_visit<WgS2Forms>(p.code, run);
  if (rc != DMB_OK) return rc;
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(p.blocks * 27 * 16), dim3(256), 0, st, workspace, dw, Cs, Cb, p.slots);
  return launch_status("conv3d_s2_wgrad reduce launch failed");
}

extern "C" int dmb_conv2d_wgrad_f32(const float* x, const float* dc, float* dw, float* workspace, int B, int Ci, int Co, int H, int W,
                                    int ksize, int dilation, void* stream) {
  if (!x || !dc || !dw || !workspace) return fail(DMB_EINVAL, "conv2d_wgrad: bad argument");
  WgradPlan p;
  const char* why = "";
  const int rc = wgrad_plan({DMB_WGRAD_2D, B, Co, Ci, 1, H, W, 0, 0, 0, ksize, dilation, align_of_both(x, dc), num_cus()}, &p, &why);
  if (rc != DMB_OK) return fail(rc, why);
  hipStream_t st = (hipStream_t)stream;
  if (p.code >> 8 == WGRAD_K5) {
    hipLaunchKernelGGL(conv2d_k5_wgrad_kernel, dim3((unsigned)p.slots), dim3(256), Wg5Cfg::lds_floats(Co, Ci) * 4, st, x, dc, workspace, B, Ci, Co, H, W,
                       p.ntx, p.nseg);
    const int n = Co * Ci * Wg5Cfg::NTAP;
    hipLaunchKernelGGL(wgrad_reduce_flat_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, workspace, dw, n, p.slots);
    return launch_status("conv2d_wgrad (kernel 5) launch failed");
  }
  if (p.code >> 8 == WGRAD_C1_2D) {
    hipLaunchKernelGGL(conv2d_c1_wgrad_kernel, dim3((unsigned)p.slots), dim3(256), WgC1x2dCfg::lds_floats(Ci) * 4, st, x, dc, workspace, B, Ci, H, W, p.ntx,
                       p.nseg);
    const int n = Ci * WgC1x2dCfg::NTAP;
    hipLaunchKernelGGL(wgrad_reduce_flat_kernel, dim3(cdiv(n, 4)), dim3(256), 0, st, workspace, dw, n, p.slots);
    return launch_status("conv2d_wgrad (1 channel) launch failed");
  }
  return wg_visit<Wg2dForms>(p.code, [&](auto c) {
    typedef decltype(c) C;
    static unsigned long long seen = 0;
    const int lrc = wg_launch(&conv2d_wgrad_kernel<C::KS, C::DIL>, C::LDS_FLOATS * 4, &seen, p, st, "conv2d_wgrad launch failed", x, dc, workspace, B, Ci,
                              Co, H, W, p.ntx, p.nseg, p.seg);
    if (lrc != DMB_OK) return lrc;
    hipLaunchKernelGGL(conv2d_wgrad_reduce_kernel, dim3(cdiv(p.blocks * C::NTAP * 1024, 256)), dim3(256), 0, st, workspace, dw, Co, Ci, p.slots, C::NTAP);
    return launch_status("conv2d_wgrad reduce launch failed");
  });
}

