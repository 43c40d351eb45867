// Stride-1 and stride-2 3x3x3 convolutions of the cost aggregators: the FP32-MFMA implicit GEMM described at the head of conv3d.hip
// (roles, data flow per workgroup).  First the stride-1 kernel, its tile shapes and the estimate that chooses among them, the
// BatchNorm-statistics form of the training path and the fused 32 -> 1 classifier head; then the stride-2 kernel and the estimate of
// its tile height.  dmb_conv3d_k3_f32 (conv3d.hip) reaches them through conv3d_s1_plan / conv3d_s2_plan and conv3d_s1_run / conv3d_s2_run.
//
// Why the two share a translation unit: the compiler propagates constants and value ranges into the small helpers of dmb_common.h /
// conv3d_mfma.h (cdiv, store_tile<1>, ...) from ALL their callers in the unit before it inlines them.  Alone, the stride-2 kernels
// see cdiv(Ci, 2) only and a store_tile<1> without the stride-1 callers, and every one of their instantiations gets another register
// allocation (e.g. 136 -> 144 VGPRs for the 22-column tile) than the measured ones of profiles/.  The stride-1 kernels, the transposed
// kernel (deconv3d.hip) and the one-channel kernels (conv3d_c1.hip) compile the same on their own
// (profiles/conv3d_split_resources_{before,after}.txt).
#include <array>
#include <tuple>
#include <type_traits>
#include <utility>

#include "conv3d_mfma.h"

namespace dmb {

// ---------------------------------------------------------------------------------------------------------
// Stride-1 kernel.
// ---------------------------------------------------------------------------------------------------------
// LIN (with G = 16, TX = W, TY = 3): the wave's 32-voxel column tiles are 32 CONSECUTIVE voxels of the (y, x) plane in memory
// order, a workgroup = TZ planes x 64 consecutive voxels (two column tiles per wave).  For the quarter-resolution layer of the
// hourglass ([4, 64, 12, 34, 60]: 97 920 voxels = 382.5 per CU) no box tiling comes near a multiple of 256 equal workgroups (216
// boxes of 4 x 4 x 60 = 84 % of the chip, one wave per SIMD); 64-voxel runs give 4 x 6 x 32 = 768 equal workgroups = exactly three
// per CU, 99.6 % of their column tiles real.  The staged tile is the 3 + 2 rows a 64-voxel run can touch (W >= 32), full width.
// (nothing reads CIN_: the kernel-name prefix S1Cfg<0, 32, 4, 48 is how scripts/summarize_profiles.py and profiles/ find the dominant layer)
template <int CIN_, int COUT_, int TY_, int TX_, int CK_, int WN_, int G_ = 0, int PMIN_ = 0, bool LIN_ = false>
struct S1Cfg {
  static constexpr int CIN = CIN_, COUT = COUT_, TY = TY_, TX = TX_, CK = CK_, WN = WN_;
  static constexpr bool LIN = LIN_;
  static constexpr bool HEAD = false;          // S1HeadCfg: the 32 -> 1 classifier head inside the epilogue
  static constexpr int G = G_;                  // row-group width: 0 = flattened tiles, 16 = row pairs, 8 = row quads
  static constexpr bool ROWPAIR = G_ != 0;     // any row-group mapping (takes the 16-byte vector path)
  static constexpr int GR = G_ ? 32 / G_ : 1;  // rows per group
  static constexpr int WZ = 4 / WN;        // waves along z; one output z-slice per wave
  static constexpr int TZ = WZ;
  // Row-pair tiles are staged with 16-byte LDS-DMA words: a staged row starts at the 16-byte aligned column x0 - 4
  // (XOFF = 3 unused floats in front of the halo column) and is a whole number of words long.  A CU retires LDS-DMA
  // at about one lane per clock whatever the word size, so this is 4x fewer TA cycles for the same bytes.
  static constexpr int XOFF = ROWPAIR ? 3 : 0;
  static constexpr int PV = (4 + TX + 1 + 3) / 4 * 4;
  static constexpr int P = ROWPAIR ? (PV > PMIN_ ? PV : PMIN_) : TX + 2;   // padded row pitch (PMIN: bank-friendly pitch)
  static constexpr int ROWS = TY + 2;
  static constexpr int PLANE = ROWS * P;
  static constexpr int ZS = TZ + 2;
  static constexpr int UPR = P / 4, UPC = ZS * ROWS * UPR;   // row-pair path: 16-byte units per row / per channel
  static constexpr int IPC = (UPC + 63) / 64;                // copy instructions per channel
  static constexpr int TR_PITCH = 36;                        // epilogue transposition scratch [32 channels][32 + 4]
  // How the 32 columns (voxels) of an MFMA B tile map onto the LDS tile:
  //  - flattened (default): 32 consecutive positions of the padded (y, x) plane; works for any TX, but the 2 halo
  //    columns per row and the last partial tile are computed and discarded (6 % at TX = 60, TY = 4);
  //  - row group (TX % G == 0, TY % (32 / G) == 0): G columns of 32 / G consecutive rows -- row pairs of 16 (lanes 0-15 =
  //    row r, 16-31 = row r + 1) or row quads of 8: every computed voxel is a real output.  Used when W % TX == 0.
  static constexpr int XS = ROWPAIR ? TX / (G_ ? G_ : 1) : 1;
  static constexpr int MT = LIN ? 2 : (ROWPAIR ? (TY / GR) * XS : (TY * P + 31) / 32);  // 32-voxel column tiles per wave
  // Which rows a row PAIR takes.  A B-fragment read (ds_read_b32) is served 32 lanes at a time, bank = dword address mod 32: lanes
  // 0-15 cover 16 banks of one row, lanes 16-31 the same columns of the pair's other row, GSTR * P floats on.  With the natural
  // pair (rows r, r + 1) and P = 56 (48-column tiles) or 40 (32-column tiles) the second row starts 24 / 8 banks on: eight lanes
  // collide and every such read takes two LDS cycles (counters of the dominant layer: 45 % of its LDS cycles were conflicts).
  // Pairing rows (r, r + 2) of a four-row tile instead -- tile q of a column = rows q and q + 2 -- puts the second row
  // 2 P = 16 (mod 32) banks on: conflict-free.  Same MFMAs on the same operands; only which accumulator holds which row changes
  // (bit-identical by checksum; scripts/README.md, retired experiments).  What it buys is LDS cycles, not time: 2.389 / 2.396 against
  // 2.386 / 2.391 ms at [4, 32, 48, 136, 240] (noise), 2.236 / 2.240 against 2.244 / 2.243 ms at [4, 32, 48, 96, 312] (-0.3 %) --
  // the LDS pipe is a quarter busy either way and the fragment reads run a k-step ahead of their MFMAs.
  static constexpr int GSTR = (G_ == 16 && TY_ == 4 && !LIN_ && (2 * P) % 32 == 16 && P % 32 != 16) ? 2 : 1;
  __device__ static constexpr int row_base(int q) { return GSTR == 2 ? q : GR * q; }   // first row of the q-th group of a column
  __device__ static constexpr int lane_off(int j) { return ROWPAIR ? (j / (G_ ? G_ : 1)) * GSTR * P + (j % (G_ ? G_ : 1)) : j; }
  __device__ static constexpr int tile_off(int mt) { return ROWPAIR ? row_base(mt / XS) * P + (mt % XS) * G_ : mt * 32; }
  __device__ static void decode(int mt, int j, int& ly, int& lx, bool& valid) {
    if (ROWPAIR) {
      ly = row_base(mt / XS) + GSTR * (j / (G_ ? G_ : 1));
      lx = (mt % XS) * G_ + j % (G_ ? G_ : 1);
      valid = true;
    } else {
      const int m = mt * 32 + j;
      ly = m / P;
      lx = m - ly * P;
      valid = m < TY * P && lx < TX;
    }
  }
  static constexpr int NTT = COUT / 32;          // 32-channel row tiles in total
  static constexpr int NT = NTT / WN;            // ... per wave
  static constexpr int CH_STRIDE = ZS * PLANE + (ROWPAIR ? 4 : 36);  // + slack read by discarded columns
  static constexpr int NK = (CK / 2) * 27;           // k-steps per chunk
  static constexpr int IN_FLOATS = CK * CH_STRIDE;   // input tile of one chunk
  static constexpr int BUF_FLOATS = IN_FLOATS + NK * NTT * 64;  // + the chunk's weight fragments
  static constexpr int LDS_FLOATS = 2 * BUF_FLOATS;  // double buffered
  // workgroups per CU: three where LDS admits them (row-group tiles: 43-49 KB; the compiler then keeps the kernel inside
  // 168 registers): 32 -> 32 at full resolution 142 -> 146 TFLOP/s
  static constexpr int WPE = (ROWPAIR && LDS_FLOATS * 4 * 3 <= 160 * 1024) ? 3 : 2;
  static_assert(ROWPAIR || P <= 64, "one wave stages one tile row per instruction");
  static_assert(CK % 2 == 0 && COUT % (32 * WN) == 0 && IN_FLOATS % 4 == 0, "shape");
  static_assert(!ROWPAIR || LIN || (G_ % 4 == 0 && TX % (G_ ? G_ : 1) == 0 && TY % GR == 0), "row-group tiles need TX % G == 0 and TY % (32 / G) == 0");
  static_assert(!LIN || (ROWPAIR && TY == 3 && TX % 4 == 0 && TX >= 32), "linear tiles: vector path, 3 + 2 staged rows, full-width rows");
  static_assert(!ROWPAIR || ((CK * IPC) % 4 == 0 && NT == 1 && LDS_FLOATS >= 4 * 32 * TR_PITCH), "row-pair staging / scratch");
};

// HEAD: the 48 x 4 row-pair tile of the 32 -> 32 classifier convolution with the 32 -> 1 head that follows it (PSMNet.py:46-54)
// inside its epilogue; see conv3d_s1_kernel.  Each workgroup leaves the head's partial sums over its own 4 x 4 x 48 voxels: a
// 6 x 6 x 50 tile (the voxels + the one-voxel halo their taps reach), summed over overlapping tiles by conv3d_head_chain_finish_kernel.
struct S1HeadCfg : S1Cfg<0, 32, 4, 48, 2, 1, 16, 0> {
  static constexpr bool HEAD = true;
  static constexpr int OZ = TZ + 2, OY = TY + 2, OX = TX + 2;
  static constexpr int OUT_FLOATS = OZ * OY * OX;   // one workspace slot
  // LDS row pitch of the tile: the two rows of a pair (GSTR * OP floats apart) start 16 banks apart, like the staged input
  static constexpr int OP = 56, OPLANE = OY * OP;
  static_assert(GSTR == 2 && XS == 3 && MT == 6 && OX % 2 == 0 && OX <= OP && (2 * OP) % 32 == 16, "head tile");
  static_assert(OZ * OPLANE + 64 <= LDS_FLOATS && (OZ * OPLANE) % 4 == 0, "the partial-sum tile lives in the freed chunk buffers");
};
constexpr int HEAD_PACKED_FLOATS = 16 * 64;   // 16 A fragments: taps (27, padded to 32) x one channel pair each
static_assert(HEAD_PACKED_FLOATS == DMB_CONV3D_HEAD_PACKED_FLOATS, "include/dmb_hip.h");

// WITH_RES: the residual operand is a compile-time property of the launch (two instantiations per tile shape).  The vector
// epilogue with its residual ring needs 3 - 5 registers more than the 168 that three workgroups per CU leave; as a run-time
// branch that meant spills -- a scratch segment -- for EVERY launch of the kernel, and a kernel with a scratch segment costs
// about 6 us of dispatch gap on either side of each launch (five of the six 32 -> 32 launches of a PSMNet step carry no
// residual).
// STATS (round 6, row-pair tiles of the training path): the epilogue also sums the RAW convolution outputs of its tile and their
// squares per channel -- FP64 per lane, the eight lanes of a channel by a fixed butterfly, the four waves in ascending order -- and
// writes one partial pair per workgroup and channel to stats[(ch * gridDim.x + blockIdx.x) * 2 + {0, 1}]: the batch statistics of
// the BatchNorm that follows (layers/basic_layers.py:68-83 under train()) without the pass over the output that
// dmb_bn_train_stats_f32 makes.  A separate instantiation: the inference kernels do not change.
template <class C, bool WITH_RES, bool STATS = false>
__global__ __launch_bounds__(256, C::WPE) void conv3d_s1_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ res, float* __restrict__ y, int Ci,
                                                           int D, int H, int W, int ntx, int nty, int ntz, int relu,
                                                           double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  // development build only (DMB_DBG is the constant 0 in the release build: these branches do not exist there) -- diagnostics
  // (option 6): 1 = no stores, 2 = no staging after the first chunk, 32 = no barrier in the chunk loop
  const int dbg = DMB_DBG((relu >> 8) & 0xff);
  relu &= 0xff;
  int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = t;         // (HEAD: the workspace slot)
  const int tx = t % ntx;     // LIN: ntx = 64-voxel runs per plane, nty = 1
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz;
  const int b = t / ntz;
  const int p0 = C::LIN ? tx * 64 : 0;                                   // LIN: first voxel of the run in its plane
  const int x0 = C::LIN ? 0 : tx * C::TX, y0 = C::LIN ? p0 / W : ty * C::TY, z0 = tz * C::TZ;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j = lane & 31, h = lane >> 5;
  const int wz = wave / C::WN, wn = wave % C::WN;
  const unsigned HW = (unsigned)H * W, DHW = (unsigned)D * HW;
  const float* xb = x + (size_t)b * Ci * DHW;

  f32x16 acc[C::MT][C::NT];   // started by the first chunk's first k-step (see `chunk`)

  // ---- staging (LDS-DMA).  Work unit = one (channel, z) plane of the haloed tile = ROWS row copies; the CK*ZS
  // planes of a chunk are dealt to the 4 waves in contiguous runs.  All copies of chunk i+1 (input rows + the
  // chunk's weight fragments) are issued before the MFMAs of chunk i and land while they run.
  constexpr int NPL = C::CK * C::ZS;            // planes per chunk
  static_assert(NPL % 4 == 0, "planes are dealt evenly to the 4 waves");
  constexpr int PPW = NPL / 4;                  // planes per wave
  constexpr int WCH = C::NK * C::NTT * 64;      // weight floats per chunk
  static_assert(WCH % 16 == 0, "weights are staged with 16-byte copies, evenly over 4 waves");
  constexpr int WPW = WCH / 16;                 // 16-byte words per wave
  constexpr int WI = (WPW + 63) / 64;           // copy instructions per wave
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wp, (unsigned)(cdiv(Ci, C::CK) * C::CK * 27 * C::COUT) * 4u);
  const int gx = x0 - 1 + lane;
  const unsigned xvoff = (lane < C::P && gx >= 0 && gx < W) ? (unsigned)gx * 4u : DMA_OOB;
  auto stage = [&](int c0, float* buf) {
    // the resource covers only this chunk's channels: 32-bit offsets then never limit the tensor size
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(xb + (size_t)c0 * DHW, (unsigned)min(C::CK, Ci - c0) * DHW * 4u);
    if constexpr (C::ROWPAIR) {
      // unit = 4 consecutive floats of a staged row; the units of one channel are linear in LDS
      constexpr int IPW = C::CK * C::IPC / 4;   // instructions per wave
#pragma unroll
      for (int q = 0; q < IPW; ++q) {
        const int id = wave * IPW + q, cl = id / C::IPC, qi = id - cl * C::IPC;
        const int u = qi * 64 + lane;
        const int zz = u / (C::ROWS * C::UPR), rr = u - zz * (C::ROWS * C::UPR), yy = rr / C::UPR, sg = rr - yy * C::UPR;
        const int gz = z0 - 1 + zz, gy = y0 - 1 + yy, gxs = x0 - 4 + sg * 4;
        const bool ok = c0 + cl < Ci && gz >= 0 && gz < D && gy >= 0 && gy < H && gxs >= 0 && gxs < W;
        if (u < C::UPC)
          dma16(xrs, ok ? ((unsigned)cl * DHW + (unsigned)gz * HW + (unsigned)gy * W + (unsigned)gxs) * 4u : DMA_OOB,
                0u, buf + cl * C::CH_STRIDE + qi * 256);
      }
    } else if (lane < C::P) {
#pragma unroll
      for (int q = 0; q < PPW; ++q) {
        const int pl = wave * PPW + q, cl = pl / C::ZS, zz = pl - cl * C::ZS;
        const int gz = z0 - 1 + zz;
        const bool zok = gz >= 0 && gz < D && c0 + cl < Ci;
        const unsigned zoff = ((unsigned)cl * DHW + (unsigned)max(gz, 0) * HW) * 4u;
        float* dpl = buf + cl * C::CH_STRIDE + zz * C::PLANE;
#pragma unroll
        for (int yy = 0; yy < C::ROWS; ++yy) {
          const int gy = y0 - 1 + yy;
          const bool ok = zok && gy >= 0 && gy < H;
          dma4(xrs, ok ? xvoff : DMA_OOB, ok ? zoff + (unsigned)gy * W * 4u : 0u, dpl + yy * C::P);
        }
      }
    }
    // weights: WCH/4 16-byte words split evenly over the 4 waves (WPW each, in WI instructions per wave), so that
    // every wave issues the same number of copies and a counted s_waitcnt vmcnt(N) means the same thing in all of them
#pragma unroll
    for (int i = 0; i < WI; ++i) {
      const int q4 = wave * WPW + i * 64 + lane;
      if (i * 64 + lane < WPW)
        dma16(wrs, (unsigned)q4 * 16u, (unsigned)(c0 / 2) * (27 * C::NTT * 64 * 4), buf + C::IN_FLOATS + (wave * WPW + i * 64) * 4);
    }
  };

  // LIN: where this lane's voxel of each column tile sits in the staged tile (rows y0 - 1 .. y0 + 3, full width)
  int lin_off[C::MT];
#pragma unroll
  for (int mt = 0; mt < C::MT; ++mt) {
    const int pos = p0 + mt * 32 + j, py = pos / W;
    lin_off[mt] = C::LIN ? (py - y0) * C::P + (pos - py * W) : 0;
  }
  const int NC = cdiv(Ci, C::CK);  // a partial last chunk reads zeros (bounds check) against zero-padded weights
  stage(0, lds);
  __syncthreads();
  // One chunk: FIRST = the launch's first chunk, whose first k-step starts the accumulators from the constant 0 operand of the
  // MFMA instead of from registers that would have to be cleared first (96 v_mov per wave, twice with this compiler's loop
  // lowering: 0.5 % of the shared ALU's time).
  auto chunk = [&](auto first_tag, int ci) {
    constexpr bool FIRST = decltype(first_tag)::value;
    const float* cur = lds + (ci & 1) * C::BUF_FLOATS;
    if (ci + 1 < NC && !(dbg & 2)) stage((ci + 1) * C::CK, lds + ((ci + 1) & 1) * C::BUF_FLOATS);  // lands while we compute
    // ---- NK k-steps on the current buffer; A and B fragments register double-buffered one k-step ahead ----
    const float* abase = cur + C::IN_FLOATS + (wn * C::NT) * 64 + lane;
    const float* bbase = cur + h * C::CH_STRIDE + wz * C::PLANE + (C::LIN ? 0 : C::lane_off(j)) + C::XOFF;
    float af[2][C::NT], bf[2][C::MT];
    auto load_frag = [&](int ks, float (&a)[C::NT], float (&bq)[C::MT]) {
      const int cp = ks / 27, tap = ks % 27;
      const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
#pragma unroll
      for (int nt = 0; nt < C::NT; ++nt) a[nt] = abase[(ks * C::NTT + nt) * 64];
      const float* bp = bbase + 2 * cp * C::CH_STRIDE + dz * C::PLANE + dy * C::P + dx;
#pragma unroll
      for (int mt = 0; mt < C::MT; ++mt) bq[mt] = bp[C::LIN ? lin_off[mt] : C::tile_off(mt)];
    };
    load_frag(0, af[0], bf[0]);
#pragma unroll
    for (int ks = 0; ks < C::NK; ++ks) {
      if (ks + 1 < C::NK) load_frag(ks + 1, af[(ks + 1) & 1], bf[(ks + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);  // keep the next step's LDS reads ahead of this step's MFMAs
#pragma unroll
      for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < C::NT; ++nt) {
          if (FIRST && ks == 0) {
            const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[mt][nt] = DMB_MFMA(af[0][nt], bf[0][mt], zero);
          } else {
            acc[mt][nt] = DMB_MFMA(af[ks & 1][nt], bf[ks & 1][mt], acc[mt][nt]);
          }
        }
      __builtin_amdgcn_sched_barrier(0);
    }
    if (!(dbg & 32)) __syncthreads();  // the compiler drains the DMA (vmcnt(0)) here: next buffer complete, current one free
  };
  chunk(std::true_type{}, 0);
  for (int ci = 1; ci < NC; ++ci) chunk(std::false_type{}, ci);

  // ---- epilogue ----
  if (dbg & 1) return;
  if constexpr (C::HEAD) {
    // The 32 -> 1 head on the matrix cores, straight from the accumulators:  P[tap][v] = sum_c w_head[c][tap] * act(y[c][v])  is a
    // GEMM with M = 27 taps (padded to 32), K = 32 channels, N = 32 voxels, and an accumulator tile already IS a stream of B
    // operands: lane (j, h) holds voxel j and, in register s, channel cd_row(s, h) -- K-step s takes register s of both lane halves
    // as its channel pair, the head weights are packed in that channel order (`res` = the 16 A fragments of
    // dmb_conv3d_head_pack_weights_f32).  No transposition, no store of the 32-channel tile.  P[tap][v] belongs to the output voxel
    // v - (tap - centre): the products are gathered into a 6 x 6 x 50 tile in LDS (the chunk buffers are free) in three phases, one
    // per dz, in which wave wz adds into plane wz + 2 - dz -- no two waves share a plane -- tap by tap, the two lane halves one
    // after the other (they hold different taps and may meet at an address; the 32 lanes of a half never do).
    // Every element so receives its terms in one fixed order.  `y` = the workspace: slot `tile` takes the 1800 partial sums,
    // contributions to voxels outside the volume included (conv3d_head_chain_finish_kernel drops them).
    float* ot = lds;                               // [OZ][OY][OP]
    float* tab = lds + C::OZ * C::OPLANE;          // [h][r]: scale, shift of channel cd_row(r, h)
    float aw[16];
#pragma unroll
    for (int s = 0; s < 16; ++s) aw[s] = res[s * 64 + lane];
    for (int i = threadIdx.x; i < C::OZ * C::OPLANE / 4; i += 256) reinterpret_cast<float4*>(ot)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (threadIdx.x < 32) {
      const int co = cd_row(threadIdx.x & 15, threadIdx.x >> 4);
      tab[threadIdx.x * 2] = scale ? scale[co] : 1.f;
      tab[threadIdx.x * 2 + 1] = shift ? shift[co] : 0.f;
    }
    __syncthreads();
    const float lo = relu ? 0.f : -__builtin_inff();
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float2 ss = *reinterpret_cast<const float2*>(tab + (h * 16 + r) * 2);
#pragma unroll
      for (int mt = 0; mt < C::MT; ++mt) acc[mt][0][r] = fmaxf(fmaf(acc[mt][0][r], ss.x, ss.y), lo);
    }
    // the products take over the registers of the accumulator tiles they consume
#pragma unroll
    for (int mt = 0; mt < C::MT; ++mt) {
      const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      f32x16 p = DMB_MFMA(aw[0], acc[mt][0][0], zero);
#pragma unroll
      for (int s = 1; s < 16; ++s) p = DMB_MFMA(aw[s], acc[mt][0][s], p);
      acc[mt][0] = p;
    }
    // voxels of a partial tile outside the volume are zero padding for the head, whatever the convolution computed there
#pragma unroll
    for (int mt = 0; mt < C::MT; ++mt) {
      const int gy = y0 + C::row_base(mt / C::XS) + C::GSTR * (j >> 4), gxo = x0 + (mt % C::XS) * 16 + (j & 15);
      const bool inb = z0 + wz < D && gy < H && gxo < W;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][0][r] = inb ? acc[mt][0][r] : 0.f;
    }
    // Plain read-add-write, not LDS atomics (measured: 162 ds_add_f32 per wave held the CU's LDS pipe long enough to stall the
    // B-fragment reads of the co-resident workgroups).  One tap of one lane half at a time: its six tiles are six distinct
    // addresses per lane and distinct across the 32 lanes, so they go as one batch; the next tap may meet them at an address
    // from another lane and must follow in program order (a wave's LDS instructions execute in order; the empty asm keeps the
    // compiler from moving a tap's reads above the previous tap's writes).
    float* ob = ot + (wz * C::OY + C::GSTR * (j >> 4)) * C::OP + (j & 15);
#pragma unroll
    for (int dz = 0; dz < 3; ++dz) {
      if (dz) __syncthreads();
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        if (h != hh) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int tap = cd_row(r, hh);
          if (tap >= 27 || tap / 9 != dz) continue;
          float cur[C::MT];
#pragma unroll
          for (int mt = 0; mt < C::MT; ++mt) {
            const int o0 = ((2 - dz) * C::OY + C::row_base(mt / C::XS) + 2) * C::OP + (mt % C::XS) * 16 + 2;
            cur[mt] = ob[o0 - ((tap / 3) % 3) * C::OP - tap % 3];
          }
#pragma unroll
          for (int mt = 0; mt < C::MT; ++mt) {
            const int o0 = ((2 - dz) * C::OY + C::row_base(mt / C::XS) + 2) * C::OP + (mt % C::XS) * 16 + 2;
            ob[o0 - ((tap / 3) % 3) * C::OP - tap % 3] = cur[mt] + acc[mt][0][r];
          }
          asm volatile("" ::: "memory");
        }
      }
    }
    __syncthreads();
    float* wt = y + (size_t)tile * C::OUT_FLOATS;
    for (int i = threadIdx.x; i < C::OUT_FLOATS / 2; i += 256) {
      const int rw = i / (C::OX / 2), c2 = i - rw * (C::OX / 2);
      *reinterpret_cast<float2*>(wt + rw * C::OX + c2 * 2) = *reinterpret_cast<const float2*>(ot + rw * C::OP + c2 * 2);
    }
    return;
  }
  const int gz = z0 + wz;
  float* yb = y + (size_t)b * C::COUT * DHW;
  const float* rb = res ? res + (size_t)b * C::COUT * DHW : nullptr;
  if constexpr (C::ROWPAIR) {
    // Each 32 x 32 accumulator tile goes through a per-wave LDS scratch (the chunk buffers are free after the last
    // barrier) so that a lane owns 4 consecutive x of one channel: 16-byte stores / residual loads, 4x fewer
    // vector-memory instructions.  Buffer addressing with an out-of-range offset for lanes outside the volume keeps
    // the code branch-free; residual loads run one tile ahead of the stores.
    float* my = lds + wave * (32 * C::TR_PITCH);
    const __amdgpu_buffer_rsrc_t yrs = make_rsrc(yb, (unsigned)C::COUT * DHW * 4u);
    const __amdgpu_buffer_rsrc_t rrs = make_rsrc(rb ? rb : yb, (unsigned)C::COUT * DHW * 4u);
    const int px = (lane & 7) * 4;
    const float lo = relu == 1 ? 0.f : -__builtin_inff();    // ReLU after the residual add
    const float lo2 = relu == 2 ? 0.f : -__builtin_inff();   // ReLU before it (GC-Net)
    float sc4[4], sh4[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int co = wn * 32 + k * 8 + (lane >> 3);
      sc4[k] = scale ? scale[co] : 1.f;
      sh4[k] = shift ? shift[co] : 0.f;
    }
    // a tile's four 16-byte words per lane are 8 channels apart: one per-lane offset per tile (out of range for lanes outside
    // the volume; adding the channel steps keeps it out of range) instead of four -- the eight offset registers of two tiles in
    // flight were what pushed this epilogue past 168 registers (3 spills = a scratch segment for the kernel, and a kernel with
    // a scratch segment costs ~6 us of dispatch gap on either side of every launch)
    const unsigned kstep = 8u * DHW * 4u;
    auto offset0 = [&](int mt) {
      if constexpr (C::LIN) {   // 4 consecutive voxels of the run (H * W % 4 == 0: a word never straddles the end of the plane)
        const unsigned pos = (unsigned)(p0 + mt * 32 + px);
        return (gz < D && pos < HW) ? ((unsigned)(wn * 32 + (lane >> 3)) * DHW + (unsigned)gz * HW + pos) * 4u : DMA_OOB;
      }
      const int gy = y0 + C::row_base(mt / C::XS) + C::GSTR * (px / C::G), gxo = x0 + (mt % C::XS) * C::G + px % C::G;
      const bool inb = gz < D && gy < H && gxo < W;
      return inb ? ((unsigned)(wn * 32 + (lane >> 3)) * DHW + (unsigned)gz * HW + (unsigned)gy * W + (unsigned)gxo) * 4u : DMA_OOB;
    };
    auto run = [&](auto has_res) {
      constexpr bool HAS_RES = decltype(has_res)::value;
      // Skip-operand loads run ahead of the stores in a ring of three register sets: tile 1 is requested when tile 0 is
      // processed, from then on TWO tiles ahead -- the accumulator registers of the tiles already written out pay for the third
      // set, so the register peak stays where the first tile puts it (96 accumulators + 2 sets).
      unsigned off0[C::MT];
      u32x4 rv[3][4];
      double ssum[STATS ? 4 : 1], ssq[STATS ? 4 : 1];   // this lane's channels k * 8 + (lane >> 3)
      (void)ssum, (void)ssq;
      if constexpr (STATS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) ssum[k] = ssq[k] = 0.0;
      }
#pragma unroll
      for (int mt = 0; mt < C::MT; ++mt) off0[mt] = 0;
      off0[0] = offset0(0);
      auto request = [&](int t) {
        off0[t] = offset0(t);
        if constexpr (HAS_RES) {
#pragma unroll
          for (int k = 0; k < 4; ++k) rv[t % 3][k] = __builtin_amdgcn_raw_buffer_load_b128(rrs, (int)(off0[t] + k * kstep), 0, 0);
        }
      };
      request(0);
#pragma unroll
      for (int mt = 0; mt < C::MT; ++mt) {
        if (mt <= 1 && mt + 1 < C::MT) request(mt + 1);   // tiles 1 and 2: one ahead (at mt = 0 all six accumulator tiles are live)
        if (mt >= 1 && mt + 2 < C::MT) request(mt + 2);   // from tile 3 on: two ahead
#pragma unroll
        for (int r = 0; r < 16; ++r) my[cd_row(r, h) * C::TR_PITCH + j] = acc[mt][0][r];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float4 v = *reinterpret_cast<const float4*>(my + (k * 8 + (lane >> 3)) * C::TR_PITCH + px);
          if constexpr (STATS) {   // four voxels of one channel: summed and squared in FP64 (the square of an FP32 value is exact
                                   // there; rounded to FP32 first, E[x^2] - mean^2 lost the variance from |mean| / std ~ 1e2 on)
            if (off0[mt] != DMA_OOB) {
              const double vx = (double)v.x, vy = (double)v.y, vz = (double)v.z, vw = (double)v.w;
              ssum[k] += (vx + vy) + (vz + vw);
              ssq[k] += fma(vx, vx, fma(vy, vy, fma(vz, vz, vw * vw)));
            }
          }
          v.x = fmaxf(fmaf(v.x, sc4[k], sh4[k]), lo2);
          v.y = fmaxf(fmaf(v.y, sc4[k], sh4[k]), lo2);
          v.z = fmaxf(fmaf(v.z, sc4[k], sh4[k]), lo2);
          v.w = fmaxf(fmaf(v.w, sc4[k], sh4[k]), lo2);
          if constexpr (HAS_RES) {   // (not __builtin_bit_cast on a vector element: this clang reads element 0 for every index)
            v.x += __uint_as_float(rv[mt % 3][k].x);
            v.y += __uint_as_float(rv[mt % 3][k].y);
            v.z += __uint_as_float(rv[mt % 3][k].z);
            v.w += __uint_as_float(rv[mt % 3][k].w);
          }
          u32x4 o;
          o.x = __float_as_uint(fmaxf(v.x, lo));
          o.y = __float_as_uint(fmaxf(v.y, lo));
          o.z = __float_as_uint(fmaxf(v.z, lo));
          o.w = __float_as_uint(fmaxf(v.w, lo));
          __builtin_amdgcn_raw_buffer_store_b128(o, yrs, (int)(off0[mt] + k * kstep), 0, 0);   // (streaming stores: step +0.3 %)
        }
      }
      if constexpr (STATS) {
        // the eight lanes of a channel (lane & 7), then the four waves (z-slices) through LDS behind the transposition scratch
        static_assert(C::NT == 1 && C::LDS_FLOATS >= 4 * 32 * C::TR_PITCH + 4 * 32 * 4, "statistics scratch");
        double* sred = reinterpret_cast<double*>(lds + 4 * 32 * C::TR_PITCH);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
          for (int o = 1; o < 8; o <<= 1) {
            ssum[k] += __shfl_xor(ssum[k], o, 64);
            ssq[k] += __shfl_xor(ssq[k], o, 64);
          }
          if ((lane & 7) == 0) {
            sred[(wave * 32 + k * 8 + (lane >> 3)) * 2] = ssum[k];
            sred[(wave * 32 + k * 8 + (lane >> 3)) * 2 + 1] = ssq[k];
          }
        }
        __syncthreads();
        if (threadIdx.x < 64) {
          const int ch = threadIdx.x >> 1, st = threadIdx.x & 1;
          const double tot = ((sred[(0 * 32 + ch) * 2 + st] + sred[(1 * 32 + ch) * 2 + st]) + sred[(2 * 32 + ch) * 2 + st]) + sred[(3 * 32 + ch) * 2 + st];
          stats[((size_t)(wn * 32 + ch) * gridDim.x + blockIdx.x) * 2 + st] = tot;
        }
      }
    };
    run(std::integral_constant<bool, WITH_RES>{});
    return;
  }
  if (gz >= D) return;
#pragma unroll
  for (int nt = 0; nt < C::NT; ++nt) {
    const int co0 = (wn * C::NT + nt) * 32;
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + cd_row(r, h);
      sc[r] = scale ? scale[co] : 1.f;
      sh[r] = shift ? shift[co] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < C::MT; ++mt) {
      int ly, lx;
      bool valid;
      C::decode(mt, j, ly, lx, valid);
      const int gy = y0 + ly, gxo = x0 + lx;
      if (valid && gy < H && gxo < W) {
        const f32x16 a1[1] = {acc[mt][nt]};
        store_tile<1>(a1, sc, sh, rb, yb, co0, h, DHW, (unsigned)gz * HW + (unsigned)gy * W + gxo, relu);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Fused classifier head (conv3d_s1_kernel on S1HeadCfg): weight pack and the pass that finishes it.
//   whp[s * 64 + lane] = w[c = cd_row(s, lane >> 5)][tap = lane & 31]   (taps 27 .. 31: zero rows)
// ---------------------------------------------------------------------------------------------------------
__global__ void pack_head_weights_kernel(const float* __restrict__ w, float* __restrict__ whp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= HEAD_PACKED_FLOATS) return;
  const int lane = i & 63, s = i >> 6, tap = lane & 31;
  whp[i] = tap < 27 ? w[cd_row(s, lane >> 5) * 27 + tap] : 0.f;
}

// The pass that finishes a CHAIN of N <= 4 fused heads (PSMNet.py:70-72: cost_k = classif_k(out_k) + cost_{k-1}) in one launch:
//   c_1[v] = (the partial sums of the at most eight tiles of ws_1 whose 6 x 6 x 50 slot covers v, in ascending tile order) + b_1 (+ res[v])
//   c_k[v] = ((the same sum over ws_k) + b_k) + c_{k-1}[v]
// -- per level the additions of a finishing pass of its own, in their order; c_{k-1} stays in registers instead of being read back.
// A thread owns four consecutive x of one row: TX % 4 == 0, so they lie in one tile and a slot row holds them as 16 contiguous
// bytes (ox = lx + 1 .. lx + 4); only the first column of a tile has a term in the left neighbour's slot (ox = OX - 1) and only the
// last column one in the right neighbour's (ox = 0).  Along z and y a voxel is covered by its own tile and, on the tile's first /
// last plane or row, by ONE neighbour: two candidates per axis, ascending.  All loads of all levels are issued before the first
// addition (N independent groups per thread).  VEC: y and res are 16-byte aligned (4-byte otherwise: dword accesses).
struct HeadChain {
  const float* ws[4];
  float* y[4];
  float bias[4];
};
struct __attribute__((packed, aligned(4))) HeadQuad {
  float v[4];
};

template <int N, bool VEC>
__global__ __launch_bounds__(256) void conv3d_head_chain_finish_kernel(HeadChain ch, const float* __restrict__ res, int D, int H, int W,
                                                                       int ntx, int nty, int ntz, long long groups) {
  using C = S1HeadCfg;
  static_assert(C::TX % 4 == 0 && C::OZ == C::TZ + 2 && C::OY == C::TY + 2 && C::OX == C::TX + 2, "four columns of a thread share a tile");
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const int W4 = W / 4;
  const int gx = (int)(g % W4) * 4;
  long long q = g / W4;
  const int gy = (int)(q % H);
  q /= H;
  const int gz = (int)(q % D), b = (int)(q / D);
  const int tz = gz / C::TZ, ty = gy / C::TY, tx = gx / C::TX;
  const int lz = gz - tz * C::TZ, ly = gy - ty * C::TY, lx = gx - tx * C::TX;
  // candidate 0 / 1 per axis: (tile, plane or row inside its slot); candidate 0 always exists
  const bool zlo = lz == 0 && tz > 0, zhi = lz == C::TZ - 1 && tz + 1 < ntz;
  const bool ylo = ly == 0 && ty > 0, yhi = ly == C::TY - 1 && ty + 1 < nty;
  const int zt[2] = {zlo ? tz - 1 : tz, zlo ? tz : tz + 1}, zo[2] = {zlo ? C::TZ + 1 : lz + 1, zlo ? 1 : 0};
  const int yt[2] = {ylo ? ty - 1 : ty, ylo ? ty : ty + 1}, yo[2] = {ylo ? C::TY + 1 : ly + 1, ylo ? 1 : 0};
  const bool zv = zlo || zhi, yv = ylo || yhi;
  const bool left = lx == 0 && tx > 0, right = lx == C::TX - 4 && tx + 1 < ntx;
  bool valid[4];
  size_t at[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    valid[i] = ((i >> 1) == 0 || zv) && ((i & 1) == 0 || yv);
    const size_t slot = (((size_t)b * ntz + zt[i >> 1]) * nty + yt[i & 1]) * ntx + tx;
    at[i] = slot * C::OUT_FLOATS + (zo[i >> 1] * C::OY + yo[i & 1]) * C::OX;
  }
  HeadQuad own[N][4];
  float lf[N][4], rt[N][4];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const float* __restrict__ ws = ch.ws[k];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!valid[i]) continue;
      own[k][i] = *reinterpret_cast<const HeadQuad*>(ws + at[i] + lx + 1);
      if (left) lf[k][i] = ws[at[i] - C::OUT_FLOATS + C::OX - 1];
      if (right) rt[k][i] = ws[at[i] + C::OUT_FLOATS];
    }
  }
  const size_t idx = (size_t)g * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f};   // c_{k-1}
  if (res) {
    if constexpr (VEC) {
      const float4 r = *reinterpret_cast<const float4*>(res + idx);
      s[0] = r.x, s[1] = r.y, s[2] = r.z, s[3] = r.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] = res[idx + j];
    }
  }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    float t[4];
    // candidate 0 (always there): the left neighbour's term, if any, comes first
    t[0] = left ? lf[k][0] + own[k][0].v[0] : own[k][0].v[0];
    t[1] = own[k][0].v[1];
    t[2] = own[k][0].v[2];
    t[3] = right ? own[k][0].v[3] + rt[k][0] : own[k][0].v[3];
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      if (!valid[i]) continue;
      if (left) t[0] += lf[k][i];
#pragma unroll
      for (int j = 0; j < 4; ++j) t[j] += own[k][i].v[j];
      if (right) t[3] += rt[k][i];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      t[j] += ch.bias[k];
      if (k > 0 || res) t[j] += s[j];
      s[j] = t[j];
    }
    float* __restrict__ y = ch.y[k];
    if constexpr (VEC) {
      *reinterpret_cast<float4*>(y + idx) = make_float4(s[0], s[1], s[2], s[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) y[idx + j] = s[j];
    }
  }
}

template <class C>
static int launch_s1(const float* x, const float* wp, const float* scale, const float* shift, const float* res,
                     float* y, int B, int Ci, int D, int H, int W, int relu, hipStream_t st) {
  const int ntx = C::LIN ? cdiv(H * W, 64) : cdiv(W, C::TX), nty = C::LIN ? 1 : cdiv(H, C::TY), ntz = cdiv(D, C::TZ);
  const long long nblk = (long long)B * ntx * nty * ntz;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d: grid too large");
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  if (res) {
    DMB_ENSURE_LDS((&conv3d_s1_kernel<C, true>), (size_t)(lds));
    hipLaunchKernelGGL((conv3d_s1_kernel<C, true>), dim3((unsigned)nblk), dim3(256), lds, st, x, wp, scale, shift, res, y, Ci, D,
                       H, W, ntx, nty, ntz, relu, (double*)nullptr);
  } else {
    DMB_ENSURE_LDS((&conv3d_s1_kernel<C, false>), (size_t)(lds));
    hipLaunchKernelGGL((conv3d_s1_kernel<C, false>), dim3((unsigned)nblk), dim3(256), lds, st, x, wp, scale, shift, res, y, Ci, D,
                       H, W, ntx, nty, ntz, relu, (double*)nullptr);
  }
  return launch_status("conv3d stride-1 launch failed");
}

// The raw convolution (no affine, skip or ReLU) with the per-workgroup channel sums of its output (conv3d_s1_kernel, STATS).
template <class C>
static int launch_s1_stats(const float* x, const float* wp, float* y, double* stats, int B, int Ci, int D, int H, int W, hipStream_t st) {
  const int ntx = cdiv(W, C::TX), nty = cdiv(H, C::TY), ntz = cdiv(D, C::TZ);
  const long long nblk = (long long)B * ntx * nty * ntz;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d: grid too large");
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  DMB_ENSURE_LDS((&conv3d_s1_kernel<C, false, true>), (size_t)(lds));
  hipLaunchKernelGGL((conv3d_s1_kernel<C, false, true>), dim3((unsigned)nblk), dim3(256), lds, st, x, wp, (const float*)nullptr,
                     (const float*)nullptr, (const float*)nullptr, y, Ci, D, H, W, ntx, nty, ntz, 0, stats);
  return launch_status("conv3d stride-1 (+ statistics) launch failed");
}

// ---- Tile choice for the stride-1 kernel ---------------------------------------------------------------------------
// Every row-group tile shape works for ANY volume with 16-byte rows (W % 4 == 0, aligned bases): partial tiles are zero-filled
// by the staging's bounds checks and masked in the epilogue.  Which one runs is a cost estimate over the instantiated shapes --
// rounds of workgroups the launch needs on this chip x resident workgroups per CU x the matrix work of one workgroup -- not a
// table of image widths: e.g. 240 columns -> 48-column row pairs (5 tiles, nothing discarded), 312 columns (KITTI, 1248 / 4) ->
// 24-column row quads of 8 rows (13 tiles, nothing discarded), 156 -> 40-column row quads (4 tiles, 2.5 % discarded).
// Without 16-byte rows: the flattened mapping (dword staging) with the TX (60 or 52) that wastes fewer columns.
constexpr double S1_EFF_32x2 = 1.0;    // 32 x 2 row pairs (two column tiles per wave): measured rate relative to the estimate, profiles/r05_kbench_small_32.log
struct S1Tile {
  int tx, ty, tz, mt;   // tile extent, 32-voxel column tiles per wave
  bool lin;             // 64-voxel runs of the (y, x) plane instead of boxes
  double eff;           // measured rate of the shape on volumes it tiles exactly, relative to the 48 x 4 row pairs
};
// A family of candidates is ONE list of S1Cfg types (+ its measured rates): what the estimate reads of a tile comes from the type,
// and s1_visit is the only place where a pick index becomes an instantiation.
template <class C>
constexpr S1Tile s1_tile(double eff) { return {C::TX, C::TY, C::TZ, C::MT, C::LIN, eff}; }
template <class Tiles, size_t... I>
constexpr std::array<S1Tile, sizeof...(I)> s1_tiles(const double (&eff)[sizeof...(I)], std::index_sequence<I...>) {
  return {{s1_tile<std::tuple_element_t<I, Tiles>>(eff[I])...}};
}
// f(C{}) for the pick-th type of the list, once (an index past the list: its last type)
template <class Tiles, class F, size_t... I>
static auto s1_visit(int pick, F&& f, std::index_sequence<I...>) {
  decltype(f(std::tuple_element_t<0, Tiles>{})) r{};
  (void)(((pick == (int)I || I + 1 == sizeof...(I)) && ((r = f(std::tuple_element_t<I, Tiles>{})), true)) || ...);
  return r;
}
static double s1_cost(const S1Tile& t, int B, int D, int H, int W, int ncu) {
  const long long n = t.lin ? (long long)B * cdiv(D, t.tz) * cdiv(H * W, 64)
                            : (long long)B * cdiv(D, t.tz) * cdiv(H, t.ty) * cdiv(W, t.tx);
  // What a CU holds is ceil(n / CUs) workgroups, each with one wave per SIMD running `mt` column tiles -- serial chains of
  // 27 Ci / 2 MFMAs -- one after the other; + 0.1: set-up and epilogue of a workgroup in units of one column tile's arithmetic.
  // (Round 4 counted rounds of `wpe` co-resident workgroups instead: the same ranking on full grids, but a step function at
  // n = wpe x CUs that misjudged launches around one round -- batch 1, small images.)  Checked against every candidate measured
  // so far: profiles/r04_kbench_hg*.log (batch 4: 240 / 120 / 60 and 312 / 156 columns) and profiles/r05_kbench_small.log (batch 1
  // at 256x512 / D 64, 544x960 and 384x1248) -- the estimate ranks them as measured.
  return (double)cdiv_ll(n, ncu) * (t.mt + 0.1) / t.eff;
}
// index of the cheapest candidate (ties: the earlier one)
static int s1_pick(const S1Tile* cand, const bool* ok, int n, int B, int D, int H, int W, int ncu) {
  int best = -1;
  double bc = 0.0;
  for (int i = 0; i < n; ++i) {
    if (!ok[i]) continue;
    const double c = s1_cost(cand[i], B, D, H, W, ncu);
    if (best < 0 || c < bc) best = i, bc = c;
  }
  return best;
}
static int flat_tx(int W) {
  const int w60 = cdiv(W, 60) * 60, w52 = cdiv(W, 52) * 52;
  // useful fraction = W / padded width * (TX / (TX + 2)) * (TY*P / (MT*32))
  const double e60 = (double)W / w60 * (60.0 / 62.0) * (248.0 / 256.0);
  const double e52 = (double)W / w52 * (52.0 / 54.0) * (216.0 / 224.0);
  return e52 > e60 ? 52 : 60;
}

// The 32-channel row-pair / row-quad tiles of the vector path: 0 = 48 x 4, 1 = 24 x 8, 2 = 32 x 4, 3 = 32 x 2
// row pairs (16 columns x 2 rows per 32-voxel column tile) of 48 or 32 columns x 4 rows, row quads (8 x 4) of 24 columns x 8
// rows; one z-slice per wave, three workgroups per CU each
// (8-row quads stage a quarter more halo rows per byte of output and store 32-byte instead of 64-byte runs: 0.972)
using S1Tiles32 = std::tuple<S1Cfg<0, 32, 4, 48, 2, 1, 16, 0>, S1Cfg<0, 32, 8, 24, 2, 1, 8, 40>, S1Cfg<0, 32, 4, 32, 2, 1, 16, 0>,
                             S1Cfg<0, 32, 2, 32, 2, 1, 16, 0>>;
constexpr double S1Eff32[4] = {1.0, 0.972, 1.0, S1_EFF_32x2};
// the fused head (S1HeadCfg) is candidate 0 with another epilogue: its workspace has one slot per workgroup of that tile
constexpr int S1_HEAD_PICK = 0;
static_assert(std::is_base_of_v<std::tuple_element_t<S1_HEAD_PICK, S1Tiles32>, S1HeadCfg>, "the head's tile is a candidate of the plain launch");
template <class F>
static auto s1_visit32(int pick, F&& f) { return s1_visit<S1Tiles32>(pick, f, std::make_index_sequence<4>{}); }
static int s1_pick32(int B, int D, int H, int W, int ncu) {
  static constexpr auto cand = s1_tiles<S1Tiles32>(S1Eff32, std::make_index_sequence<4>{});
  const bool ok[4] = {true, true, true, true};
  int pick = s1_pick(cand.data(), ok, 4, B, D, H, W, ncu);
  // (round 6) a launch of at most ONE 32 x 4 workgroup per CU: two 32 x 2 workgroups per CU instead, so that one's prologue and
  // epilogue fall under the other's multiply phase ([1, 32, 16, 64, 128]: 57.6 -> 55.7 us, profiles/r06_sk_probe_midsizes.log)
  if (pick == 2 && (long long)B * cdiv(D, 4) * cdiv(H, 4) * cdiv(W, 32) <= ncu) pick = 3;
  return pick;
}
static long long s1_blocks32(int pick, int B, int D, int H, int W) {
  return s1_visit32(pick, [&](auto c) {
    using C = decltype(c);
    return (long long)B * cdiv(W, C::TX) * cdiv(H, C::TY) * cdiv(D, C::TZ);
  });
}

// The 64-channel tiles of the vector path: 64-voxel runs of the plane in memory order for rows of up to 64 voxels (planes no box
// tiling fills the chip with: the deepest hourglass level), row quads of 40 / 24 / 32 columns x 4 rows otherwise; two z-slices x two
// channel tiles per workgroup.  A launch here is only a few rounds of workgroups deep, so the estimate decides per launch.
// (round 5) + row pairs of 16 columns x 2 rows: ONE column tile per wave, for launches that do not fill the chip (batch 1,
// small images: 62 -> 37 us at [1, 64, 8, 32, 64], 59 -> 33 us at [1, 64, 4, 16, 32]); twice the halo per output of the quads
// (round 6: chunks of four input channels for this tile -- a chunk of two is 27 MFMAs per wave between two barriers, less than
// the copies' round trip: [1, 64, 8, 32, 64] 33.5 -> 31.6 us, [1, 64, 12, 34, 60] 59.6 -> 56.0 us; two workgroups per CU)
using S1Tiles64 = std::tuple<S1Cfg<0, 64, 3, 64, 2, 2, 16, 0, true>, S1Cfg<0, 64, 4, 40, 2, 2, 8, 56>, S1Cfg<0, 64, 4, 24, 2, 2, 8, 40>,
                             S1Cfg<0, 64, 4, 32, 2, 2, 8, 40>, S1Cfg<0, 64, 2, 16, 4, 2, 16, 0>>;
constexpr double S1Eff64[5] = {1.0, 1.0, 1.0, 1.0, 0.95};
// the runs (candidate 0) take rows of 32 .. 64 voxels and planes of whole 16-byte words; `runs` = false: the box tiles only
static bool s1_runs_ok(int H, int W) { return W >= 32 && W <= 64 && (H * W) % 4 == 0; }
static int s1_pick64(int B, int D, int H, int W, int ncu, bool runs) {
  static constexpr auto cand = s1_tiles<S1Tiles64>(S1Eff64, std::make_index_sequence<5>{});
  const bool ok[5] = {runs && s1_runs_ok(H, W), true, true, true, true};
  return s1_pick(cand.data(), ok, 5, B, D, H, W, ncu);
}

// f(C{}) for the instantiation a stride-1 plan code names: the one place where a code becomes a type, for the plan's own
// workgroup count and for the launch
template <class F>
static auto s1_form(int plan, F&& f) {
  const int form = plan >> 8, k = plan & 0xff;
  if (form == CONV_S1_VEC) return k < 4 ? s1_visit32(k, f) : s1_visit<S1Tiles64>(k - 4, f, std::make_index_sequence<5>{});
  if (form == CONV_S1_FLAT) {
    if (k == 0) return f(S1Cfg<0, 32, 4, 60, 2, 1, 0, 0>{});
    if (k == 1) return f(S1Cfg<0, 32, 4, 52, 2, 1, 0, 0>{});
    if (k == 2) return f(S1Cfg<0, 64, 4, 60, 2, 2, 0, 0>{});
    return f(S1Cfg<0, 64, 4, 52, 2, 2, 0, 0>{});
  }
  // CONV_S1_C128, GC-Net's deepest level: 2 waves x 2 row tiles, 2-row tiles keep the accumulators at 160 registers
  return f(S1Cfg<0, 128, 2, 60, 2, 2, 0, 0>{});
}

int conv3d_s1_plan(const ConvDesc& d, const char** why) {
  const int B = d.B, Co = d.Co, D = d.D, H = d.H, W = d.W;
  const bool out_small = (long long)Co * D * H * W * 4 < 0x7fffffffLL;   // the vector epilogue addresses the whole output item
  // the vector path: 16-byte rows for staging, skip operand and stores
  const bool vec = W % 4 == 0 && d.x_align >= 16 && d.y_align >= 16 && d.res_align >= 16 && out_small;
  if (Co != 32 && Co != 64 && Co != 128) return *why = CONV3D_UNSUPPORTED, -DMB_EUNSUPPORTED;
  const int flat = (Co == 64 ? 2 : 0) + (flat_tx(W) == 52 ? 1 : 0);   // the flattened tile of this width
  int form = Co == 128 ? CONV_S1_C128 : (vec ? CONV_S1_VEC : CONV_S1_FLAT), k = 0;
  if (form == CONV_S1_VEC) k = Co == 32 ? s1_pick32(B, D, H, W, d.ncu) : 4 + s1_pick64(B, D, H, W, d.ncu, true);
  if (form == CONV_S1_FLAT) k = flat;
  // ---- development switches (the release build has none): the one place where they act on a stride-1 plan
  if (form == CONV_S1_VEC) {
    const int first = Co == 32 ? 0 : 4, n = Co == 32 ? 4 : 5, force = DMB_OPT(19);   // 19 = k: candidate k - 1 of the list in play
    if (force > 0 && force <= n && (first + force - 1 != 4 || s1_runs_ok(H, W))) k = first + force - 1;
    if (DMB_OPT(13) && k == 4) k = 4 + s1_pick64(B, D, H, W, d.ncu, false);   // 13: boxes instead of runs
    if (DMB_OPT(2)) form = CONV_S1_FLAT, k = flat;                             // 2: flattened tiles
  }
  const int plan = (form << 8) | k;
  const long long nblk = s1_form(plan, [&](auto c) {
    using C = decltype(c);
    return (long long)B * (C::LIN ? cdiv(H * W, 64) : cdiv(W, C::TX) * cdiv(H, C::TY)) * cdiv(D, C::TZ);
  });
  if (nblk > 0x7fffffffLL) return *why = "conv3d: grid too large", -DMB_EUNSUPPORTED;
  return plan;
}

int conv3d_s1_run(int plan, const float* x, const float* wpack, const float* scale, const float* shift, const float* residual, float* y,
                  int B, int Ci, int D, int H, int W, int relu, hipStream_t st) {
  return s1_form(plan, [&](auto c) { return launch_s1<decltype(c)>(x, wpack, scale, shift, residual, y, B, Ci, D, H, W, relu, st); });
}

// ---------------------------------------------------------------------------------------------------------
// Stride-2 kernel (k3, pad 1): input voxel = 2*out - 1 + tap.  LDS tile rows are split by y parity so that
// a flattened output index m = ly*(TX+1) + lx maps to LDS offset 2*m + const(tap); the x stride of 2 floats
// is a harmless 2-way bank conflict (LDS has > 4x headroom next to a 64-cycle MFMA).
// ---------------------------------------------------------------------------------------------------------
// V16 (W % 4 == 0, aligned base): rows are staged with 16-byte LDS-DMA words from the aligned column 2*x0 - 4 (XOFF = 3
// unused floats in front of the halo column), row pitch 64 floats = output-position pitch 32: with dword copies a
// stride-2 tile (4x the input per output) cost more TA cycles than its MFMAs cost matrix-core cycles.
// WM: wave groups along the output positions.  WM = 2 makes a workgroup of EIGHT waves on the same LDS tile, each with half of
// the tile's 32-position column tiles (32 instead of 64 accumulator registers): two workgroups per CU (the LDS bound) then
// put four waves on every SIMD instead of two, so that one wave's staging waits and epilogue hide behind three others.
// VEP (with V16): the epilogue goes through a per-wave LDS scratch so that a lane owns TWO adjacent output columns of one channel
// and stores them as one 8-byte word (16 bytes would need 4-column alignment, and a 30-column tile starts on an odd pair in every
// second tile): a CU retires vector-memory lanes at about one per clock whatever their width, and the dword epilogue's 50 M lane
// stores of the 32 -> 64 layer were 0.08 of its 0.72 ms (diagnostic switch 1).
template <int CIN_, int COUT_, int TY_, int TX_, int CK_, int WN_, bool V16_ = false, int WM_ = 1, bool VEP_ = false>
struct S2Cfg {
  static constexpr int CIN = CIN_, COUT = COUT_, TY = TY_, TX = TX_, CK = CK_, WN = WN_;
  static constexpr bool V16 = V16_, VEP = V16_ && VEP_;
  static constexpr int TR_PITCH = 40;          // epilogue transposition scratch [32 channels][32 + 8]: = 8 (mod 16), see the kernel
  static constexpr int WM = WM_, NWAVES = 4 * WM_, NTHREADS = 64 * NWAVES;
  static constexpr int WZ = 4 / WN;
  static constexpr int TZ = WZ;
  static constexpr int XOFF = V16 ? 3 : 0;
  static constexpr int PO = V16 ? (XOFF + 2 * TX + 1 + 7) / 8 * 4 : TX + 1;   // output-position pitch
  static constexpr int R = 2 * PO;             // LDS row pitch (input columns 2*x0-1 .. 2*x0+2*TX-1, padded)
  static constexpr int PYPL = (TY + 1) * R;    // one y-parity plane
  static constexpr int ZPL = 2 * PYPL;         // one input z-slice
  static constexpr int ZS = 2 * TZ + 1;
  static constexpr int INROWS = 2 * TY + 1;
  static constexpr int INCOLS = 2 * TX + 1;
  static constexpr int MT = (TY * PO + 31) / 32;
  static constexpr int MTW = MT / WM;          // column tiles per wave
  static constexpr int NTT = COUT / 32;
  static constexpr int NT = NTT / WN;
  static constexpr int CH_STRIDE = ZS * ZPL + 72;
  static constexpr int UPR = R / 4, UPC = ZS * ZPL / 4;      // vector path: 16-byte units per row / per channel
  static constexpr int IPC = (UPC + 63) / 64;                // copy instructions per channel
  static constexpr int NK = (CK / 2) * 27;
  static constexpr int IN_FLOATS = CK * CH_STRIDE;
  static constexpr int BUF_FLOATS = IN_FLOATS + NK * NTT * 64;
  static constexpr int LDS_FLOATS = 2 * BUF_FLOATS;  // double buffered
  static constexpr int WPE = (LDS_FLOATS * 4 * 2 <= 160 * 1024) ? 2 : 1;  // workgroups per CU the LDS admits
  static_assert(CK % 2 == 0 && COUT % (32 * WN) == 0 && IN_FLOATS % 4 == 0, "shape");
  static_assert(LDS_FLOATS * 4 <= 160 * 1024, "LDS budget");
  static_assert(MT % WM == 0, "the column tiles are dealt evenly to the wave groups");
  static_assert(!VEP || (PO % 2 == 0 && TX % 2 == 0 && LDS_FLOATS >= NWAVES * 32 * TR_PITCH), "pair epilogue: even tiles, scratch");
};

template <class C>
// (HIP: the second launch-bounds figure is the minimum number of WAVES PER SIMD, which for four-wave workgroups equals the
// workgroups per CU)
__global__ __launch_bounds__(C::NTHREADS, C::WPE * C::WM) void conv3d_s2_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ res, float* __restrict__ y, int Ci,
                                                           int D, int H, int W, int Do, int Ho, int Wo, int ntx, int nty,
                                                           int ntz, int relu) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  int t = xcd_remap(blockIdx.x, gridDim.x);
  const int tx = t % ntx;
  t /= ntx;
  const int ty = t % nty;
  t /= nty;
  const int tz = t % ntz;
  const int b = t / ntz;
  const int x0 = tx * C::TX, y0 = ty * C::TY, z0 = tz * C::TZ;  // output coordinates
  const int dbg = DMB_DBG(relu >> 8);   // development build only (option 6): 1 = no stores, 2 = no staging after the first chunk
  relu &= 0xff;

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j = lane & 31, h = lane >> 5;
  const int wm = wave / 4, w4 = wave % 4;      // wave group along the positions; (z, channel tile) inside the group
  const int wz = w4 / C::WN, wn = w4 % C::WN;
  const unsigned HW = (unsigned)H * W, DHW = (unsigned)D * HW;
  const float* xb = x + (size_t)b * Ci * DHW;

  f32x16 acc[C::MTW][C::NT];
#pragma unroll
  for (int mt = 0; mt < C::MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  // ---- staging (LDS-DMA): unit = (channel, input z-slice, 64-column pass) = INROWS row copies; dealt to the
  // waves in contiguous runs (see conv3d_s1_kernel).  Rows go to the y-parity plane they belong to.
  constexpr int NPASS = (C::INCOLS + 63) / 64;
  constexpr int NUNIT = C::CK * C::ZS * NPASS;
  constexpr int UPW = (NUNIT + C::NWAVES - 1) / C::NWAVES;
  constexpr int WCH = C::NK * C::NTT * 64;
  constexpr int WV4 = (WCH / 4 + C::NTHREADS - 1) / C::NTHREADS;
  static_assert(WCH % 4 == 0, "weights are staged with 16-byte copies");
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wp, (unsigned)(cdiv(Ci, C::CK) * C::CK * 27 * C::COUT) * 4u);
  // Vector path: the per-lane source offsets of a chunk's copies depend on the tile only, not on the chunk (the chunk's
  // channels are selected by the resource base), so they are computed ONCE here.  Recomputing the unit -> (z, parity, row,
  // column) decode and the bounds tests for every copy of every chunk cost about two vector instructions per MFMA.
  constexpr int S_NI = C::CK * C::IPC, S_IPW = (S_NI + C::NWAVES - 1) / C::NWAVES;
  unsigned xoff[C::V16 ? S_IPW : 1];
  if constexpr (C::V16) {
#pragma unroll
    for (int q = 0; q < S_IPW; ++q) {
      const int id = wave * S_IPW + q;
      const int cl = id / C::IPC, qi = id - cl * C::IPC;
      const int u = qi * 64 + lane;
      const int zz = u / (C::ZPL / 4), r1 = u - zz * (C::ZPL / 4), pp = r1 / (C::PYPL / 4), r2 = r1 - pp * (C::PYPL / 4);
      const int row = r2 / C::UPR, sg = r2 - row * C::UPR;
      const int ry = 2 * row + pp;
      const int gz = 2 * z0 - 1 + zz, gy = 2 * y0 - 1 + ry, gxs = 2 * x0 - 4 + sg * 4;
      const bool ok = ry < C::INROWS && gz >= 0 && gz < D && gy >= 0 && gy < H && gxs >= 0 && gxs < W;
      // (a channel past Ci lies beyond the chunk's resource: the bounds check returns zeros for it)
      xoff[q] = ok ? ((unsigned)cl * DHW + (unsigned)gz * HW + (unsigned)gy * W + (unsigned)gxs) * 4u : DMA_OOB;
    }
  }
  auto stage = [&](int c0, float* buf) {
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(xb + (size_t)c0 * DHW, (unsigned)min(C::CK, Ci - c0) * DHW * 4u);
    if constexpr (C::V16) {
      // unit = 4 consecutive floats of a staged row; the units of one channel ([z][y parity][row][64]) are linear in LDS
#pragma unroll
      for (int q = 0; q < S_IPW; ++q) {
        const int id = wave * S_IPW + q;
        if (S_NI % C::NWAVES == 0 || id < S_NI) {
          const int cl = id / C::IPC, qi = id - cl * C::IPC;
          if (qi * 64 + lane < C::UPC) dma16(xrs, xoff[q], 0u, buf + cl * C::CH_STRIDE + qi * 256);
        }
      }
    } else {
#pragma unroll
    for (int q = 0; q < UPW; ++q) {
      const int uid = wave * UPW + q, pl = uid / NPASS, pass = uid - pl * NPASS;
      if (uid >= NUNIT) continue;
      const int cl = pl / C::ZS, zz = pl - cl * C::ZS;
      const int gz = 2 * z0 - 1 + zz, col = pass * 64 + lane, gx = 2 * x0 - 1 + col;
      const bool zok = gz >= 0 && gz < D && c0 + cl < Ci;
      const unsigned xvoff = (col < C::INCOLS && gx >= 0 && gx < W) ? (unsigned)gx * 4u : DMA_OOB;
      const unsigned zoff = ((unsigned)cl * DHW + (unsigned)max(gz, 0) * HW) * 4u;
      float* dpl = buf + cl * C::CH_STRIDE + zz * C::ZPL + pass * 64;
      if (col < C::R) {
#pragma unroll
        for (int ry = 0; ry < C::INROWS; ++ry) {
          const int gy = 2 * y0 - 1 + ry;
          const bool ok = zok && gy >= 0 && gy < H;
          dma4(xrs, ok ? xvoff : DMA_OOB, ok ? zoff + (unsigned)gy * W * 4u : 0u,
               dpl + (ry & 1) * C::PYPL + (ry >> 1) * C::R);
        }
      }
    }
    }
#pragma unroll
    for (int i = 0; i < WV4; ++i) {
      const int q4 = i * C::NTHREADS + threadIdx.x;
      if (q4 < WCH / 4)
        dma16(wrs, (unsigned)q4 * 16u, (unsigned)(c0 / 2) * (27 * C::NTT * 64 * 4), buf + C::IN_FLOATS + (i * C::NTHREADS + wave * 64) * 4);
    }
  };

  const int NC = cdiv(Ci, C::CK);  // a partial last chunk reads zeros (bounds check) against zero-padded weights
  stage(0, lds);
  __syncthreads();
  for (int ci = 0; ci < NC; ++ci) {
    const float* cur = lds + (ci & 1) * C::BUF_FLOATS;
    if (ci + 1 < NC && !(dbg & 2)) stage((ci + 1) * C::CK, lds + ((ci + 1) & 1) * C::BUF_FLOATS);
    const float* abase = cur + C::IN_FLOATS + (wn * C::NT) * 64 + lane;
    const float* bbase = cur + h * C::CH_STRIDE + (2 * wz) * C::ZPL + 2 * j + C::XOFF + wm * C::MTW * 64;
    float af[2][C::NT], bf[2][C::MTW];
    auto load_frag = [&](int ks, float (&a)[C::NT], float (&bq)[C::MTW]) {
      const int cp = ks / 27, tap = ks % 27;
      const int dz = tap / 9, dy = (tap / 3) % 3, dx = tap % 3;
#pragma unroll
      for (int nt = 0; nt < C::NT; ++nt) a[nt] = abase[(ks * C::NTT + nt) * 64];
      const float* bp = bbase + 2 * cp * C::CH_STRIDE + dz * C::ZPL + (dy & 1) * C::PYPL + (dy >> 1) * C::R + dx;
#pragma unroll
      for (int mt = 0; mt < C::MTW; ++mt) bq[mt] = bp[mt * 64];
    };
    load_frag(0, af[0], bf[0]);
#pragma unroll
    for (int ks = 0; ks < C::NK; ++ks) {
      if (ks + 1 < C::NK) load_frag(ks + 1, af[(ks + 1) & 1], bf[(ks + 1) & 1]);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int mt = 0; mt < C::MTW; ++mt)
#pragma unroll
        for (int nt = 0; nt < C::NT; ++nt) acc[mt][nt] = DMB_MFMA(af[ks & 1][nt], bf[ks & 1][mt], acc[mt][nt]);
      __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
  }

  const int gz = z0 + wz;
  if (gz >= Do || (dbg & 1)) return;
  const unsigned HWo = (unsigned)Ho * Wo, DHWo = (unsigned)Do * HWo;
  float* yb = y + (size_t)b * C::COUT * DHWo;
  const float* rb = res ? res + (size_t)b * C::COUT * DHWo : nullptr;
  if constexpr (C::VEP) {
    // Each 32 x 32 accumulator tile (32 positions of one output row x 32 channels) goes through this wave's scratch (the chunk
    // buffers are free after the last barrier): lane = (channel c4 of a group of 4, position pair p2), 8 groups = 8 words of 8
    // bytes.  Scratch pitch 40: the two lane halves of the write (channel rows 4 apart) and the four channel rows of a read land
    // on disjoint bank groups.  Branch-free: lanes outside the tile / volume get an out-of-range buffer offset.
    float* my = lds + wave * (32 * C::TR_PITCH);
    const __amdgpu_buffer_rsrc_t yrs = make_rsrc(yb, (unsigned)C::COUT * DHWo * 4u);
    const __amdgpu_buffer_rsrc_t rrs = make_rsrc(rb ? rb : yb, (unsigned)C::COUT * DHWo * 4u);
    const int p2 = (lane & 15) * 2, c4 = lane >> 4;
    const float lo = relu == 1 ? 0.f : -__builtin_inff();    // ReLU after the residual add
    const float lo2 = relu == 2 ? 0.f : -__builtin_inff();   // ReLU before it (GC-Net)
    const unsigned kstep = 4u * DHWo * 4u;                   // the 8 words of a lane are 4 channels apart
#pragma unroll
    for (int nt = 0; nt < C::NT; ++nt) {
      const int co0 = (wn * C::NT + nt) * 32;
      float sc8[8], sh8[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        sc8[k] = scale ? scale[co0 + k * 4 + c4] : 1.f;
        sh8[k] = shift ? shift[co0 + k * 4 + c4] : 0.f;
      }
#pragma unroll
      for (int mt = 0; mt < C::MTW; ++mt) {
        const int m = (wm * C::MTW + mt) * 32 + p2;
        const int ly = m / C::PO, lx = m - ly * C::PO;
        const int gy = y0 + ly, gxo = x0 + lx;
        const bool ok = m < C::TY * C::PO && lx < C::TX && gy < Ho && gxo < Wo;   // (PO, TX, Wo even: a pair is in or out as a whole)
        const unsigned off = ok ? ((unsigned)(co0 + c4) * DHWo + (unsigned)gz * HWo + (unsigned)gy * Wo + (unsigned)gxo) * 4u : DMA_OOB;
        u32x2 rv[8];
        if (rb) {
#pragma unroll
          for (int k = 0; k < 8; ++k) rv[k] = __builtin_amdgcn_raw_buffer_load_b64(rrs, (int)(off + k * kstep), 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) my[cd_row(r, h) * C::TR_PITCH + j] = acc[mt][nt][r];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          float2 v = *reinterpret_cast<const float2*>(my + (k * 4 + c4) * C::TR_PITCH + p2);
          v.x = fmaxf(fmaf(v.x, sc8[k], sh8[k]), lo2);
          v.y = fmaxf(fmaf(v.y, sc8[k], sh8[k]), lo2);
          if (rb) {
            v.x += __uint_as_float(rv[k].x);
            v.y += __uint_as_float(rv[k].y);
          }
          u32x2 o;
          o.x = __float_as_uint(fmaxf(v.x, lo));
          o.y = __float_as_uint(fmaxf(v.y, lo));
          __builtin_amdgcn_raw_buffer_store_b64(o, yrs, (int)(off + k * kstep), 0, 0);
        }
      }
    }
    return;
  }
#pragma unroll
  for (int nt = 0; nt < C::NT; ++nt) {
    const int co0 = (wn * C::NT + nt) * 32;
    float sc[16], sh[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + cd_row(r, h);
      sc[r] = scale ? scale[co] : 1.f;
      sh[r] = shift ? shift[co] : 0.f;
    }
#pragma unroll
    for (int mt = 0; mt < C::MTW; ++mt) {
      const int m = (wm * C::MTW + mt) * 32 + j;
      const int ly = m / C::PO, lx = m - ly * C::PO;
      const int gy = y0 + ly, gxo = x0 + lx;
      if (m < C::TY * C::PO && lx < C::TX && gy < Ho && gxo < Wo) {
        const f32x16 a1[1] = {acc[mt][nt]};
        store_tile<1>(a1, sc, sh, rb, yb, co0, h, DHWo, (unsigned)gz * HWo + (unsigned)gy * Wo + gxo, relu);
      }
    }
  }
}

template <class C>
static int launch_s2(const float* x, const float* wp, const float* scale, const float* shift, const float* res,
                     float* y, int B, int Ci, int D, int H, int W, int relu, hipStream_t st) {
  const int Do = (D - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
  const int ntx = cdiv(Wo, C::TX), nty = cdiv(Ho, C::TY), ntz = cdiv(Do, C::TZ);
  const long long nblk = (long long)B * ntx * nty * ntz;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d: grid too large");
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  DMB_ENSURE_LDS((&conv3d_s2_kernel<C>), (size_t)(lds));
  hipLaunchKernelGGL((conv3d_s2_kernel<C>), dim3((unsigned)nblk), dim3(C::NTHREADS), lds, st, x, wp, scale, shift, res, y, Ci, D,
                     H, W, Do, Ho, Wo, ntx, nty, ntz, relu);
  return launch_status("conv3d stride-2 launch failed");
}

// The 32 -> 64 / 64 -> 64 tiles of the vector path (16-byte staging, eight-wave workgroups, 8-byte epilogue): 30 columns x 4, 2 or
// 1 rows; + the 22-column four-wave tile
using S2Rows4 = S2Cfg<0, 64, 4, 30, 2, 2, true, 2, true>;
using S2Rows2 = S2Cfg<0, 64, 2, 30, 2, 2, true, 2, true>;
using S2Rows1 = S2Cfg<0, 64, 1, 30, 2, 2, true, 1, true>;
using S2Narrow = S2Cfg<0, 64, 4, 22, 2, 2, true>;

// f(C{}) for the instantiation a stride-2 plan index names (conv3d_mfma.h: S2_ROWS1 ...)
template <class F>
static auto s2_form(int k, F&& f) {
  if (k == S2_ROWS1) return f(S2Rows1{});
  if (k == S2_ROWS2) return f(S2Rows2{});
  if (k == S2_ROWS4) return f(S2Rows4{});
  if (k == S2_NARROW) return f(S2Narrow{});
  if (k == S2_ROWS4_DWORD) return f(S2Cfg<0, 64, 4, 30, 2, 2, true, 2>{});
  if (k == S2_FLAT64) return f(S2Cfg<0, 64, 4, 30, 2, 2>{});
  if (k == S2_FLAT32) return f(S2Cfg<0, 32, 4, 30, 2, 1>{});
  return f(S2Cfg<0, 128, 4, 30, 2, 4>{});
}

static int s2_pick(const ConvDesc& d) {
  const int B = d.B, Co = d.Co, D = d.D, H = d.H, W = d.W;
  const bool v16 = W % 4 == 0 && d.x_align >= 16;   // 16-byte aligned input rows
  if (Co == 64 && v16) {
    // output positions computed per tile row: 32 with 30-column tiles, 24 with 22-column ones; the narrower tile wins at
    // the training-crop widths (Wo = 64: 3 x 96 against 3 x 128 positions per 4 rows, Wo = 32: 2 x 96 against 2 x 128)
    const int Wo = (W - 1) / 2 + 1, Ho = (H - 1) / 2 + 1, Do = (D - 1) / 2 + 1;
    // 8-byte epilogue: W % 4 == 0 makes Wo even; the output (and skip operand) base must be 8-byte aligned and one batch item
    // of the output addressable with 32-bit byte offsets
    const bool pair_ok = d.y_align >= 8 && d.res_align >= 8 && (long long)Co * Do * Ho * Wo * 4 < 0x7fffffffLL;
    const bool narrow = cdiv(Wo, 22) * 96 < cdiv(Wo, 30) * 128;
    // (round 5) Tile height by estimate.  What a CU holds is ceil(workgroups / CUs) workgroups, and one SIMD runs a workgroup's
    // column tiles one after the other -- 4 with the 4 x 30 eight-wave tiles, 3 with 4 x 22, 2 with two-row tiles, 1 with one-row
    // tiles -- so finer tiles shorten the chain of a launch that leaves CUs idle (batch 1, small images: 112 -> 59 us at
    // [1, 64, 24, 68, 120]) and even out a grid that does not divide over the chip (432 four-row workgroups on 256 CUs: the
    // 64 -> 64 layer at batch 4, 201 -> 188 us on 1632 one-row ones), at the price of more halo rows per output: efficiencies
    // fitted to profiles/r05_s2_tile_probe.log and r05_kbench_small.log (same results bit for bit whatever the tile).
    const long long nz = (long long)B * cdiv(Do, 2);
    const int ncu = d.ncu;
    const double c_old = (double)cdiv_ll(nz * (narrow ? cdiv(Wo, 22) : cdiv(Wo, 30)) * cdiv(Ho, 4), ncu) * (narrow ? 3.0 / 0.85 : 4.0);
    const double c_two = (double)cdiv_ll(nz * cdiv(Wo, 30) * cdiv(Ho, 2), ncu) * 2.0 / 0.97;
    const double c_one = (double)cdiv_ll(nz * cdiv(Wo, 30) * Ho, ncu) * 1.0 / 0.94;
    int rows = 4;   // of the 30-column tile
    if (pair_ok) rows = (c_one < c_two && c_one < c_old) ? 1 : (c_two < c_old ? 2 : 4);
    const int four = narrow ? S2_NARROW : (pair_ok ? S2_ROWS4 : S2_ROWS4_DWORD);
    int k = rows == 1 ? S2_ROWS1 : (rows == 2 ? S2_ROWS2 : four);
    // ---- development switches (the release build has none): the one place where they act on a stride-2 plan
    const int tile = DMB_OPT(10);   // 10: 2 = four-row tiles with the dword epilogue, 3 / 4 = one- / two-row tiles, whatever the estimate says
    if (tile == 2) k = narrow ? S2_NARROW : S2_ROWS4_DWORD;
    if (tile == 3 && pair_ok) k = S2_ROWS1;
    if (tile == 4 && pair_ok) k = S2_ROWS2;
    if (DMB_OPT(3)) k = S2_FLAT64;   // 3: dword staging
    return k;
  }
  return Co == 64 ? S2_FLAT64 : (Co == 32 ? S2_FLAT32 : (Co == 128 ? S2_FLAT128 : -1));
}

int conv3d_s2_plan(const ConvDesc& d, const char** why) {
  const int k = s2_pick(d);
  if (k < 0) return *why = CONV3D_UNSUPPORTED, -DMB_EUNSUPPORTED;
  const int Do = (d.D - 1) / 2 + 1, Ho = (d.H - 1) / 2 + 1, Wo = (d.W - 1) / 2 + 1;
  const long long nblk = s2_form(k, [&](auto c) {
    using C = decltype(c);
    return (long long)d.B * cdiv(Wo, C::TX) * cdiv(Ho, C::TY) * cdiv(Do, C::TZ);
  });
  if (nblk > 0x7fffffffLL) return *why = "conv3d: grid too large", -DMB_EUNSUPPORTED;
  return (CONV_S2 << 8) | k;
}

int conv3d_s2_run(int plan, const float* x, const float* wpack, const float* scale, const float* shift, const float* residual, float* y,
                  int B, int Ci, int D, int H, int W, int relu, hipStream_t st) {
  return s2_form(plan & 0xff, [&](auto c) { return launch_s2<decltype(c)>(x, wpack, scale, shift, residual, y, B, Ci, D, H, W, relu, st); });
}

}  // namespace dmb

using namespace dmb;

// Raw stride-1 convolution Ci -> 32 + the batch statistics' partial sums (training path).  Applies to the vector path only.
static bool s1_stats_shape(int Ci, int Co, int D, int H, int W) {   // (positive extents)
  return Co == 32 && Ci > 0 && W % 4 == 0 && (long long)Co * D * H * W * 4 < 0x7fffffffLL && (long long)8 * D * H * W * 4 < 0x7fffffffLL;
}
static bool s1_stats_applicable(const float* x, const float* y, int B, int Ci, int Co, int D, int H, int W) {
  return s1_stats_shape(Ci, Co, D, H, W) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && DMB_OPT(2) == 0;
}
extern "C" long long dmb_conv3d_k3_bnstats_partials(int B, int Ci, int Co, int D, int H, int W) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || !s1_stats_shape(Ci, Co, D, H, W)) return 0;
  return s1_blocks32(s1_pick32(B, D, H, W, num_cus()), B, D, H, W);
}
extern "C" int dmb_conv3d_k3_bnstats_f32(const float* x, const float* wpack, float* y, double* stats, int B, int Ci, int Co, int D, int H,
                                         int W, void* stream) {
  if (!x || !wpack || !y || !stats || B <= 0 || Ci <= 0 || D <= 0 || H <= 0 || W <= 0) return fail(DMB_EINVAL, "conv3d_bnstats: bad argument");
  if (!s1_stats_applicable(x, y, B, Ci, Co, D, H, W)) return fail(DMB_EUNSUPPORTED, "conv3d_bnstats: 32 output channels, 16-byte rows");
  hipStream_t st = (hipStream_t)stream;
  return s1_visit32(s1_pick32(B, D, H, W, num_cus()), [&](auto c) { return launch_s1_stats<decltype(c)>(x, wpack, y, stats, B, Ci, D, H, W, st); });
}

// ---- 32 -> 32 classifier convolution + its 32 -> 1 head in one launch (+ the finishing pass) -----------------------------------
// The kernel runs on any volume of 16-byte rows (partial tiles are zero-filled and masked like the plain kernel's);
// dmb_conv3d_k3_head_preferred tells whether dmb_conv3d_k3_f32 would take the same 48 x 4 row-pair tile for the 32 -> 32 layer alone.
static bool s1_head_runs(int B, int D, int H, int W) {
  if (B <= 0 || D <= 0 || H <= 0 || W <= 0 || W % 4 != 0 || DMB_OPT(2) != 0) return false;
  return (long long)32 * D * H * W * 4 < 0x7fffffffLL;
}
extern "C" long long dmb_conv3d_k3_head_workspace_floats(int B, int D, int H, int W) {
  if (!s1_head_runs(B, D, H, W)) return 0;
  return s1_blocks32(S1_HEAD_PICK, B, D, H, W) * S1HeadCfg::OUT_FLOATS;
}
extern "C" int dmb_conv3d_k3_head_preferred(int B, int D, int H, int W) {
  return s1_head_runs(B, D, H, W) && s1_pick32(B, D, H, W, num_cus()) == S1_HEAD_PICK;
}
extern "C" int dmb_conv3d_head_pack_weights_f32(const float* w, float* wpack, void* stream) {
  if (!w || !wpack) return fail(DMB_EINVAL, "conv3d_head_pack_weights: bad argument");
  hipLaunchKernelGGL(pack_head_weights_kernel, dim3(HEAD_PACKED_FLOATS / 256), dim3(256), 0, (hipStream_t)stream, w, wpack);
  return launch_status("conv3d_head_pack_weights launch failed");
}
// first half: the convolution launch; slot `tile` of the workspace takes that workgroup's 6 x 6 x 50 partial sums
extern "C" int dmb_conv3d_k3_head_partial_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                              const float* head_wpack, float* workspace, int B, int Ci, int D, int H, int W, int relu,
                                              void* stream) {
  using C = S1HeadCfg;
  if (!x || !wpack || !head_wpack || !workspace || B <= 0 || Ci <= 0 || D <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "conv3d_head: bad argument");
  if (relu & DMB_CONV_SINGLE_CHAIN) return fail(DMB_EUNSUPPORTED, "conv3d_head: not a single-chain sum (use dmb_conv3d_k3_f32 + dmb_conv3d_k3_c1_f32)");
  relu &= 0xff;
  if (!s1_head_runs(B, D, H, W) || (((uintptr_t)x) & 15) != 0 || (((uintptr_t)workspace) & 7) != 0)
    return fail(DMB_EUNSUPPORTED, "conv3d_head: 16-byte rows only (W % 4 == 0, x 16-byte aligned, 32 channels of one batch item below 2 GiB), workspace 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int ntx = cdiv(W, C::TX), nty = cdiv(H, C::TY), ntz = cdiv(D, C::TZ);
  const long long nblk = (long long)B * ntx * nty * ntz;
  if (nblk > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d_head: grid too large");
  const size_t lds = (size_t)C::LDS_FLOATS * sizeof(float);
  DMB_ENSURE_LDS((&conv3d_s1_kernel<C, false>), (size_t)(lds));
  hipLaunchKernelGGL((conv3d_s1_kernel<C, false>), dim3((unsigned)nblk), dim3(256), lds, st, x, wpack, scale, shift, head_wpack,
                     workspace, Ci, D, H, W, ntx, nty, ntz, relu, (double*)nullptr);
  return launch_status("conv3d_head launch failed");
}

// second half: one finishing pass over the workspaces of a chain of heads (conv3d_head_chain_finish_kernel)
template <int N>
static void launch_head_chain(const HeadChain& ch, const float* res, bool vec, int D, int H, int W, int ntx, int nty, int ntz,
                              long long groups, hipStream_t st) {
  const dim3 grid((unsigned)cdiv_ll(groups, 256));
  if (vec)
    hipLaunchKernelGGL((conv3d_head_chain_finish_kernel<N, true>), grid, dim3(256), 0, st, ch, res, D, H, W, ntx, nty, ntz, groups);
  else
    hipLaunchKernelGGL((conv3d_head_chain_finish_kernel<N, false>), grid, dim3(256), 0, st, ch, res, D, H, W, ntx, nty, ntz, groups);
}
extern "C" int dmb_conv3d_head_chain_finish_f32(int nlevels, const float* const* workspaces, const float* bias_host,
                                                const float* residual, float* const* y, int B, int D, int H, int W, void* stream) {
  using C = S1HeadCfg;
  if (nlevels < 1 || nlevels > 4 || !workspaces || !bias_host || !y || B <= 0 || D <= 0 || H <= 0 || W <= 0)
    return fail(DMB_EINVAL, "conv3d_head_chain_finish: bad argument (1 .. 4 levels)");
  if (!s1_head_runs(B, D, H, W)) return fail(DMB_EUNSUPPORTED, "conv3d_head_chain_finish: 16-byte rows only (W % 4 == 0, 32 channels of one batch item below 2 GiB)");
  HeadChain ch{};
  bool vec = (((uintptr_t)residual) & 15) == 0;
  for (int k = 0; k < nlevels; ++k) {
    if (!workspaces[k] || !y[k]) return fail(DMB_EINVAL, "conv3d_head_chain_finish: NULL workspace or output");
    ch.ws[k] = workspaces[k], ch.y[k] = y[k], ch.bias[k] = bias_host[k];
    vec = vec && (((uintptr_t)y[k]) & 15) == 0;
  }
  const int ntx = cdiv(W, C::TX), nty = cdiv(H, C::TY), ntz = cdiv(D, C::TZ);
  const long long groups = (long long)B * D * H * (W / 4);
  if (cdiv_ll(groups, 256) > 0x7fffffffLL) return fail(DMB_EUNSUPPORTED, "conv3d_head_chain_finish: grid too large");
  hipStream_t st = (hipStream_t)stream;
  switch (nlevels) {
    case 1: launch_head_chain<1>(ch, residual, vec, D, H, W, ntx, nty, ntz, groups, st); break;
    case 2: launch_head_chain<2>(ch, residual, vec, D, H, W, ntx, nty, ntz, groups, st); break;
    case 3: launch_head_chain<3>(ch, residual, vec, D, H, W, ntx, nty, ntz, groups, st); break;
    default: launch_head_chain<4>(ch, residual, vec, D, H, W, ntx, nty, ntz, groups, st); break;
  }
  return launch_status("conv3d_head finishing launch failed");
}

extern "C" int dmb_conv3d_k3_head_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                      const float* head_wpack, float bias, const float* residual, float* y, float* workspace,
                                      int B, int Ci, int D, int H, int W, int relu, void* stream) {
  if (!y) return fail(DMB_EINVAL, "conv3d_head: bad argument");
  const int rc = dmb_conv3d_k3_head_partial_f32(x, wpack, scale, shift, head_wpack, workspace, B, Ci, D, H, W, relu, stream);
  if (rc != DMB_OK) return rc;
  const float* ws = workspace;
  return dmb_conv3d_head_chain_finish_f32(1, &ws, &bias, residual, &y, B, D, H, W, stream);
}
