// Transposed 3x3x3 convolution (stride 2) of the cost aggregators, box-tiled persistent form: the FP32-MFMA implicit GEMM described
// at the head of conv3d.hip, one accumulator set per output parity.  dmb_deconv3d_k3s2_f32 (at the end) runs what deconv_plan
// (deconv3d_plan.h) names: the split-K form (conv3d_sk.hip), the work-queue form (deconv3d_zy.hip) or this one.
#include <type_traits>

#include "conv3d_mfma.h"
#include "deconv3d_plan.h"

#ifndef DMB_EPI_LD
#define DMB_EPI_LD 0   // buffer cache policy of the transposed kernel's epilogue: bit 1 = nt (streaming)
#endif
#ifndef DMB_EPI_ST
#define DMB_EPI_ST 0
#endif

namespace dmb {

// ---------------------------------------------------------------------------------------------------------
// Transposed convolution k3 s2 p1 op1:  y[2i - 1 + k] += x[i] * w[k]  per axis.  An output of parity 0 (even)
// sees k=1 from i=o/2; parity 1 (odd) sees k=2 from i=(o-1)/2 and k=0 from i=(o+1)/2.  One workgroup =
// (input-resolution tile, z parity, y parity); both x parities are accumulated by the same wave so that a
// lane owns two adjacent outputs and stores them as one 8-byte word.  No zero-insertion, no wasted MACs.
// ---------------------------------------------------------------------------------------------------------
// V16: rows are 16-byte aligned (W % 4 == 0, aligned base): the tile is staged with 16-byte LDS-DMA words (row pitch
// rounded up to 64 floats).  A CU retires LDS-DMA at about one LANE per clock whatever the word size, and with dword
// copies this kernel spent more TA cycles on staging than matrix-core cycles on arithmetic.
// VEPI (with V16): the 16-byte epilogue through the LDS scratch; a separate instantiation, not a run-time switch -- with both
// epilogues in one kernel the register allocation of the one not taken spilled into the other (the scalar form ran 1.6x
// slower once the vector form was added next to it).
template <int CIN_, int COUT_, int TY_, int TX_, int CK_, int WN_, bool V16_ = false, bool VEPI_ = false>
struct DCfg {
  static constexpr int CIN = CIN_, COUT = COUT_, TY = TY_, TX = TX_, CK = CK_, WN = WN_;
  static constexpr bool V16 = V16_, VEPI = V16_ && VEPI_;
  static constexpr int WZ = 4 / WN;
  static constexpr int TZ = WZ;
  static constexpr int P = V16 ? (TX + 1 + 3) / 4 * 4 : TX + 1;
  static constexpr int ROWS = TY + 1;
  static constexpr int PLANE = ROWS * P;
  static constexpr int ZS = TZ + 1;
  static constexpr int MT = (TY * P + 31) / 32;
  static constexpr int NTT = COUT / 32;
  static constexpr int NT = NTT / WN;
  static constexpr int CH_STRIDE = ZS * PLANE + (V16 ? 4 : 36);   // = 4 (mod 32): the two lane halves hit disjoint banks
  static constexpr int IN_FLOATS = CK * CH_STRIDE;
  static constexpr int UPR = P / 4, UPC = ZS * ROWS * UPR;    // vector path: 16-byte units per row / per channel
  static constexpr int IPC = (UPC + 63) / 64;                 // copy instructions per channel
  static constexpr int RUN = 9 * NTT * 64;                    // weight floats of one (channel pair, kz)
  static constexpr int W_FLOATS = (CK / 2) * 2 * RUN;         // worst case: two kz taps (odd output z)
  static constexpr int BUF_FLOATS = IN_FLOATS + W_FLOATS;
  static constexpr int LDS_FLOATS = 2 * BUF_FLOATS;           // double buffered
  static constexpr int AFF_FLOATS = 2 * COUT;                 // scale / shift table behind the chunk buffers
  // Vector epilogue (V16): PCH channels x 64 output columns of one output row go through a per-wave LDS scratch so that
  // a lane stores 4 consecutive x.  The scratch is the part of the just-consumed chunk buffer that only this wave's own
  // copies write (its CK/4 channels), or a dedicated region behind the affine table where that part is too small.
  static constexpr int SCR_PITCH = 68;
  static constexpr int PRIV_FLOATS = (CK / 4) * CH_STRIDE;
  static constexpr int PCH = PRIV_FLOATS >= 16 * SCR_PITCH ? 16 : 8;
  static constexpr bool SCR_PRIVATE = PRIV_FLOATS >= PCH * SCR_PITCH;
  static constexpr int SCR_FLOATS = (VEPI && !SCR_PRIVATE) ? 4 * PCH * SCR_PITCH : 0;
  static constexpr int WPE = ((LDS_FLOATS + AFF_FLOATS + SCR_FLOATS) * 4 * 2 <= 160 * 1024 && MT * NT <= 2) ? 2 : 1;  // workgroups per CU
  static_assert(P <= 64, "one wave stages one tile row per instruction");
  static_assert(CK % 2 == 0 && COUT % (32 * WN) == 0 && IN_FLOATS % 4 == 0 && (!V16 || (CH_STRIDE % 4 == 0 && TX % 4 == 0)), "shape");
  static_assert((LDS_FLOATS + AFF_FLOATS + SCR_FLOATS) * 4 <= 160 * 1024, "LDS budget");
  static_assert(!V16 || P == 32 || P == 64, "a 32-position tile of the vector epilogue is part of one input row");
};

// Body for one z parity PZ.  A work item = (input-resolution tile, z parity): the outputs of z parity PZ for BOTH y
// parities and BOTH x parities (4 accumulator sets), so the staged input tile is used by every tap that can touch it:
// per (channel pair, kz) unit 9*MT*NT MFMAs against 4*MT B reads and 9*NT A reads.
// The kernel is PERSISTENT: a workgroup walks tiles first, first + stride, ... and the chunk pipeline runs across
// tiles (the first chunk of the next tile is copied while the last chunk of this one is multiplied).  A work item
// here lasts only 40-75 k cycles, so a per-item prologue (DMA latency with idle matrix cores) and a workgroup
// re-dispatch per item would cost 15-25 %.
template <class C, int PZ>
__device__ __forceinline__ void deconv_body(float* lds, const float* __restrict__ x, const float* __restrict__ wp,
                                            const float* __restrict__ scale, const float* __restrict__ shift,
                                            const float* __restrict__ res, float* __restrict__ y, int Ci, int D, int H,
                                            int W, int ntx, int nty, int ntz, int first, int stride, int ntiles,
                                            int relu, int cvalid) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int j = lane & 31, h = lane >> 5;
  const int wz = wave / C::WN, wn = wave % C::WN;
  const unsigned HW = (unsigned)H * W, DHW = (unsigned)D * HW;
  if (first >= ntiles) return;
  const int my_tiles = (ntiles - first + stride - 1) / stride;
  const int dbg = DMB_DBG(relu >> 8);   // development build only (option 6)
  relu &= 0xff;

  struct Tile {
    int b, x0, y0, z0;
  };
  auto tile_at = [&](int it) {
    int t = first + it * stride;
    Tile tl;
    tl.x0 = (t % ntx) * C::TX;
    t /= ntx;
    tl.y0 = (t % nty) * C::TY;
    t /= nty;
    tl.z0 = (t % ntz) * C::TZ;
    tl.b = t / ntz;
    return tl;
  };

  // ---- staging: whole channels per wave; weights: per channel pair the 9 (ky, kx) taps of each needed kz, laid
  // out [cp][az][ky][kx][nt][64] with az = 0 -> kz = (PZ ? 2 : 1), az = 1 -> kz = 0.
  constexpr int NAZ = 1 + PZ;
  static_assert(C::CK % 4 == 0, "each wave stages whole channels");
  constexpr int CPW = C::CK / 4;                        // channels per wave per chunk
  constexpr int WCH4 = (C::CK / 2) * NAZ * C::RUN / 4;  // 16-byte copies per chunk
  constexpr int WV4 = (WCH4 + 255) / 256;
  const __amdgpu_buffer_rsrc_t wrs = make_rsrc(wp, (unsigned)(cdiv(Ci, C::CK) * C::CK * 27 * C::COUT) * 4u);
  // Vector path: a copy's per-lane source offset depends on the tile only (the chunk's channels are selected by the
  // resource base), so the unit -> (z, row, column) decode and the bounds tests run once per tile (tile_offsets), not once
  // per copy and chunk: they cost more vector-instruction issue slots than the chunk's MFMAs left free.
  unsigned woff[WV4];   // weight copies: per-lane source offset inside a chunk's block (the chunk goes into the scalar offset)
#pragma unroll
  for (int i = 0; i < WV4; ++i) {
    const int q4 = i * 256 + (int)threadIdx.x;
    const int run = q4 / (C::RUN / 4), off = q4 - run * (C::RUN / 4);
    const int cp = run / NAZ, az = run - cp * NAZ;
    const int kz = PZ ? (az ? 0 : 2) : 1;
    woff[i] = (unsigned)(((cp * 27 + kz * 9) * C::NTT * 64) * 4 + off * 16);
  }
  constexpr int NQ = C::V16 ? CPW * C::IPC : 1;
  auto tile_offsets = [&](const Tile& tl, unsigned (&o)[NQ]) {
    if constexpr (C::V16) {
#pragma unroll
      for (int cc = 0; cc < CPW; ++cc) {
        const int cl = wave * CPW + cc;
#pragma unroll
        for (int q = 0; q < C::IPC; ++q) {
          const int u = q * 64 + lane;
          const int zz = u / (C::ROWS * C::UPR), rr = u - zz * (C::ROWS * C::UPR), yy = rr / C::UPR, sg = rr - yy * C::UPR;
          const int gz = tl.z0 + zz, gy = tl.y0 + yy, gx = tl.x0 + sg * 4;
          // (a channel past Ci lies beyond the chunk's resource: the bounds check returns zeros for it)
          o[cc * C::IPC + q] = (gz < D && gy < H && gx < W)
                                   ? ((unsigned)cl * DHW + (unsigned)gz * HW + (unsigned)gy * W + (unsigned)gx) * 4u : DMA_OOB;
        }
      }
    }
  };
  // A chunk's copies are numbered: pieces [0, NQ) = the input tile (vector path), [NQ, NQ + WV4) = the weights; stage()
  // issues pieces [lo, hi) so that the main loop can deal them out between its MFMA groups (a wave that queues a dozen
  // 1-KiB copies back to back sits in the address queue for a few thousand cycles with its matrix pipe idle).
  constexpr int NPIECE = NQ + WV4;
  auto stage = [&](const Tile& tl, const unsigned (&toff)[NQ], int c0, float* buf, int lo = 0, int hi = 1 << 20) {
    const __amdgpu_buffer_rsrc_t xrs = make_rsrc(x + ((size_t)tl.b * Ci + c0) * DHW, (unsigned)min(C::CK, Ci - c0) * DHW * 4u);
    if constexpr (C::V16) {
      // unit = 4 consecutive floats of a staged row; the units of one channel are linear in LDS
#pragma unroll
      for (int cc = 0; cc < CPW; ++cc) {
        const int cl = wave * CPW + cc;
#pragma unroll
        for (int q = 0; q < C::IPC; ++q)
          if (cc * C::IPC + q >= lo && cc * C::IPC + q < hi && q * 64 + lane < C::UPC)
            dma16(xrs, toff[cc * C::IPC + q], 0u, buf + cl * C::CH_STRIDE + q * 256);
      }
    } else if (lo == 0) {
    const int gx = tl.x0 + lane;
    const unsigned xvoff = (lane < C::P && gx < W) ? (unsigned)gx * 4u : DMA_OOB;
    if (lane < C::P) {
#pragma unroll
      for (int cc = 0; cc < CPW; ++cc) {
        const int cl = wave * CPW + cc;
        float* dc = buf + cl * C::CH_STRIDE;
#pragma unroll
        for (int zz = 0; zz < C::ZS; ++zz) {
          const bool zok = tl.z0 + zz < D && c0 + cl < Ci;
          const unsigned zoff = ((unsigned)cl * DHW + (unsigned)(tl.z0 + zz) * HW) * 4u;
#pragma unroll
          for (int yy = 0; yy < C::ROWS; ++yy) {
            const bool ok = zok && tl.y0 + yy < H;
            dma4(xrs, ok ? xvoff : DMA_OOB, ok ? zoff + (unsigned)(tl.y0 + yy) * W * 4u : 0u,
                 dc + zz * C::PLANE + yy * C::P);
          }
        }
      }
    }
    }
#pragma unroll
    for (int i = 0; i < WV4; ++i)
      if (NQ + i >= lo && NQ + i < hi && i * 256 + (int)threadIdx.x < WCH4)
        dma16(wrs, woff[i], (unsigned)(c0 / 2) * (27 * C::NTT * 64 * 4), buf + C::IN_FLOATS + (i * 256 + wave * 64) * 4);
  };

  // Per-channel affine, staged ONCE into LDS behind the chunk buffers.  (Global loads of scale / shift inside the tile
  // loop stay "pending" in the compiler's wait-count model on the paths that do not consume them; the first reuse of
  // their registers in the next tile then drains vmcnt(0) and stalls on the chunk copy that was just put in flight.
  // LDS reads count on lgkmcnt instead and cost no registers across the loop.)
  float* aff = lds + C::LDS_FLOATS;
  if (threadIdx.x < C::COUT) {
    const bool real = (int)threadIdx.x < cvalid;   // rows >= cvalid are padding (the 1-channel head uses a 32-row tile)
    aff[threadIdx.x] = (scale && real) ? scale[threadIdx.x] : 1.f;
    aff[C::COUT + threadIdx.x] = (shift && real) ? shift[threadIdx.x] : 0.f;
  }

  const int NC = cdiv(Ci, C::CK);  // a partial last chunk reads zeros (bounds check) against zero-padded weights
  constexpr int NU = (C::CK / 2) * NAZ;  // (channel pair, az) units per chunk
  const int Ho = 2 * H, Wo = 2 * W;
  const unsigned HWo = (unsigned)Ho * Wo, DHWo = 2u * D * HWo;
  Tile cur_t = tile_at(0);
  unsigned coff[NQ], noff[NQ];
  tile_offsets(cur_t, coff);
  stage(cur_t, coff, 0, lds);
  __syncthreads();
  int g = 0;  // chunks consumed by this workgroup so far: selects the LDS buffer
  for (int it = 0; it < my_tiles; ++it) {
    const bool has_next = it + 1 < my_tiles;
    Tile next_t = cur_t;
    if (has_next) {
      next_t = tile_at(it + 1);
      tile_offsets(next_t, noff);
    }

    f32x16 acc[2][2][C::MT][C::NT];  // [py][px]
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px)
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < C::NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[py][px][mt][nt][r] = 0.f;

    for (int ci = 0; ci < NC; ++ci, ++g) {
      const float* cur = lds + (g & 1) * C::BUF_FLOATS;
      float* nxt = lds + ((g + 1) & 1) * C::BUF_FLOATS;
      // the next chunk's copies (of this tile, or the first chunk of the next one) are dealt out over the first SU units
      constexpr int SU = C::V16 ? (NU >= 6 ? NU - 2 : (NU > 1 ? NU - 1 : 1)) : 1, PPU = (NPIECE + SU - 1) / SU;
      const int smode = (dbg & 2) ? 0 : (ci + 1 < NC ? 1 : (has_next ? 2 : 0));
      auto deal = [&](int u) {
        if (smode == 1)
          stage(cur_t, coff, (ci + 1) * C::CK, nxt, u * PPU, (u + 1) * PPU);
        else if (smode == 2)
          stage(next_t, noff, 0, nxt, u * PPU, (u + 1) * PPU);
      };
      if (!C::V16) deal(0);
      const float* abase = cur + C::IN_FLOATS + (wn * C::NT) * 64 + lane;
      const float* bbase = cur + h * C::CH_STRIDE + wz * C::PLANE + j;
      float af[2][9][C::NT], bf[2][2][2][C::MT];  // bf[buf][ay][ox][mt]
      auto load_frag = [&](int u, float (&a)[9][C::NT], float (&bq)[2][2][C::MT]) {
        const int cp = u / NAZ, az = u % NAZ;
#pragma unroll
        for (int k = 0; k < 9; ++k)
#pragma unroll
          for (int nt = 0; nt < C::NT; ++nt) a[k][nt] = abase[(u * 9 + k) * C::NTT * 64 + nt * 64];
        const float* bp = bbase + 2 * cp * C::CH_STRIDE + az * C::PLANE;
#pragma unroll
        for (int ay = 0; ay < 2; ++ay)
#pragma unroll
          for (int ox = 0; ox < 2; ++ox)
#pragma unroll
            for (int mt = 0; mt < C::MT; ++mt) bq[ay][ox][mt] = bp[ay * C::P + ox + mt * 32];
      };
      load_frag(0, af[0], bf[0]);
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        if (u + 1 < NU) load_frag(u + 1, af[(u + 1) & 1], bf[(u + 1) & 1]);
        if (C::V16 && u < SU) deal(u);
        __builtin_amdgcn_sched_barrier(0);
        const auto& a = af[u & 1];
        const auto& bq = bf[u & 1];
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < C::NT; ++nt) {
            // even y (py = 0): ky = 1 from input row ay = 0
            acc[0][0][mt][nt] = DMB_MFMA(a[3 + 1][nt], bq[0][0][mt], acc[0][0][mt][nt]);  // even x: kx = 1, ox = 0
            acc[0][1][mt][nt] = DMB_MFMA(a[3 + 2][nt], bq[0][0][mt], acc[0][1][mt][nt]);  // odd x:  kx = 2, ox = 0
            acc[0][1][mt][nt] = DMB_MFMA(a[3 + 0][nt], bq[0][1][mt], acc[0][1][mt][nt]);  //         kx = 0, ox = 1
            // odd y (py = 1): ky = 2 from ay = 0, ky = 0 from ay = 1
            acc[1][0][mt][nt] = DMB_MFMA(a[6 + 1][nt], bq[0][0][mt], acc[1][0][mt][nt]);
            acc[1][1][mt][nt] = DMB_MFMA(a[6 + 2][nt], bq[0][0][mt], acc[1][1][mt][nt]);
            acc[1][1][mt][nt] = DMB_MFMA(a[6 + 0][nt], bq[0][1][mt], acc[1][1][mt][nt]);
            acc[1][0][mt][nt] = DMB_MFMA(a[0 + 1][nt], bq[1][0][mt], acc[1][0][mt][nt]);
            acc[1][1][mt][nt] = DMB_MFMA(a[0 + 2][nt], bq[1][0][mt], acc[1][1][mt][nt]);
            acc[1][1][mt][nt] = DMB_MFMA(a[0 + 0][nt], bq[1][1][mt], acc[1][1][mt][nt]);
          }
        __builtin_amdgcn_sched_barrier(0);
      }
      __syncthreads();
    }

    // ---- epilogue of cur_t ----
    const int gzi = cur_t.z0 + wz;
    if constexpr (C::VEPI) {
      if (!(dbg & 1)) {
      // ---- vector epilogue: per (channel tile, 32-position tile, y parity) the two x-parity accumulator tiles are
      // interleaved in LDS ([PCH channels][64 output columns], 8-byte writes), read back as 4 consecutive x of one
      // channel and stored / residual-loaded as 16-byte words through buffer resources (lanes outside the volume get an
      // out-of-range offset: branch-free).  Residual loads run one pass ahead of the stores.
      // (g has been advanced past the last chunk: buffer (g & 1) is being filled for the next tile, ((g - 1) & 1) is
      // the one just consumed; every wave's reads of it completed before the barrier that ended the chunk loop)
      float* scr = C::SCR_PRIVATE ? lds + ((g - 1) & 1) * C::BUF_FLOATS + wave * C::PRIV_FLOATS
                                  : lds + C::LDS_FLOATS + C::AFF_FLOATS + wave * (C::PCH * C::SCR_PITCH);
      const unsigned gz = 2 * gzi + PZ;
      float* yb = y + (size_t)cur_t.b * C::COUT * DHWo;
      const __amdgpu_buffer_rsrc_t yrs = make_rsrc(yb, (unsigned)C::COUT * DHWo * 4u);
      const __amdgpu_buffer_rsrc_t rrs = make_rsrc(res ? res + (size_t)cur_t.b * C::COUT * DHWo : yb, (unsigned)C::COUT * DHWo * 4u);
      const int rl = lane >> 4, x4 = (lane & 15) * 4;
      const float lo = relu == 1 ? 0.f : -__builtin_inff();    // ReLU after the residual add
      const float lo2 = relu == 2 ? 0.f : -__builtin_inff();   // ReLU before it (GC-Net)
      constexpr int QP = 32 / C::PCH, KP = C::PCH / 4;        // passes per 32-channel tile, 16-byte words per lane and pass
      constexpr int NPASS = C::NT * C::MT * 2 * QP;
      auto pass_off = [&](int t, unsigned (&off)[KP], int (&ch)[KP]) {
        const int q = t % QP, py = (t / QP) % 2, mt = (t / (2 * QP)) % C::MT, nt = t / (2 * QP * C::MT);
        const int ly = (mt * 32) / C::P, lx0 = (mt * 32) % C::P;
        const int gyi = cur_t.y0 + ly, gxi = cur_t.x0 + lx0 + x4 / 2;
        const bool ok = gzi < D && gyi < H && lx0 + x4 / 2 < C::TX && gxi < W && !(dbg & 4);
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          ch[k] = (wn * C::NT + nt) * 32 + q * C::PCH + 4 * k + rl;
          off[k] = ok ? ((unsigned)ch[k] * DHWo + gz * HWo + (unsigned)(2 * gyi + py) * Wo + 2u * (unsigned)(cur_t.x0 + lx0) + (unsigned)x4) * 4u
                      : DMA_OOB;
        }
      };
      auto run = [&](auto has_res) {
        constexpr bool HAS_RES = decltype(has_res)::value;
        // A wave has no other work to hide a load behind (the accumulators take half of its registers), so the residual
        // loads run in a ring RD passes deep (16 words of 16 bytes in flight per lane): one exposed latency per item
        // instead of one per pass.
        constexpr int RD = HAS_RES ? (16 / KP < NPASS ? 16 / KP : NPASS) : 1;
        u32x4 rv[RD][KP];   // (offsets are recomputed at use: only the loaded words stay live across passes)
        if constexpr (HAS_RES) {
#pragma unroll
          for (int t = 0; t < RD; ++t) {
            unsigned o0[KP];
            int c0[KP];
            pass_off(t, o0, c0);
#pragma unroll
            for (int k = 0; k < KP; ++k) rv[t][k] = __builtin_amdgcn_raw_buffer_load_b128(rrs, (int)o0[k], 0, DMB_EPI_LD);
          }
        }
#pragma unroll
        for (int t = 0; t < NPASS; ++t) {
          const int q = t % QP, py = (t / QP) % 2, mt = (t / (2 * QP)) % C::MT, nt = t / (2 * QP * C::MT);
          const int sl = t % RD;
          unsigned off[KP];
          int ch[KP];
          pass_off(t, off, ch);
#pragma unroll
          for (int rr = 0; rr < C::PCH / 2; ++rr) {
            const int r = q * (C::PCH / 2) + rr;
            const int row = (r & 3) + 4 * h + (C::PCH == 16 ? 8 * ((r >> 2) & 1) : 0);
            *reinterpret_cast<float2*>(scr + row * C::SCR_PITCH + 2 * j) =
                make_float2(acc[py][0][mt][nt][r], acc[py][1][mt][nt][r]);
          }
#pragma unroll
          for (int k = 0; k < KP; ++k) {
            float4 v = *reinterpret_cast<const float4*>(scr + (4 * k + rl) * C::SCR_PITCH + x4);
            const float sc = aff[ch[k]], sh = aff[C::COUT + ch[k]];
            v.x = fmaxf(fmaf(v.x, sc, sh), lo2);
            v.y = fmaxf(fmaf(v.y, sc, sh), lo2);
            v.z = fmaxf(fmaf(v.z, sc, sh), lo2);
            v.w = fmaxf(fmaf(v.w, sc, sh), lo2);
            if constexpr (HAS_RES) {
              v.x += __uint_as_float(rv[sl][k].x);
              v.y += __uint_as_float(rv[sl][k].y);
              v.z += __uint_as_float(rv[sl][k].z);
              v.w += __uint_as_float(rv[sl][k].w);
            }
            u32x4 o;
            o.x = __float_as_uint(fmaxf(v.x, lo));
            o.y = __float_as_uint(fmaxf(v.y, lo));
            o.z = __float_as_uint(fmaxf(v.z, lo));
            o.w = __float_as_uint(fmaxf(v.w, lo));
            __builtin_amdgcn_raw_buffer_store_b128(o, yrs, (int)off[k], 0, DMB_EPI_ST);
          }
          if constexpr (HAS_RES) {
            if (t + RD < NPASS) {   // refill the slot just consumed
              pass_off(t + RD, off, ch);
#pragma unroll
              for (int k = 0; k < KP; ++k) rv[sl][k] = __builtin_amdgcn_raw_buffer_load_b128(rrs, (int)off[k], 0, DMB_EPI_LD);
            }
          }
        }
      };
      if (res)
        run(std::true_type{});
      else
        run(std::false_type{});
      }
    } else if (gzi < D && !(dbg & 1)) {
      const unsigned gz = 2 * gzi + PZ;
      const int cout = cvalid < C::COUT ? cvalid : C::COUT;   // channels the output tensor really has
      float* yb = y + (size_t)cur_t.b * cout * DHWo;
      const float* rb = res ? res + (size_t)cur_t.b * cout * DHWo : nullptr;
#pragma unroll
      for (int nt = 0; nt < C::NT; ++nt) {
        const int co0 = (wn * C::NT + nt) * 32;
        float sc[16], sh[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          sc[r] = aff[co0 + cd_row(r, h)];
          sh[r] = aff[C::COUT + co0 + cd_row(r, h)];
        }
#pragma unroll
        for (int mt = 0; mt < C::MT; ++mt) {
          const int m = mt * 32 + j;
          const int ly = m / C::P, lx = m - ly * C::P;
          const int gyi = cur_t.y0 + ly, gxi = cur_t.x0 + lx;
          if (m < C::TY * C::P && lx < C::TX && gyi < H && gxi < W) {
#pragma unroll
            for (int py = 0; py < 2; ++py) {
              const f32x16 a2[2] = {acc[py][0][mt][nt], acc[py][1][mt][nt]};
              store_tile<2>(a2, sc, sh, rb, yb, co0, h, DHWo, gz * HWo + (unsigned)(2 * gyi + py) * Wo + 2u * gxi, relu, cvalid);
            }
          }
        }
      }
    }
    cur_t = next_t;
#pragma unroll
    for (int q = 0; q < NQ; ++q) coff[q] = noff[q];
  }
}

// Workgroups [0, g0) take the even-z work items, the rest the odd-z ones (which carry twice the MFMAs).
template <class C>
__global__ __launch_bounds__(256, C::WPE) void deconv3d_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                               const float* __restrict__ scale,
                                                               const float* __restrict__ shift,
                                                               const float* __restrict__ res, float* __restrict__ y,
                                                               int Ci, int D, int H, int W, int ntx, int nty, int ntz,
                                                               int ntiles, int g0, int relu, int cvalid) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  if ((int)blockIdx.x < g0)
    deconv_body<C, 0>(lds, x, wp, scale, shift, res, y, Ci, D, H, W, ntx, nty, ntz, blockIdx.x, g0, ntiles, relu, cvalid);
  else
    deconv_body<C, 1>(lds, x, wp, scale, shift, res, y, Ci, D, H, W, ntx, nty, ntz, blockIdx.x - g0, gridDim.x - g0,
                      ntiles, relu, cvalid);
}

// (deconv_plan has checked that the tile count fits the grid)
template <class C>
static int launch_deconv(const DeconvArgs& a) {
  const int ntx = cdiv(a.W, C::TX), nty = cdiv(a.H, C::TY), ntz = cdiv(a.D, C::TZ);
  const long long ntiles = (long long)a.B * ntx * nty * ntz;
  const size_t lds = (size_t)(C::LDS_FLOATS + C::AFF_FLOATS + C::SCR_FLOATS) * sizeof(float);
  DMB_ENSURE_LDS((&deconv3d_kernel<C>), (size_t)(lds));
  const int ncu = num_cus();
  // persistent grid: C::WPE workgroups per CU; a third of them walk the even-z items, two thirds the odd-z items
  // (twice the work each).  With fewer items than slots every workgroup gets exactly one item.
  const long long slots = (long long)C::WPE * ncu;
  long long g0, g1;
  if (2 * ntiles <= slots) {
    g0 = g1 = ntiles;
  } else {
    // twice as many workgroups as resident slots: each walks half as many items, and the dispatcher's dynamic placement
    // evens out what a static walk cannot (measured 64 -> 32 at half resolution: 0.98 -> 0.82 ms)
    const long long total = 2 * slots;
    g0 = total / 3 > 0 ? total / 3 : 1;
    g1 = total - g0;
    if (g0 > ntiles) g0 = ntiles;
    if (g1 > ntiles) g1 = ntiles;
  }
  hipLaunchKernelGGL((deconv3d_kernel<C>), dim3((unsigned)(g0 + g1)), dim3(256), lds, a.st, a.x, a.wp, a.scale, a.shift, a.res, a.y,
                     a.Ci, a.D, a.H, a.W, ntx, nty, ntz, (int)ntiles, (int)g0, a.relu, a.Co);
  return launch_status("deconv3d launch failed");
}

// The two-parity tile of plan config K (deconv3d_plan.h: D_TILE; 32-row tiles first).  Fewer than 32 output channels (GC-Net's
// 1-channel head) run the 32-row tiles: zero-padded weight rows, masked scalar epilogue.
template <int K, int T = K % D_TILES, int CO = K < D_TILES ? 32 : 64>
using DTileCfg = DCfg<0, CO, D_TILE[T].ty, D_TILE[T].tx, 256 / CO, CO / 32, D_TILE[T].v16, D_TILE[T].vepi>;

}  // namespace dmb

using namespace dmb;

extern "C" int dmb_deconv3d_k3s2_plan(int B, int Ci, int Co, int D, int H, int W, int Wout, int x_align, int y_align, int residual_align,
                                      int workspace_align, int single_chain, int ncu) {
  const char* why = "";
  const int plan = deconv_plan({B, Ci, Co, D, H, W, Wout, x_align, y_align, residual_align, workspace_align, single_chain != 0,
                                ncu > 0 ? ncu : num_cus()}, &why);
  set_last_error(why);
  return plan;
}

extern "C" int dmb_deconv3d_k3s2_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                     const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int Wout,
                                     int relu, void* workspace, void* stream) {
  if (!x || !wpack || !y) return fail(DMB_EINVAL, "deconv3d: bad argument");
  const char* why = "";
  const int plan = deconv_plan({B, Ci, Co, D, H, W, Wout, align_of(x), align_of(y), align_of(residual), workspace ? align_of(workspace) : 0,
                                (relu & DMB_CONV_SINGLE_CHAIN) != 0, num_cus()}, &why);
  if (plan < 0) return fail(-plan, why);
  const int cfg = plan & 0xff;
  // bits 8..: the development build's diagnostic bits (option 6), passed on to the kernels
  const DeconvArgs a{x, wpack, scale, shift, residual, y, B, Ci, Co, D, H, W, Wout, (relu & 0xff) | (DMB_OPT(6) << 8), (hipStream_t)stream};
  if (plan >> 8 == DECONV_SPLIT_K) return deconv3d_sk_launch(cfg, a);
  if (plan >> 8 == DECONV_QUEUE) return deconv3d_zy_launch(cfg, a, static_cast<int*>(workspace));
  return deconv_visit(cfg, [&](auto k) { return launch_deconv<DTileCfg<decltype(k)::value>>(a); }, std::make_integer_sequence<int, 2 * D_TILES>{});
}
