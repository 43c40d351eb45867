// Launch plan of the transposed 3x3x3 convolution (k3, stride 2, padding 1, output_padding 1): WHICH kernel form and WHICH tile
// instantiation dmb_deconv3d_k3s2_f32 runs for a launch, as one pure host function of the launch's description.  No device code.
//
// The family has three kernel forms, tried in this order:
//   split-K     (conv3d_sk.hip,   DSKCfg)  launches that leave most of the chip idle: the waves of a workgroup split the input channels
//   work queue  (deconv3d_zy.hip, ZYCfg)   items (tile, z parity, y parity) drawn from counters in the caller's workspace
//   two-parity  (deconv3d.hip,    DCfg)    items (tile, z parity), static walk: whatever the other two do not take
// deconv_plan() below holds every condition that decides between them and every refusal; the launch functions (declared at the
// end) take the planned config and cannot decline.  dmb_deconv3d_k3s2_plan (include/dmb_hip.h) returns the plan as an integer, so
// the choice is testable without a GPU (tests/test_deconv3d_plan_host.py).
//
// Plan codes: (form << 8) | config, config = tile + (Co == 64 ? tiles of the form : 0).  The tile tables below are plain data: the three
// translation units instantiate their DSKCfg / ZYCfg / DCfg from them, so a config index names one instantiation here and there.
#pragma once
#include <utility>

#include "dmb_common.h"

namespace dmb {
enum { DECONV_SPLIT_K = 1, DECONV_QUEUE = 2, DECONV_PARITY = 3 };

// work-queue tiles: MT 32-column MFMA tiles per input row of an item; FULL: all 32 MT staged positions are real, else 4 fewer
enum { ZY_N28 = 0, ZY_F32 = 1, ZY_F64 = 2, ZY_W60 = 3, ZY_TILES = 4 };
constexpr struct { int mt; bool full; } ZY_TILE[ZY_TILES] = {{1, false}, {1, true}, {2, true}, {2, false}};
constexpr int zy_tx(int tile) { return 32 * ZY_TILE[tile].mt - (ZY_TILE[tile].full ? 0 : 4); }
// ZY_W60 is never planned without development option 29: a launch that is not `narrow` has c_old = cdiv(W, 60) * 64 >=
// cdiv(W, 64) * 64 = c_f64, so `full` is 2 -- or 1 where c_f32 < c_f64 <= c_old.  The release library does not build it.
#ifdef DMB_DEV
constexpr int ZY_BUILT = ZY_TILES;
#else
constexpr int ZY_BUILT = ZY_W60;
#endif
// two-parity tiles: TY x TX input positions per item; dword staging, 16-byte staging with the 8-byte scattered epilogue, 16-byte
// staging with the 16-byte epilogue
enum { D_W60_DWORD = 0, D_W60_V16 = 1, D_W60_VEPI = 2, D_N28_V16 = 3, D_N28_VEPI = 4, D_TILES = 5 };
constexpr struct { int ty, tx; bool v16, vepi; } D_TILE[D_TILES] = {{1, 60, false, false}, {1, 60, true, false}, {1, 60, true, true}, {2, 28, true, false}, {2, 28, true, true}};
// the split-K tile: four waves, 16 x 2 input positions per workgroup (eight waves, and 32 x 2 positions with either wave count, lost
// every measured shape: profiles/r06_sk_probe_deconv.log); floats per channel of the largest class, floats of a wave's partial tile
constexpr int DSK_NW = 4, DSK_XS = 1, DSK_TXI = 16 * DSK_XS, DSK_TYI = 2, DSK_IN_MAX = 2 * 3 * (DSK_TXI + 4), DSK_PART = 32 * (DSK_XS * 64 + 4);

struct DeconvDesc {
  int B, Ci, Co, D, H, W, Wout;
  int x_align, y_align, res_align;   // bytes (a power of two; 16 or more = 16-byte aligned; no residual: 16)
  int ws_align;                      // the workspace's alignment in bytes, 0 = no workspace
  bool single_chain;                 // DMB_CONV_SINGLE_CHAIN: one fma chain per output whatever the launch's size
  int ncu;                           // compute units of the device
};

// -> the plan code (form << 8) | config, or minus the DMB_E* code of a refusal with its message in *why
inline int deconv_plan(const DeconvDesc& d, const char** why) {
  const int B = d.B, Ci = d.Ci, Co = d.Co, D = d.D, H = d.H, W = d.W, Wout = d.Wout, ncu = d.ncu;
  auto refuse = [&](int err, const char* msg) { return *why = msg, -err; };
  auto plan = [](int form, int cfg) { return (form << 8) | cfg; };
  const long long LIM = 0x7fffffffLL;   // 32-bit buffer offsets

  // ---- the arguments
  if (B <= 0 || Ci <= 0 || D <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "deconv3d: bad argument");
  if (Wout <= 0 || Wout > 2 * W || Wout <= 2 * W - 8 || (Wout & 1))
    return refuse(DMB_EINVAL, "deconv3d: Wout must be 2 W, or 2 W minus the (at most 3) doubled padding columns");
  const long long vox = (long long)D * H * W;
  if (8 * vox * 4 >= LIM)
    return refuse(DMB_EUNSUPPORTED, "deconv3d: 8 input channels of one batch item must stay below 2 GiB (32-bit buffer offsets)");
  const bool aligned16 = d.x_align >= 16 && d.y_align >= 16 && d.res_align >= 16;
  const bool out_small = (long long)Co * 8 * vox * 4 < LIM;   // one batch item of the output below 2 GiB
  const bool scalar = DMB_OPT(3) != 0;                        // (development option 3: dword staging / store paths only)

  // ---- 1. split-K: launches that leave most of the chip idle.  Units: input-resolution tiles x 32-channel row tiles.
  // measured (profiles/r06_sk_probe_deconv.log, persistent form, four waves per workgroup):
  // 128 units ([1, 64, 4, 16, 32] -> 64 channels) 37.3 -> 14.2 us, 192 units 38.0 -> 16.7, 360 units 37.8 -> 26.7, 576 units 59.3 -> 40.3,
  // 1632 units 99 against 103 (a tie); 512 units ([1, 64, 8, 32, 64] -> 32 channels) 50.2 -> 36.9, 768 units 69.2 -> 52.5, 1200 units
  // 80.6 -> 76.6, 2304 units 136 against 143: from there on the work-queue kernel wins
  {
    const long long tiles = (long long)B * D * cdiv(H, DSK_TYI) * cdiv(W, DSK_TXI), ntt = cdiv(Co, 32);
    bool sk = !d.single_chain && tiles * ntt <= 5LL * ncu;
    if (DMB_OPT(25) == 1) sk = false;   // (development option 25: 1 = never, 2 = force)
    if (DMB_OPT(25) == 2) sk = true;
    // 16-byte rows everywhere, whole channel pairs per wave with their taps in registers, 32-bit offsets inside a wave's channels
    if (sk && Co <= 64 && W % 4 == 0 && Wout % 4 == 0 && aligned16 && Ci % (2 * DSK_NW) == 0 && Ci <= 64 &&
        (long long)(Ci / DSK_NW) * vox * 4 < LIM) {
      if (tiles * 4 * ntt > LIM) return refuse(DMB_EUNSUPPORTED, "deconv3d: grid too large");
      const long long in_floats = (long long)Ci * DSK_IN_MAX, part_floats = (long long)DSK_NW * DSK_PART;
      if ((in_floats > part_floats ? in_floats : part_floats) * 4 <= 160 * 1024) return plan(DECONV_SPLIT_K, 0);
    }
  }

  // 2 rows x 28 columns per item instead of 1 x 60 where that computes fewer positions (input W = 64: 3 x 32 against 2 x 64 per row;
  // 80 columns: 96 against 128).  Both forms below use it: the tile width stays a multiple of 4 for the 16-byte staging.
  const bool narrow = cdiv(W, 28) * 32 < cdiv(W, 60) * 64;

  // ---- 2. work queue: three workgroups per CU.  16-byte aligned rows, all 32 or 64 output channels real, whole 16-channel chunks
  // and at least two of them in every class, 16 input channels of one batch item and one batch item of the output below 2 GiB.
  bool queue = d.ws_align > 0 && !scalar;
  if (DMB_OPT(4) == 1) queue = false;   // (development option 4 = 1: the two-parity form)
  if (queue) {
    if (d.ws_align < 4) return refuse(DMB_EINVAL, "deconv3d: misaligned workspace");
    if ((Co == 32 || Co == 64) && Ci % 16 == 0 && Ci >= 32 && W % 4 == 0 && Wout % 4 == 0 && aligned16 && 16 * vox * 4 < LIM && out_small) {
      // (round 6) tiles of 32 / 64 REAL columns (a longer staged row) where those compute fewer columns than the 28- / 60-column
      // ones: 64 input columns 64 against 96, 32 columns 32 against 64, 156 (KITTI) 160 against 192.  Same arithmetic per output
      // whatever the tile.  A tie between 60- and 64-column tiles -- 120 input columns: 2 x 64 computed either way -- goes to the
      // 64-column form, whose tiles start on 512-byte boundaries of the output rows: 849-865 -> 829 us for conv6 at
      // [4, 64, 24, 68, 120] alone, equal within the noise inside the step (807 against 803 us under rocprofv3).
      const int c_old = narrow ? cdiv(W, 28) * 32 : cdiv(W, 60) * 64, c_f32 = cdiv(W, 32) * 32, c_f64 = cdiv(W, 64) * 64;
      int full = c_f64 <= c_old && c_f64 <= c_f32 ? 2 : (c_f32 < c_old ? 1 : 0);
      if (DMB_OPT(29) == 1) full = 0;   // (development option 29: 1 = never, 2 / 3 = force the 32- / 64-column form)
      if (DMB_OPT(29) >= 2) full = DMB_OPT(29) - 1;
      // (round 6) A 64-channel launch of about one item per workgroup slot (conv5 of one 544x960 pair: 816 items of weight 1 .. 4 on
      // 768 slots) is faster on the two-parity form's items: 0.099 -> 0.069 ms at [1, 64, 12, 34, 60]; equal at the KITTI shape and
      // from two pairs on (scripts/kbench_hg.py, KB_B = 1 / 2).  Same arithmetic, bit-identical results.
      const long long items = 4LL * B * cdiv(W, narrow ? 28 : 60) * H * cdiv(D, 2);
      if (!(Co == 64 && Wout == 2 * W && 4 * items <= 5LL * 3 * ncu)) {
        const int tile = full == 2 ? ZY_F64 : (full == 1 ? ZY_F32 : (narrow ? ZY_N28 : ZY_W60));
        const long long ntiles = (long long)B * cdiv(W, zy_tx(tile)) * H * cdiv(D, Co == 64 ? 2 : 4);
        if (4 * ntiles > 0x3fffffffLL) return refuse(DMB_EUNSUPPORTED, "deconv3d: grid too large");
        // (the ticket field of a published draw holds 27 bits; 33 M tiles: far beyond any volume here)
        if (4 * ntiles < (1LL << 27)) return plan(DECONV_QUEUE, tile + (Co == 64 ? ZY_TILES : 0));
      }
    }
  }

  // ---- 3. two-parity
  if (Wout != 2 * W)
    return refuse(DMB_EUNSUPPORTED, "deconv3d: a row-padded input (Wout < 2 W) needs the workspace form: Co 32 or 64, Ci % 16 == 0, Wout % 4 == 0, aligned operands");
  if (Co > 32 && Co != 64) return refuse(DMB_EUNSUPPORTED, "deconv3d: output channels must be <= 32 or 64");
  const bool v16 = W % 4 == 0 && d.x_align >= 16 && !scalar;   // 16-byte aligned rows
  // 16-byte epilogue: aligned output / residual rows, every channel real, one batch item of the output below 2 GiB
  const bool vepi = v16 && Co % 32 == 0 && d.y_align >= 16 && d.res_align >= 16 && out_small;
  const int tile = v16 && narrow ? (vepi ? D_N28_VEPI : D_N28_V16) : (!v16 ? D_W60_DWORD : (vepi ? D_W60_VEPI : D_W60_V16));
  // fewer than 32 channels (GC-Net's 1-channel head): the 32-row tiles with zero-padded weight rows and the masked scalar epilogue
  const long long ntiles = (long long)B * cdiv(W, D_TILE[tile].tx) * cdiv(H, D_TILE[tile].ty) * cdiv(D, Co == 64 ? 2 : 4);
  if (ntiles > 0x3fffffffLL) return refuse(DMB_EUNSUPPORTED, "deconv3d: grid too large");
  return plan(DECONV_PARITY, tile + (Co == 64 ? D_TILES : 0));
}

// f(integral_constant<k>) for a planned config index k: where a translation unit turns the index into its instantiation
template <class F, int... I>
static int deconv_visit(int k, F&& f, std::integer_sequence<int, I...>) {
  int rc = DMB_EUNSUPPORTED;
  const bool hit = ((k == I && ((rc = f(std::integral_constant<int, I>{})), true)) || ...);
  return hit ? rc : fail(DMB_EUNSUPPORTED, "deconv3d: the plan names a tile this build does not hold");
}

// What one launch passes on to the planned form.  relu: bits 0-7 the ReLU mode, bits 8.. the development build's diagnostic bits.
struct DeconvArgs {
  const float *x, *wp, *scale, *shift, *res;
  float* y;
  int B, Ci, Co, D, H, W, Wout, relu;
  hipStream_t st;
};
int deconv3d_sk_launch(int cfg, const DeconvArgs& a);              // conv3d_sk.hip
int deconv3d_zy_launch(int cfg, const DeconvArgs& a, int* ws);     // deconv3d_zy.hip; ws: zeros on entry, zeros again afterwards

}  // namespace dmb
