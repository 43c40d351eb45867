// Launch plan of the weight gradients (wgrad.hip): WHICH kernel instantiation, WHICH segment length and WHICH grid dmb_conv3d_k3_wgrad_f32,
// dmb_conv3d_k3s2_wgrad_f32 and dmb_conv2d_wgrad_f32 run for a launch, as one pure host function of the launch's description.  No
// device code.
//
// Every form is a persistent launch: workgroup slot s of a (32 x 32) channel block walks items s, s + slots, ... and leaves one
// partial result in the workspace; an item is (batch item, tile, segment of the axis the tile walks: z, or y in 2-D).  wgrad_plan()
// (wgrad.hip, next to the config types it reads the tile sizes from) holds every refusal and every choice -- tile, staging width,
// segment length, grid; the entry points describe, plan, launch the planned code and reduce, and cannot decline after planning.
// dmb_conv_wgrad_plan (include/dmb_hip.h, which documents the codes) returns the plan, so the choice is testable without a GPU
// (tests/test_wgrad_plan_host.py).
#pragma once
#include "dmb_common.h"

namespace dmb {
// the form, bits 8.. of a plan code; bits 0-7: the position in the form's list of instantiations (wgrad.hip)
enum { WGRAD_S1 = 1, WGRAD_S2 = 2, WGRAD_C1 = 3, WGRAD_2D = 4, WGRAD_HW = 5, WGRAD_K5 = 6, WGRAD_C1_2D = 7 };

// What the three entry points decide a launch from: no pointers, no device.
struct WgradDesc {
  int kind;             // DMB_WGRAD_S1 (plans WGRAD_S1, or WGRAD_C1 for one output channel), DMB_WGRAD_S2 (WGRAD_S2, or WGRAD_HW
                        // where the operands have the same depth of two planes or more), DMB_WGRAD_2D (WGRAD_2D, or WGRAD_K5 for
                        // kernel 5 on 1 .. 16 channels, or WGRAD_C1_2D for kernel 3, dilation 1, one output channel, 1 .. 16 input
                        // channels)
  int B, Co, Ci;        // channels of the operand that gives dw its rows (dc; stride 2: small) and its columns (x; stride 2: big)
  int D, H, W;          // extents of both operands; stride 2: of the small one; 2-D: D = 1
  int Db, Hb, Wb;       // stride 2: extents of the big operand
  int ksize, dilation;  // 2-D
  int align;            // of both operands together, bytes (a power of two; 16 or more = 16-byte aligned)
  int ncu;              // compute units of the device
};

// items of the launch = B * ntx * nty * nseg, walked by `slots` workgroups per channel block: grid (slots, blocks)
struct WgradPlan {
  int code;         // (form << 8) | index
  int ntx, nty;     // tiles along x and y (2-D: column strips and row classes = the dilation)
  int seg, nseg;    // planes (2-D: class rows; kernel 5 and 2-D one-channel: a tile's rows) per segment, segments (one output channel: 1, D)
  int slots, blocks;
};

// The split of `extent` planes into equal segments that minimises rounds x (segment length + prologue): a round = one item on
// every slot, `items_per_segment_count` = the launch's items with one segment.  Segments shorter than `min_len` are not tried.
struct WgSeg {
  int min_len;
  double prologue;   // what starting a segment costs, in planes: the ring is filled before the first multiply
};
constexpr WgSeg WG_SEG_S1 = {4, 0.5}, WG_SEG_S2 = {4, 1.0}, WG_SEG_2D = {8, 2.0};
// Stride (1, 2, 2): the layers are small (8 x 16 to 32 x 64 planes, 9 or 14 deep), so a segment may be a single plane, and a segment's
// start -- three big planes and one small one staged with nothing to multiply -- costs about one plane's step (fitted on the
// 128 <- 64 launch at [1, 128, 9, 8, 16]: docs/design/20-deeppruner-aggregator-backward.md)
constexpr WgSeg WG_SEG_HW = {1, 1.0};
constexpr double WG2_EFF_4x8 = 1.1;   // rate of the 4 x 8 stride-2 tile relative to 2 x 12 on shapes both tile exactly (wgrad_plan)

inline int segment_search(int extent, long long items_per_segment_count, int nslots, WgSeg s, double* cost_out = nullptr) {
  double best = 1e30;
  int seg = extent;
  for (int n = 1; n <= extent; ++n) {
    const int len = cdiv(extent, n);
    if (len < s.min_len && n > 1) break;
    const double cost = (double)cdiv_ll(items_per_segment_count * cdiv(extent, len), nslots) * (len + s.prologue);
    if (cost < best - 1e-9) {
      best = cost;
      seg = len;
    }
  }
  if (cost_out) *cost_out = best;
  return seg;
}

// workgroup slots per (32 x 32) channel block: the CUs (x workgroups per CU) are shared between the blocks of one launch.  The
// workspace-size functions and the plan read this one.
inline int wgrad_slots_per_block(int Co, int Ci, int per_cu, int ncu) {
  const int s = per_cu * ncu / (cdiv(Co, 32) * cdiv(Ci, 32));
  return s < 1 ? 1 : s;
}

// -> DMB_OK and *p, or the DMB_E* code of a refusal with its message in *why
int wgrad_plan(const WgradDesc& d, WgradPlan* p, const char** why);

}  // namespace dmb
