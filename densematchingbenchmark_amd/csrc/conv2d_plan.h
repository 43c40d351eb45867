// Launch plan of the 2-D convolution: WHICH kernel form and WHICH instantiation dmb_conv2d_f32 runs for a launch, as one pure host
// function of the launch's description.  No device code.
//
// The family has two kernel forms, tried in this order:
//   split-K  (conv3d_sk.hip, SKCfg with KZ = 1)  3x3 stride-1 launches that leave most of the chip idle: the waves of a workgroup
//                                                split the input channels of a 16 x 2 pixel tile
//   tiles    (conv2d.hip, C2Cfg)                 persistent workgroups walking 48-column tiles: everything else
// conv2d_plan() (conv2d.hip, next to the table of C2Cfg types it reads) holds every condition that decides between them and every
// refusal; the launch functions take the planned instantiation and cannot decline.  dmb_conv2d_plan (include/dmb_hip.h, which
// documents the codes) returns the plan as an integer, so the choice is testable without a GPU (tests/test_conv2d_plan_host.py).
#pragma once
#include "dmb_common.h"

namespace dmb {
// the form, bits 8.. of a plan code; bits 0-7: C2_SPLIT_K: (dilation 2 ? 2 : 0) + (both row tiles of a pair per workgroup ? 1 : 0),
// C2_TILES: the position in C2Tiles (conv2d.hip)
enum { C2_SPLIT_K = 1, C2_TILES = 2 };

// What dmb_conv2d_f32 decides a launch from: no pointers, no device.
struct Conv2dDesc {
  int B, Ci, Co, H, W, ksize, stride, dilation;
  int in_ctot, out_ctot, res_ctot;   // channels a batch item of the three tensors holds (no residual: Co or more, see c2_desc)
  int x_align, y_align, res_align;   // of the WINDOW pointers, bytes (a power of two; 16 or more = 16-byte aligned; no residual: 16)
  bool single_chain;                 // DMB_CONV_SINGLE_CHAIN: one fma chain per output whatever the launch's size
  int ncu;                           // compute units of the device
};

// -> the plan code (form << 8) | index, or minus the DMB_E* code of a refusal with its message in *why
int conv2d_plan(const Conv2dDesc& d, const char** why);

// csrc/conv3d_sk.hip.  conv2d_sk_applies: whether split-K `variant` (bits 0-7 of a C2_SPLIT_K code) takes the launch's shape and
// alignments (pure); conv2d_sk_launch runs a variant that applies.  x / y / res are the channel windows the caller has already
// offset; relu: after the skip add.
bool conv2d_sk_applies(int variant, const Conv2dDesc& d);
int conv2d_sk_launch(int variant, const float* x, const float* wp, const float* scale, const float* shift, const float* res, float* y,
                     int B, int Ci, int Co, int H, int W, int relu, int in_ctot, int out_ctot, int res_ctot, hipStream_t st);

}  // namespace dmb
