// 3-D convolution family of the cost aggregators as FP32 implicit GEMMs on the gfx950 matrix cores.
//
//   y[co, p] = sum_{ci, tap} w[co, ci, tap] * x[ci, p + tap]        (M = Cout, N = voxels, K = Cin * 27)
//
// v_mfma_f32_32x32x2_f32 is exact FP32 (bitwise an fmaf chain in k order) and runs at the FP32 vector peak
// (157.3 TFLOP/s), reached from one wave per SIMD -- which a VALU kernel cannot do.  Roles: A = weights
// (row = output channel), B = input voxels (column = voxel), so that every accumulator register holds one
// output channel x 32 consecutive voxels along W and the epilogue stores 128-byte runs into NCDHW.
//
// Data flow per workgroup (256 threads = 4 waves, 2 workgroups per CU so one stages while the other
// computes):  for each chunk of CK input channels: stage the haloed input tile [CK][TZ+2][TY+2][TX+2]
// into LDS (zero padding materialised there) -> every wave runs (CK/2)*27 k-steps; per k-step one
// coalesced 256-B weight-fragment load (L2-resident, prepacked) and MT ds_read_b32 B-fragments feed
// MT*NT MFMAs.  The "voxel" index of a B fragment walks the FLATTENED padded (y, x) plane of the LDS tile,
// so a tap (dz, dy, dx) is a compile-time address offset and 32 lanes always read 32 consecutive floats
// (conflict-free); the 2 halo columns per row are computed and discarded (2/(TX+2) waste).
//
// Reference semantics: dmb/modeling/stereo/layers/basic_layers.py:68-100,160-177 (Conv3d/ConvTranspose3d
// + BatchNorm3d + ReLU factories), cost_processors/utils/hourglass.py:62-86.
//
// One translation unit per kernel family: conv3d_s1s2.hip (stride 1, + BatchNorm statistics, + the fused classifier head; stride 2),
// deconv3d.hip (transposed), conv3d_c1.hip (one output channel, VALU); split-K and the later forms: conv3d_sk.hip,
// deconv3d_zy.hip, conv3d_hw.hip.  Here: the weight packers they share and dmb_conv3d_k3_f32, which chooses among them.
#include "conv3d_mfma.h"

namespace dmb {

// ---------------------------------------------------------------------------------------------------------
// Weight prepack: A fragments in k-step order.
//   wp[((kp * 27 + tap) * NTT + nt) * 64 + lane] = W(co = nt*32 + (lane & 31), ci = 2*kp + (lane >> 5), tap)
// For nn.Conv3d W(co, ci, tap) = w[co][ci][tap]; for nn.ConvTranspose3d W(co, ci, tap) = w[ci][co][tap]; for the data
// gradient of a stride-1 nn.Conv3d W(co, ci, tap) = w[ci][co][26 - tap].
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_one(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int Cipad, int mode) {
  const int NTT = cdiv(Co, 32);   // output channels beyond Co are zero rows (1-channel transposed head of GC-Net)
  const long long total = (long long)Cipad * 27 * NTT * 32;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const int lane = (int)(i & 63);
    long long r = i >> 6;
    const int nt = (int)(r % NTT);
    r /= NTT;
    const int tap = (int)(r % 27);
    const int kp = (int)(r / 27);
    const int co = nt * 32 + (lane & 31);
    const int ci = 2 * kp + (lane >> 5);
    float v = 0.f;  // channels >= Ci are zero padding (the kernels consume Ci rounded up to their chunk size)
    // mode 2: data gradient of a stride-1 convolution = the same convolution with the channel roles exchanged and the taps
    // mirrored; mode 1: transposed convolution
    if (ci < Ci && co < Co)
      v = mode == 2 ? w[((size_t)ci * Co + co) * 27 + 26 - tap]
                    : (mode ? w[((size_t)ci * Co + co) * 27 + tap] : w[((size_t)co * Ci + ci) * 27 + tap]);
    wp[i] = v;
  }
}
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int Co, int Ci, int Cipad,
                                    int transposed) {
  pack_one(w, wp, Co, Ci, Cipad, transposed);
}

// Many weight tensors in ONE launch (a training step re-packs every unit's forward and data-gradient weights after each optimizer
// update: 52 launches of 4.8 us in a PSMNet step): blockIdx.y = job, the table lives in device memory (dmb_pack_job, dmb_hip.h).
struct PackJob {
  const float* w;
  float* wp;
  int Co, Ci, mode, pad;
};
__global__ void pack_weights_multi_kernel(const PackJob* __restrict__ jobs) {
  const PackJob jb = jobs[blockIdx.y];
  pack_one(jb.w, jb.wp, jb.Co, jb.Ci, (jb.Ci + 7) / 8 * 8, jb.mode);
}

}  // namespace dmb

using namespace dmb;

static int ci_padded(int Ci) { return (Ci + 7) / 8 * 8; }  // covers every kernel's channel-chunk size
static int co_padded(int Co) { return cdiv(Co, 32) * 32; }
extern "C" long long dmb_conv3d_packed_floats(int Co, int Ci) { return (long long)co_padded(Co) * ci_padded(Ci) * 27; }
extern "C" long long dmb_deconv3d_packed_floats(int Ci, int Co) { return (long long)co_padded(Co) * ci_padded(Ci) * 27; }

static int pack_common(const float* w, float* wp, int Co, int Ci, int transposed, void* stream) {
  if (!w || !wp || Co <= 0 || Ci <= 0) return fail(DMB_EINVAL, "pack_weights: bad argument");
  const long long total = (long long)co_padded(Co) * ci_padded(Ci) * 27;
  const int blocks = (int)((total + 255) / 256 < 1024 ? (total + 255) / 256 : 1024);
  hipLaunchKernelGGL(pack_weights_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, w, wp, Co, Ci, ci_padded(Ci),
                     transposed);
  return launch_status("pack_weights launch failed");
}

extern "C" int dmb_conv3d_pack_weights_f32(const float* w, float* wpack, int Co, int Ci, void* stream) {
  return pack_common(w, wpack, Co, Ci, 0, stream);
}
extern "C" int dmb_deconv3d_pack_weights_f32(const float* w, float* wpack, int Ci, int Co, void* stream) {
  return pack_common(w, wpack, Co, Ci, 1, stream);
}
extern "C" int dmb_conv3d_pack_dgrad_weights_f32(const float* w, float* wpack, int Co, int Ci, void* stream) {
  return pack_common(w, wpack, Ci, Co, 2, stream);   // a convolution Co -> Ci
}
extern "C" int dmb_conv3d_pack_weights_multi_f32(const void* jobs_device, int njobs, void* stream) {
  static_assert(sizeof(PackJob) == sizeof(dmb_pack_job), "dmb_pack_job layout");
  if (!jobs_device || njobs <= 0 || njobs > 65535) return fail(DMB_EINVAL, "pack_weights_multi: bad argument");
  hipLaunchKernelGGL(pack_weights_multi_kernel, dim3(64, njobs), dim3(256), 0, (hipStream_t)stream,
                     static_cast<const PackJob*>(jobs_device));
  return launch_status("pack_weights_multi launch failed");
}

// ---- Which launches take the split-K form (csrc/conv3d_sk.hip): 0 = none, else its variant --------------------------------
// A full-grid kernel gives one wave the whole chain of 27 Ci / 2 MFMAs of a tile, in chunks of two channels behind a barrier each:
// with fewer tile chains than SIMDs a launch costs ~1 us per chunk whatever its arithmetic (31-35 us for 64 channels).  Split-K
// puts eight waves on a tile.  Units: 32-voxel column tiles (16 x 2 row pairs) x 32-channel row tiles.
static int sk_variant(int B, int Ci, int Co, int D, int H, int W, int stride, int ncu) {
  const int Do = (D - 1) / stride + 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const long long tiles = (long long)B * Do * cdiv(Ho, 2) * cdiv(Wo, 16);
  const int ntt = Co / 32;
  // measured (profiles/r06_sk_probe.log, one MI355X): [1, 64, 4, 16, 32] 64 -> 64: stride 1 32.4 -> 12.8 us, stride 2 (from
  // [1, 64, 8, 32, 64]) 33.8 -> 14.9 us with one row tile per workgroup (128 workgroups); [1, 32, 16, 64, 128] -> 64 channels at
  // stride 2: 31.6 -> 22.0 us with 32 x 2 voxels x both row tiles (256 workgroups; 32 input channels = 2 pairs per wave keep the
  // A fragments of both row tiles in registers).  At 1500 tile chains and more the full-grid kernels win (each split-K workgroup
  // re-reads its share of the weights from L2: 0.45 of the matrix peak at best).
  if (tiles * ntt <= ncu + ncu / 2) return 1;
  if (stride == 2 && Ci == 32 && Co == 64 && tiles * ntt <= 4LL * ncu) return 3;
  return 0;
}

// The plan of a launch: every condition that decides among the family's forms, and every refusal (conv3d_mfma.h has the codes)
static int conv3d_plan(const ConvDesc& d, const char** why) {
  const int B = d.B, Ci = d.Ci, Co = d.Co, D = d.D, H = d.H, W = d.W, stride = d.stride;
  auto refuse = [&](int err, const char* msg) { return *why = msg, -err; };
  if (B <= 0 || Ci <= 0 || D <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "conv3d: bad argument");
  if ((long long)8 * D * H * W * 4 >= 0x7fffffffLL)
    return refuse(DMB_EUNSUPPORTED, "conv3d: 8 channels of one batch item must stay below 2 GiB (32-bit buffer offsets)");
  if ((stride == 1 || stride == 2) && (Co == 32 || Co == 64)) {
    // (round 6) launches that leave most of the chip idle: the K chain of a tile split over the eight waves of a workgroup
    // (csrc/conv3d_sk.hip)
    int v = d.single_chain ? 0 : sk_variant(B, Ci, Co, D, H, W, stride, d.ncu);
    // ---- development switch 23 (the release build has none): 1 = never, k >= 2 = force variant k - 1; one that the build does not
    // hold, or whose requirements the launch misses, is declined below and the launch takes its full-grid plan
    if (DMB_OPT(23) >= 1) v = DMB_OPT(23) - 1;
    if (v > 0 && conv3d_sk_applies(v, d)) return (CONV_SPLIT_K << 8) | (v + 4 * (stride - 1));
  }
  if (stride == 1) return conv3d_s1_plan(d, why);
  if (stride == 2) return conv3d_s2_plan(d, why);
  return refuse(DMB_EUNSUPPORTED, CONV3D_UNSUPPORTED);
}

extern "C" int dmb_conv3d_k3_plan(int B, int Ci, int Co, int D, int H, int W, int stride, int x_align, int y_align, int residual_align,
                                  int single_chain, int ncu) {
  const char* why = "";
  const int plan = conv3d_plan({B, Ci, Co, D, H, W, stride, x_align, y_align, residual_align, single_chain != 0, ncu > 0 ? ncu : num_cus()}, &why);
  set_last_error(why);
  return plan;
}

extern "C" int dmb_conv3d_k3_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                 const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W,
                                 int stride, int relu, void* stream) {
  if (!x || !wpack || !y) return fail(DMB_EINVAL, "conv3d: bad argument");
  const char* why = "";
  const int plan = conv3d_plan({B, Ci, Co, D, H, W, stride, align_of(x), align_of(y), align_of(residual), (relu & DMB_CONV_SINGLE_CHAIN) != 0,
                                num_cus()}, &why);
  if (plan < 0) return fail(-plan, why);
  hipStream_t st = (hipStream_t)stream;
  relu &= 0xff;
  if (plan >> 8 == CONV_SPLIT_K)
    return conv3d_sk_launch((plan & 0xff) - 4 * (stride - 1), x, wpack, scale, shift, residual, y, B, Ci, Co, D, H, W, stride, relu, st);
  relu |= (DMB_OPT(6) & 0xff) << 8;                    // (development build: diagnostics, see the kernels)
  if (plan >> 8 == CONV_S2) return conv3d_s2_run(plan, x, wpack, scale, shift, residual, y, B, Ci, D, H, W, relu, st);
  return conv3d_s1_run(plan, x, wpack, scale, shift, residual, y, B, Ci, D, H, W, relu, st);
}
