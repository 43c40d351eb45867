// Launch plan of the kernels at the output end of a model -- trilinear (align_corners) and learned (k8 / s4) up-sampling of the cost
// volume, the soft-argmin fused into either, and the adjoints of the up-sampling: WHICH kernel, WHICH layout and WHICH grid the entry
// points of regression.hip and the up-sampling half of path_bwd.hip run for a launch, as pure host functions of the launch's
// description.  No pointers; the one device call is num_cus(), made only where a choice depends on the compute units and the caller
// gave none (ncu <= 0).
//
// upsample_plan() and upsample_bwd_plan() hold every refusal that depends on the shape and every choice; the entry points check their
// pointers, plan, and launch what was planned.  dmb_upsample_plan / dmb_upsample_bwd_plan (include/dmb_hip.h, which documents the
// codes) return the plans, so the choices are testable without a GPU (tests/test_upsample_plan_host.py) and a GPU test can ask which
// launch reaches a form on the device it runs on (tests/test_upsample_every_planned_form_gpu.py).
#pragma once
#include <math.h>

#include "dmb_common.h"
#include "interp.h"

namespace dmb {

// Output positions that may blend input index i under align_corners with FP32 `scale` = (in - 1) / (out - 1): src = scale * o lies in
// (i - 1, i + 1), widened by one on either side for the rounding of the division, clamped to [0, out - 1].  scale <= 0 (one input or
// one output position): every output blends input 0 only.  The adjoint kernels gather over this range; the plan measures it.
__host__ __device__ inline void gather_range(int i, float scale, int out, int& lo, int& hi) {
  if (scale <= 0.f) {
    lo = 0;
    hi = i == 0 ? out - 1 : -1;
    return;
  }
  lo = (int)floorf((float)(i - 1) / scale) - 1;
  hi = (int)ceilf((float)(i + 1) / scale) + 1;
  lo = lo < 0 ? 0 : lo;
  hi = hi > out - 1 ? out - 1 : hi;
}

// ------------------------------------------------------------------------------------------------------------------ forward
// the entry point (DMB_UPSAMPLE_* of include/dmb_hip.h)
enum { UP_TRILINEAR_AC = 1, UP_TRILINEAR_AC_SOFT_ARGMIN = 2, UP_TRILINEAR_SOFT_ARGMIN = 3, UP_K8S4 = 4, UP_K8S4_SOFT_ARGMIN = 5 };
// the kernel, bits 8.. of a plan code
enum {
  UPK_ZCOL = 1,        // trilinear_zcol_kernel<false>:  index = (flat ? 8 : 0) + log2(zsplit)
  UPK_ROWS = 2,        // trilinear_kernel (Ho > 65535): index 0
  UPK_ZCOL_DISP = 3,   // trilinear_zcol_kernel<true>:   index = (flat ? 2 : 0) + (four columns per thread ? 1 : 0)
  UPK_PIXEL_DISP = 4,  // trilinear_soft_argmin_kernel:  index 0
  UPK_K8S4 = 5         // deconv_k8s4_zcol_kernel:       index = (with the regression ? 4 : 0) + threads / 64 - 1
};
constexpr int UP_ZCOL_MIN_BLOCKS = 2048;   // the unfused plane walk is split while the grid has fewer workgroups than this
constexpr int UP_ZSPLIT_MAX = 16;

struct UpsampleDesc {
  int entry;
  int B, Di, Hi, Wi, Do, Ho, Wo;   // k8 / s4: Di, Hi, Wi = the input's D, H, W; Do, Ho, Wo are not read (the output is exactly 4x)
  int ncu;                         // compute units to plan for; <= 0: the current device's, asked for only where they decide
};
struct UpsamplePlan {
  int code;                 // (kernel << 8) | index
  int nx, flat, zsplit;     // output columns per thread, flat (1) or row (0) layout, parts of the plane walk
  unsigned gx, gy, gz;      // the grid
  int threads;              // per workgroup
};

// Row form or flat form of trilinear_zcol_kernel (see the kernel): flat wherever rows are 16-byte multiples.  Measured inside
// the PSMNet step, forms alternated in one process (scripts/ab_step.py, development option 22): 544 x 960 (240 of a row block's 256
// lanes busy) 27.05 ms with the row form against 26.94 flat; 384 x 1248 (312 of 512) 26.60 against 26.24.
inline int trilinear_flat(int Ho, int Wo) {
  if ((Wo & 3) != 0 || (long long)Ho * (Wo / 4) >= 0x7fffff00LL) return 0;
  if (DMB_OPT(22)) return DMB_OPT(22) == 2;   // (development option 22: 1 = row form, 2 = flat form)
  return 1;
}

// -> DMB_OK and *p, or the DMB_E* code of a refusal with its message in *why
inline int upsample_plan(const UpsampleDesc& d, UpsamplePlan* p, const char** why) {
  const int B = d.B, Di = d.Di, Hi = d.Hi, Wi = d.Wi, Do = d.Do, Ho = d.Ho, Wo = d.Wo;
  auto refuse = [&](int err, const char* msg) { return *why = msg, err; };
  auto set = [&](int kernel, int index, int nx, int flat, int zsplit, long long gx, long long gy, long long gz, int threads) {
    *p = UpsamplePlan{(kernel << 8) | index, nx, flat, zsplit, (unsigned)gx, (unsigned)gy, (unsigned)gz, threads};
    return DMB_OK;
  };
  switch (d.entry) {
    case UP_TRILINEAR_AC: {
      if (B <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return refuse(DMB_EINVAL, "trilinear: bad argument");
      if ((long long)cdiv(cdiv(Wo, 4), 256) * Do * Ho > 0x7fffffffLL || B > 65535) return refuse(DMB_EUNSUPPORTED, "trilinear: grid too large");
      if (Ho > 65535)   // rows do not fit grid.y: one thread per four outputs of a (plane, row) pair, rows flattened into grid.x
        return set(UPK_ROWS, 0, 4, 0, 1, (long long)cdiv(cdiv(Wo, 4), 256) * Do * Ho, B, 1, 256);
      const int flat = trilinear_flat(Ho, Wo);
      const long long nxb = flat ? ((long long)Ho * (Wo / 4) + 255) / 256 : cdiv(cdiv(Wo, 4), 256);
      // split the plane walk only when the (row, column-block) grid alone cannot fill the chip
      const long long nblk0 = nxb * (flat ? 1 : Ho) * B;
      int zsplit = 1, lg = 0;
      while (nblk0 * zsplit < UP_ZCOL_MIN_BLOCKS && zsplit * 2 <= Do && zsplit < UP_ZSPLIT_MAX) zsplit *= 2, ++lg;
      return set(UPK_ZCOL, (flat ? 8 : 0) + lg, 4, flat, zsplit, nxb * zsplit, flat ? 1 : Ho, B, 256);
    }
    case UP_TRILINEAR_AC_SOFT_ARGMIN: {
      if (B <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0)
        return refuse(DMB_EINVAL, "trilinear_ac_soft_argmin: bad argument");
      if (Ho > 65535 || B > 65535) return refuse(DMB_EUNSUPPORTED, "trilinear_ac_soft_argmin: grid too large");
      if (Do > DMB_MAX_DISP_SAMPLES) return refuse(DMB_EINVAL, "disparity sample count out of range");
      const int flat = trilinear_flat(Ho, Wo);
      // (round 6) fewer than one wave per SIMD at four columns per thread: one column per thread -- four times the waves, each with a
      // quarter of the per-plane arithmetic of its serial walk over the Do planes (one 256x512 map: 20 -> 12 us); same bits
      const int ncu = d.ncu > 0 ? d.ncu : num_cus();
      if ((long long)B * Ho * cdiv(Wo, 4) < 4LL * 64 * ncu && (long long)Ho * Wo < 0x7fffff00LL) {
        const long long nxb1 = flat ? ((long long)Ho * Wo + 255) / 256 : cdiv(Wo, 256);
        return set(UPK_ZCOL_DISP, flat ? 2 : 0, 1, flat, 1, nxb1, flat ? 1 : Ho, B, 256);
      }
      const long long nxb = flat ? ((long long)Ho * (Wo / 4) + 255) / 256 : cdiv(cdiv(Wo, 4), 256);
      return set(UPK_ZCOL_DISP, (flat ? 2 : 0) + 1, 4, flat, 1, nxb, flat ? 1 : Ho, B, 256);
    }
    case UP_TRILINEAR_SOFT_ARGMIN: {
      if (B <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return refuse(DMB_EINVAL, "trilinear_soft_argmin: bad argument");
      if (Do <= 0 || Do > DMB_MAX_DISP_SAMPLES) return refuse(DMB_EINVAL, "disparity sample count out of range");
      if (Ho > 65535 || B > 65535) return refuse(DMB_EUNSUPPORTED, "trilinear_soft_argmin: grid too large");
      return set(UPK_PIXEL_DISP, 0, 1, 0, 1, cdiv(Wo, 256), Ho, B, 256);
    }
    case UP_K8S4:
    case UP_K8S4_SOFT_ARGMIN: {
      const int D = Di, H = Hi, W = Wi, with_disp = d.entry == UP_K8S4_SOFT_ARGMIN;
      if (B <= 0 || D <= 0 || H <= 0 || W <= 0) return refuse(DMB_EINVAL, "deconv_k8s4_soft_argmin: bad argument");
      if (4LL * H > 65535 || B > 65535) return refuse(DMB_EUNSUPPORTED, "deconv_k8s4_soft_argmin: grid too large");
      if (with_disp && 4LL * D > DMB_MAX_DISP_SAMPLES) return refuse(DMB_EINVAL, "disparity sample count out of range");
      // a row's W threads in cdiv(W, 256) workgroups of equal size, rounded up to whole waves (312 input columns: 2 x 192 threads
      // instead of 256 + 56 of 256)
      const int nwg = cdiv(W, 256), wgt = cdiv(cdiv(W, nwg), 64) * 64;
      return set(UPK_K8S4, (with_disp ? 4 : 0) + wgt / 64 - 1, 4, 0, 1, nwg, 4 * H, B, wgt);
    }
  }
  return refuse(DMB_EINVAL, "upsample_plan: no such entry point");
}

// ------------------------------------------------------------------------------------------------------------------ adjoints
enum { UPB_TRILINEAR_AC = 1, UPB_TRILINEAR_AC_SOFT_ARGMIN = 2, UPB_BILINEAR_AC = 3 };
// the (y, x) contraction's kernel = the plan code
enum {
  UPB_ROWS = 1,          // upsample_bwd_hw_rows_kernel<UPB_R>: groups of UPB_R low-resolution rows, row sums in LDS
  UPB_VOXEL_WINDOW = 2,  // upsample_regress_bwd_hw_kernel, every voxel's column window under UPB_KMAX: the windowed path throughout
  UPB_VOXEL_LOOP = 3,    // the same kernel, a window of UPB_KMAX columns or more somewhere: those voxels take the general loop
  UPB_WAVE = 4           // bilinear_ac_bwd_small_kernel: one wave per input element
};
constexpr int UPB_R = 8;       // low-resolution rows per workgroup of the row-group kernel
constexpr int UPB_KMAX = 16;   // column weights a thread keeps in registers (both kernels)
constexpr int UPB_LDS_MAX = 64 * 1024;

struct UpsampleBwdDesc {
  int entry;
  int B, planes;   // the trilinear entries: planes = Di
  int Hi, Wi, Do, Ho, Wo;   // Do: the trilinear entries only
  bool classify;   // tell UPB_VOXEL_WINDOW from UPB_VOXEL_LOOP (a walk over the Wi columns; the kernel decides per thread, so the
                   // launch does not ask)
};
struct UpsampleBwdPlan {
  int code;
  int nrmax, lds;        // UPB_ROWS: rows of LDS a group may fill, and their bytes; else 0
  unsigned gx, gy, gz;
  int threads;
  float sh, sw;
};

inline int upsample_bwd_plan(const UpsampleBwdDesc& d, UpsampleBwdPlan* p, const char** why) {
  const int B = d.B, planes = d.planes, Hi = d.Hi, Wi = d.Wi, Do = d.Do, Ho = d.Ho, Wo = d.Wo;
  auto refuse = [&](int err, const char* msg) { return *why = msg, err; };
  switch (d.entry) {
    case UPB_TRILINEAR_AC:
      if (B <= 0 || planes <= 0 || Hi <= 0 || Wi <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return refuse(DMB_EINVAL, "trilinear_bwd: bad argument");
      if (Ho > 65535 || (long long)planes * Hi > 65535 || B > 65535) return refuse(DMB_EUNSUPPORTED, "trilinear_bwd: grid too large");
      break;
    case UPB_TRILINEAR_AC_SOFT_ARGMIN:
      if (B <= 0 || planes <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return refuse(DMB_EINVAL, "trilinear_soft_argmin_bwd: bad argument");
      if (Ho > 65535 || (long long)planes * Hi > 65535 || B > 65535)
        return refuse(DMB_EUNSUPPORTED, "trilinear_soft_argmin_bwd: grid too large");
      if (Do <= 0 || Do > DMB_MAX_DISP_SAMPLES) return refuse(DMB_EINVAL, "disparity sample count out of range");
      break;
    case UPB_BILINEAR_AC:
      if (B <= 0 || planes <= 0 || Hi <= 0 || Wi <= 0 || Ho <= 0 || Wo <= 0) return refuse(DMB_EINVAL, "bilinear_bwd: bad argument");
      if ((long long)planes * Hi > 65535 || B > 65535 || planes > 65535) return refuse(DMB_EUNSUPPORTED, "bilinear_bwd: grid too large");
      break;
    default:
      return refuse(DMB_EINVAL, "upsample_bwd_plan: no such entry point");
  }
  const float sh = ac_scale(Hi, Ho), sw = ac_scale(Wi, Wo);
  if (d.entry == UPB_BILINEAR_AC && (long long)Hi * Wi * 64 <= (long long)Ho * Wo) {   // footprints of >= 64 output pixels
    *p = UpsampleBwdPlan{UPB_WAVE, 0, 0, (unsigned)(Hi * Wi), (unsigned)planes, (unsigned)B, 64, sh, sw};
    return DMB_OK;
  }
  // the row-group form where it applies (both scales > 0, column windows of at most UPB_KMAX outputs, the group's row sums within
  // 64 KB of LDS), else one thread per low-resolution voxel
  if (sh > 0.f && sw > 0.f && Hi >= 2 && Wi >= 2) {
    const int win = (int)ceilf(2.f / sw) + 5;                     // columns a low-resolution pixel may blend (bound of xhi - xlo + 1)
    const int nrmax = (int)ceilf((float)(UPB_R + 1) / sh) + 6;    // rows a group of UPB_R may blend (bound of ghi - glo + 1)
    const size_t lds = (size_t)nrmax * Wi * sizeof(float);
    if (win <= UPB_KMAX && lds <= (size_t)UPB_LDS_MAX && cdiv(Hi, UPB_R) <= 65535 && planes <= 65535) {
      *p = UpsampleBwdPlan{UPB_ROWS, nrmax, (int)lds, (unsigned)cdiv(Hi, UPB_R), (unsigned)planes, (unsigned)B, 256, sh, sw};
      return DMB_OK;
    }
  }
  int code = UPB_VOXEL_WINDOW;
  if (d.classify)
    for (int xl = 0; xl < Wi; ++xl) {
      int xlo, xhi;
      gather_range(xl, sw, Wo, xlo, xhi);
      if (xhi - xlo >= UPB_KMAX) {
        code = UPB_VOXEL_LOOP;
        break;
      }
    }
  *p = UpsampleBwdPlan{code, 0, 0, (unsigned)cdiv(Wi, 256), (unsigned)(planes * Hi), (unsigned)B, 256, sh, sw};
  return DMB_OK;
}

}  // namespace dmb
