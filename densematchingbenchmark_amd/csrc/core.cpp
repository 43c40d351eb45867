// libdmb_hip.so bookkeeping: ABI version, the per-thread last-error string, the per-device CU count.
#include <atomic>

#include "dmb_common.h"

namespace dmb {
static thread_local const char* g_last_error = "";
void set_last_error(const char* msg) { g_last_error = msg ? msg : ""; }

// multiProcessorCount per device ordinal.  Read-mostly cache: a racing first use queries twice and stores the same value.
int num_cus() {
  static std::atomic<int> cache[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  int n = cache[dev].load(std::memory_order_relaxed);
  if (n > 0) return n;
  hipDeviceProp_t prop;
  n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  cache[dev].store(n, std::memory_order_relaxed);
  return n;
}
}  // namespace dmb

#ifdef DMB_DEV
// Development knobs of the DEVELOPMENT build only (lib/libdmb_hip_dev.so; see dmb_common.h).  All 0 by default.  They select kernel
// variants for A/B measurements inside one process (scripts/ab_step.py, scripts/kbench_hg.py):
//    1  = 1: VALU form of the group-wise correlation                    2  = 1: flattened conv3d tiles (no row pairs / groups / runs)
//    3  = 1: scalar (dword) staging / store paths                       4  transposed conv: 1 = never the work-queue form
//    5  rows per workgroup (gwc) / z segments (wgrad)                   6  diagnostic bits of the conv3d kernels (no stores, no staging)
//   10  stride 2: 2 = dword epilogue, 3 / 4 = one- / two-row tiles      13  = 1: box tiles instead of linear runs (stride-1, 64 ch)
//   16  zy item order: tiles per class run (0 = default)                18  = 1 / 2: four / two rows per wave in conv2d_plan
//   19  = k: stride-1 tile candidate k - 1 of the list in play          20  = 1: zy items from ONE counter instead of one per XCD
//   22  up-sampling: 1 = row form, 2 = flat form
//   23  split-K conv3d: 1 = never, k >= 2 = force variant k - 1          24  32 -> 1 head: 1 = never the split-channel form, 2 = always
//   25  split-K transposed conv: 1 = never, 2 = force                   26  split-K 3x3 conv2d: 1 = never, 2 = always
//   27  stride-2 weight gradient: 1 = 2 x 12 tile, 2 = 4 x 8 tile       29  zy tile: 1 = never 32 / 64 real columns, 2 / 3 = force them
// (7, 8, 9, 12, 21 and 28 belonged to decided experiments of the transposed convolution and are gone: scripts/README.md has the
// findings; csrc/deconv3d_plan.h is where 3, 4, 25 and 29 act on that family; 5 and 27 act on the weight gradients in wgrad_plan,
// csrc/wgrad.hip, and nowhere else there.)
// (0, 14, 17, 19 = 6 .. 9 and 10 = 1, 5, 6 belonged to decided experiments of the stride-1 / stride-2 convolutions and are gone, with
// the split-K variants that 23 alone could reach: scripts/README.md has the findings; 2, 13, 19 act in conv3d_s1_plan, 3 and 10 in
// s2_pick (csrc/conv3d_s1s2.hip), 23 in conv3d_plan (csrc/conv3d.hip), at one marked place each.)
namespace dmb {
int g_dev_opts[32] = {0};
}
extern "C" void dmb_dev_set_option(int key, int value) {
  if (key >= 0 && key < 32) dmb::g_dev_opts[key] = value;
}
#endif

extern "C" int dmb_abi_version(void) { return DMB_ABI_VERSION; }
extern "C" const char* dmb_last_error(void) { return dmb::g_last_error; }
