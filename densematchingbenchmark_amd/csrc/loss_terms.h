// What the loss kernels share (losses.hip, deeppruner_loss.hip): the block size, the FP64 block reduction and the ONE statement of
// the smooth-L1 term.  Every reduction is FP64, per block then one finalising block: deterministic, no floating-point atomics.
#pragma once
#include "dmb_common.h"

namespace dmb {

constexpr int LOSS_BLOCK = 256;

// Sum over a 1-D block of LOSS_BLOCK threads; sm holds 4 doubles.  A fixed tree: the result does not depend on the run.
__device__ __forceinline__ double block_sum(double v, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  __syncthreads();
  if (lane == 0) sm[wave] = v;
  __syncthreads();
  return sm[0] + sm[1] + sm[2] + sm[3];
}

// F.smooth_l1_loss (beta = 1) of d = |x - gt|, in FP32.
__device__ __forceinline__ float smooth_l1_term(float d) { return d < 1.f ? 0.5f * d * d : d - 0.5f; }

}  // namespace dmb
