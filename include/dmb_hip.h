/*
 * dmb_hip.h -- C ABI of libdmb_hip.so: the MI355X (gfx950) cost-volume -> 3-D aggregation
 * -> disparity-regression path of DenseMatchingBenchmark's dmb.modeling.stereo pipeline.
 *
 * Boundary rules:
 *   - every pointer is a DEVICE pointer owned by the caller (the PyTorch-ROCm caching
 *     allocator in the Python host layer) unless the parameter name ends in `_host`;
 *   - all tensors are FP32, contiguous, NC(D)HW exactly as the reference lays them out;
 *   - `stream` is the caller's hipStream_t (NULL = the legacy default stream); every entry
 *     point only enqueues kernel launches on that stream: no synchronisation, no allocation, no
 *     memset / memcpy -- so a sequence of calls can be captured into a HIP graph and replayed
 *     (tests/test_graph_gpu.py captures a whole PSMNet step).  Scratch memory a kernel needs is a
 *     caller-provided workspace argument (dmb_*_workspace_bytes / DMB_*_WORKSPACE_BYTES), as the
 *     reference's own native op takes caller-allocated tensors only
 *     (dmb/ops/spn/functions/gaterecurrent2dnoind.py:8-39);
 *   - return value 0 = success, otherwise the hipError_t value of the failing launch or one of
 *     the DMB_E* codes below.  Nothing here calls exit() (the reference's only native op,
 *     dmb/ops/spn/src/gaterecurrent2dnoind_kernel.cu:544-549, does; this library does not);
 *   - host-side state, all of it: a thread-local pointer to the last error string, and two
 *     per-device read-mostly caches filled on first use (the device's compute-unit count; which
 *     kernels have had their dynamic-LDS limit raised on which device, a per-device attribute
 *     that hipFuncSetAttribute requires before a launch with more than 64 KB of LDS).  No
 *     option table, no device allocations, nothing a launch depends on besides its arguments:
 *     calls from several host threads on distinct streams are safe (the workspace of
 *     dmb_deconv3d_k3s2_f32 must then be distinct per stream, see there).  The release library
 *     exports exactly the functions declared here (tests/test_host_logic.py compares the two lists);
 *     kernel-variant switches exist only in the development build (build.py dev=True ->
 *     lib/libdmb_hip_dev.so, used by scripts/, never by the package, the tests or bench.py).
 *
 * Sizes:
 *   - inside ONE batch item the kernels address memory with 32-bit byte offsets (hand-built buffer resources, LDS-DMA copies):
 *     where an entry point says that an item -- or some channels of it -- stays "below 2 GiB", a larger one is refused with
 *     DMB_EUNSUPPORTED before any launch;
 *   - ACROSS batch items every base is 64-bit, so the size of an operand as a whole is limited only by the batch count: a tensor
 *     may pass 2 GiB, 4 GiB and 2^31 elements as long as each item stays within the rule above.  Where the batch count is a grid
 *     dimension -- most entry points -- B may be at most 65535 (dmb_cat_fms_bwd_f32 / dmb_dif_fms_bwd_f32: B * C); beyond that the
 *     call returns DMB_EUNSUPPORTED or the launch's hipError_t, and nothing is computed;
 *   - element and row counts (`rows`, `n`, `n_elements`, `S`) are `long long`.
 *   Supported or refused, never silently wrong: tests/test_large_tensors_gpu.py launches the entry points on operands of more than
 *   2^31 elements, the size coming from B alone, and compares every item with launches on slices below 2 GiB.
 *
 * Each entry point names the reference interface it replaces (file:line under the reference
 * tree).  The reference is pure PyTorch on this path, so "replaces" means: the same
 * arithmetic that those torch calls perform, as one hand-written HIP kernel launch.
 */
#ifndef DMB_HIP_H
#define DMB_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define DMB_OK 0
#define DMB_EINVAL 100001   /* bad argument (NULL pointer, non-positive size, D too large ...) */
#define DMB_EUNSUPPORTED 100002 /* shape outside what the kernels are instantiated for */

#define DMB_MAX_DISP_SAMPLES 256 /* upper bound on the number of disparity samples D */

/* ABI version: bumped whenever a signature below changes (13: dmb_upsample_plan and dmb_upsample_bwd_plan added; 12: dmb_conv_wgrad_plan added; 11: dmb_conv2d_plan added; 10: dmb_conv3d_k3_plan added; 9: dmb_deconv3d_k3s2_plan added; 8: dmb_bn_train_fwd_f32, dmb_catconv_pack_weights_f32, dmb_conv3d_pack_weights_multi_f32, dmb_cat_first_wgrad_maps_f32, dmb_conv3d_k3_bnstats_f32 and dmb_bn_train_act_f32 added, dmb_bn_act_bwd_f32 takes the gradient its
 * skip operand already holds (`dres_acc`); 7: DMB_CONV_SINGLE_CHAIN in the `relu` argument of the convolution
 * entry points, `flags` argument of dmb_conv3d_k3_c1_f32; 6: dmb_stereo_pad_normalize_f32 / _u8 added; 5: dmb_fast_fms_bwd_f32 takes a mode, the forward's norm and an
 * optional gradient buffer for per-pixel samples; 4: workspace argument of dmb_deconv3d_k3s2_f32, the merged-heads entry
 * points of version 3 removed).  The define is the one place the number is written: dmb_abi_version() returns it and the Python
 * binding reads it from this file. */
#define DMB_ABI_VERSION 13
int dmb_abi_version(void);
/* Static string describing the last DMB_E* code returned on this thread ("" if none). */
const char* dmb_last_error(void);
/* sha256 (hex) of the sources this binary was built from: every translation unit, the shared headers, this file and the
 * compiler flags (densematchingbenchmark_amd/build.py::sources_digest).  The Python binding refuses a library whose id does
 * not match the sources next to it -- a prebuilt library that travels with a snapshot is then PROVEN to be built from that
 * snapshot's sources, not merely assumed to be. */
const char* dmb_build_id(void);

/* ------------------------------------------------------------------------------------------
 * Cost-volume builders
 * ---------------------------------------------------------------------------------------- */

/* cat_fms: dmb/modeling/stereo/cost_processors/utils/cat_fms.py:7-48.
 *   out[b, c,   k, y, x] = L[b, c, y, x]        if in range else 0
 *   out[b, C+c, k, y, x] = R[b, c, y, x - d_k]  if in range else 0
 * "in range": d_k > 0 -> x >= d_k;  d_k == 0 -> all x;  d_k < 0 -> x < W + d_k  (cat_fms.py:36-44)
 * L, R: [B, C, H, W]; out: [B, 2C, D, H, W]; disp_idx_host: D ints on the HOST, d_k as produced by
 * int(linspace(start, start+max_disp-1, D)[k]) (cat_fms.py:28-35).  Pure copy: bit-exact. */
int dmb_cat_fms_f32(const float* L, const float* R, float* out, int B, int C, int H, int W, int D,
                    const int* disp_idx_host, void* stream);

/* dif_fms: dmb/modeling/stereo/cost_processors/utils/dif_fms.py:7-46.
 *   out[b, c, k, y, x] = L[b, c, y, x] - R[b, c, y, x - d_k] if in range else 0;  out: [B, C, D, H, W]. */
int dmb_dif_fms_f32(const float* L, const float* R, float* out, int B, int C, int H, int W, int D,
                    const int* disp_idx_host, void* stream);

/* fast_cat_fms: dmb/modeling/stereo/cost_processors/utils/cat_fms.py:51-82 (CAT_FUNCS["fast_mode"]; the builder
 * DeepPruner.py:192 calls with per-pixel samples) on layers/inverse_warp_3d.py:4-52.
 *   T[b, c, k, y, x]     = tri-linear blend of R[b, c] around ix = (x - s) * W / (W - 1) - 0.5, iy = y * H / (H - 1) - 0.5,
 *                          iz = k * D / (D - 1) - 0.5, zero padding (F.grid_sample on a (size - 1)-normalised grid with
 *                          align_corners=False: what the reference computes on torch >= 1.3), s = disp_sample
 *   out[b, c,     k, y, x] = L[b, c, y, x] * (T > 0)        (cat_fms.py:77)
 *   out[b, C + c, k, y, x] = T
 * disp_sample (DEVICE): [B, D, H, W] if per_pixel else [D] (cat_fms.py:55-63: linspace(start, end, D), not truncated).
 * FP32 operation for operation as the reference on CPU: bit-exact.  D, H, W >= 2 (the reference divides by size - 1). */
int dmb_fast_cat_fms_f32(const float* L, const float* R, const float* disp_sample, float* out, int B, int C, int D, int H,
                         int W, int per_pixel, void* stream);

/* fast_dif_fms: dif_fms.py:49-86 (DIF_FUNCS["fast_mode"]; AnyNet.py:73).  out[b, c, k, y, x] = L * (T > 0) - T with T as
 * above; normalize != 0: out[b, k, y, x] = || . ||_p over the channels (dif_fms.py:80-82), out is [B, D, H, W]. */
int dmb_fast_dif_fms_f32(const float* L, const float* R, const float* disp_sample, float* out, int B, int C, int D, int H,
                         int W, int per_pixel, int normalize, float p, void* stream);

/* Backward of fast_cat_fms (mode 0), fast_dif_fms (mode 1) and fast_dif_fms(normalize=True) (mode 2): what the reference
 * obtains from torch.autograd through F.grid_sample, the expand of inverse_warp_3d.py:19-20 and torch.norm (cat_fms.py:51-82,
 * dif_fms.py:49-86).
 *   dvol: gradient of the builder's output ([B, 2C, D, H, W] / [B, C, D, H, W] / [B, D, H, W]);  dL, dR: [B, C, H, W];
 *   norm_out: mode 2 only (else NULL): the forward's output [B, D, H, W], with its p;
 *   d_samples: NULL, or [B, D, H, W] = the gradient with respect to per-pixel samples (per_pixel != 0 only: the sampler's
 *     column derivative times -(W / 2) * 2 / (W - 1), summed over the channels -- the path AnyNet.py:60-73 and
 *     DeepPruner.py:192 train through);
 *   partial: workspace of B * C * H * 2 * W floats (per output row the gradient rows of its two source rows).
 *   dL = sum_k dvol_ref * (T > 0);  dR = the sampler's adjoint of dvol_tgt (cat) or of -dvol (dif); the mask (T > 0) is a
 *   constant, as in the reference (cat_fms.py:77).
 * Sums along x go through LDS atomics (their order is the hardware's, as in the reference's own GPU backward).  Same
 * D, H, W >= 2 rule as the forward; W <= 1024 (two groups of 8 channel rows in 64 KiB of LDS: DMB_EUNSUPPORTED beyond -- the
 * forward has no such limit, the host layer refuses wider maps under autograd up front). */
int dmb_fast_fms_bwd_f32(const float* L, const float* R, const float* disp_sample, const float* dvol, const float* norm_out,
                         float* dL, float* dR, float* d_samples, float* partial, int B, int C, int D, int H, int W,
                         int per_pixel, int mode, float p, void* stream);

/* Spatial propagation scan: dmb/ops/spn (GateRecurrent2dnoind: functions/gaterecurrent2dnoind.py:10-44 on
 * src/gaterecurrent2dnoind_kernel.cu:10-166,288-345,535-552), the reference's only native op (CUDA; one kernel launch per
 * scanned line there, ONE launch here).  X, G1, G2, G3, H: [N, C, H, W].
 *   H[s, t] = (1 - g1 - g2 - g3) * X[s, t] + g1 * H[s', t - 1] + g2 * H[s', t] + g3 * H[s', t + 1],   g_k = G_k[s, t] where
 *   the neighbour lies inside the image, else 0; s along the columns if horizontal else along the rows, s' = s - 1 (s + 1 if
 *   reverse).  The line across the scan direction may hold at most 2046 positions (forward and backward alike).
 * Backward: dH = gradient of the output; writes dX, dG1, dG2, dG3 (zero where a link leaves the image).  Unlike the reference
 * (kernel.cu:317) it does not overwrite dH.  Parity UNPINNED: the reference op cannot be built here (CUDA). */
int dmb_spn_gaterecurrent2d_f32(const float* X, const float* G1, const float* G2, const float* G3, float* H_out, int N, int C,
                                int H, int W, int horizontal, int reverse, void* stream);
int dmb_spn_gaterecurrent2d_bwd_f32(const float* X, const float* G1, const float* G2, const float* G3, const float* H_fwd,
                                    const float* dH, float* dX, float* dG1, float* dG2, float* dG3, int N, int C, int H, int W,
                                    int horizontal, int reverse, void* stream);

/* Group-wise correlation volume (GwcNet).  ABSENT from the reference (README.md:16 only names it);
 * occupies the COR_FUNCS slot of cost_processors/utils/correlation1d_cost.py:29-31.  Spec:
 *   out[b, g, k, y, x] = (1/(C/G)) * sum_{c in group g} L[b,c,y,x] * R[b,c,y,x-d_k]  if in range else 0
 * L, R: [B, C, H, W], C % G == 0; out: [B, G, D, H, W] written into a tensor whose channel count is
 * `out_channels` at channel offset `out_ch_offset` (so the volume can be produced directly inside a
 * wider concatenated volume).  Sum order over the group's channels: ascending c, FP32 fma chain. */
int dmb_gwc_fms_f32(const float* L, const float* R, float* out, int B, int C, int G, int H, int W, int D,
                    const int* disp_idx_host, int out_channels, int out_ch_offset, void* stream);

/* First convolution of the aggregators (aggregators/PSMNet.py:31-33, AcfNet.py:28-31: dres0[0] = Conv3d(2C, Co, 3,
 * padding 1) + BatchNorm3d + ReLU) applied to the concatenation volume of cat_fms (cat_fms.py:7-48) with d_k = k, WITHOUT
 * the volume: the left half of that volume does not depend on z and the right half depends on (z, x) through x - z, so the
 * layer is a sum of 2-D maps (3x3 convolutions of the two feature maps with the dz slices of the weight: dmb_conv2d_f32)
 * looked up at x and at x - (z + dz - 1); see csrc/catconv.hip.  Same FP32 products, summed per dz.
 *
 * dmb_copy_window_f32: dst[r, j] = src[r, j + xs] (0 outside [0, W)), j in [0, Wd): the zero-extended / cropped feature
 *   rows the 2-D convolutions run on.
 * dmb_catconv_finalize_f32: per-dz maps -> sums over dz.  FA [B, CA, H, W] (channel dz*Co + co: left half, all taps),
 *   FB [B, CB, H, Wc] (channel (m-1)*CB/2 + dz*Co + co: left half, taps dx >= m, m = 1, 2, columns [0, Wc)),
 *   HC [B, CA, H, W+4] (right half at n = j - 4), HD [B, CA, H, Wc] (right half without the dx = 2 tap at n = j + W - Wc)
 *   -> FM [B, Co, H, W] and GM [B, Co, H, W+4] (interior planes), BAND [B, Co, H, D, 4] (left half at x = z - 2 .. z + 1 of
 *   plane z), GB [B, Co, H, D] (right half at x = W - 1 of plane z).  W % 4 == 0, D >= 3, D + 2 <= Wc <= W.
 * dmb_catconv_combine_f32: out[b, co, z, y, x] = act(scale[co] * (f + g) + shift[co]) -> [B, Co, D, H, W], one pass
 *   (planes 0 and D-1 are summed from FA / HC on the fly).  D % 4 == 0, W >= D + 8, Wc = D + 4.
 * dmb_catconv_pack_weights_f32 (ABI 8): the five conv2d weight packs of that form from the layer's weight [Co, 2C, 3, 3, 3]
 *   (dif != 0: [Co, C, 3, 3, 3] of a layer on the difference volume of dif_fms.py:7-46, right half = -w) in one launch: `packs`
 *   = 5 consecutive packs of dmb_conv2d_packed_floats(CA, C, 3) floats in the order A, B1, B2 (left half, dx taps from 0 / 1 /
 *   2), HC, HD (right half, dx taps up to 2 / 1), rows dz * Co + co, zero rows from 3 Co on (3 Co <= CA in {32, 64, 128}).
 *   A training step re-packs after every optimizer update: as torch slicing this was 25 launches. */
int dmb_catconv_pack_weights_f32(const float* w, float* packs, int Co, int C, int CA, int dif, void* stream);
int dmb_copy_window_f32(const float* src, float* dst, long long rows, int W, int Wd, int xs, void* stream);
/* t[r, x0 .. pitch) = 0 for rows r of `pitch` floats: re-zeroes the padding columns of a row-padded tensor after a convolution has
 * run over it as if they were image columns (see dmb_deconv3d_k3s2_f32, `Wout`). */
int dmb_zero_columns_f32(float* t, long long rows, int pitch, int x0, void* stream);
int dmb_catconv_finalize_f32(const float* FA, const float* FB, const float* HC, const float* HD, float* FM, float* BAND,
                             float* GM, float* GB, int B, int Co, int CA, int CB, int D, int H, int W, int Wc, void* stream);
int dmb_catconv_combine_f32(const float* FA, const float* HC, const float* FM, const float* BAND, const float* GM,
                            const float* GB, const float* scale, const float* shift, float* out, int B, int Co, int CA, int D,
                            int H, int W, int relu, void* stream);

/* correlation1d_cost (cost_processors/utils/correlation1d_cost.py:7-27), the reference's COR_FUNCS['default']:
 *   out[b, j, y, x] = leaky_relu( sum_c L[b,c,y,x] * R[b,c,y, x + j - (D-1)], negative_slope ),  0 <= j < D
 * i.e. the first D of the 2D-1 patch offsets of SpatialCorrelationSampler(kernel_size 1, patch_size (1, 2D-1), stride 1,
 * padding 0, dilation_patch 1) -- channel j is disparity D-1-j, R is 0 outside the image, no 1/C normalisation.
 * L, R: [B, C, H, W]; out: [B, D, H, W] (4-D: this volume feeds 2-D aggregators).  The sampler is a third-party
 * package absent from the reference tree (ClementPinard/Pytorch-Correlation-extension, branch fix_1.7 per
 * INSTALL.md:60-66, unpinned in requirements.txt): restated from its published semantics, parity UNPINNED. */
int dmb_correlation1d_f32(const float* L, const float* R, float* out, int B, int C, int H, int W, int D,
                          float negative_slope, void* stream);

/* Same as dmb_cat_fms_f32 but writing into channels [out_ch_offset, out_ch_offset+2C) of a volume with
 * `out_channels` channels (GwcNet's gwc+concat volume). */
int dmb_cat_fms_into_f32(const float* L, const float* R, float* out, int B, int C, int H, int W, int D,
                         const int* disp_idx_host, int out_channels, int out_ch_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * 3-D convolution family (the aggregators' layers)
 *
 * Replaces nn.Conv3d / nn.ConvTranspose3d + nn.BatchNorm3d (eval) + residual add + ReLU as composed by
 * dmb/modeling/stereo/layers/basic_layers.py:68-100,160-177, cost_processors/utils/hourglass.py:62-86 and
 * cost_processors/aggregators/{PSMNet.py:55-95, AcfNet.py:59-90, StereoNet.py:42-55}.
 *
 * Epilogue, in this order (matches the reference's op order):
 *     v = acc * scale[co] + shift[co]      (scale/shift may be NULL -> 1 / 0; BN and bias folded by caller)
 *     v = max(v, 0)                        (if relu == 2: GC-Net adds its skips to the ACTIVATED output,
 *                                           aggregators/GCNet.py:108-116)
 *     v = v + residual[...]                (residual may be NULL; same shape as y)
 *     v = max(v, 0)                        (if relu == 1: hourglass.py:67-81 activates after the skip add)
 * acc is an FP32 fma chain over (ci, kd, kh, kw) -- ONE chain per output voxel in the kernels a launch that fills the chip
 * takes.  A launch that would leave most of the chip idle (one small stereo pair per call: dmb/apis/inference.py:191-225)
 * takes a split-K form instead (csrc/conv3d_sk.hip, conv3d_c1s_kernel): the input channels of a voxel are split over the waves
 * of a workgroup and the partial chains added in a fixed order -- reproducible run to run, but the last bits then depend on which
 * form the launch's SIZE selects (batch 1 and batch 4 of the same pair may differ by an FP32 rounding of the sum).
 * DMB_CONV_SINGLE_CHAIN, or-ed into the `relu` argument of dmb_conv3d_k3_f32 / dmb_deconv3d_k3s2_f32 / dmb_conv2d_f32 (bits 0-7
 * stay the activation mode) or passed as `flags` of dmb_conv3d_k3_c1_f32, keeps a launch on the single-chain kernels whatever its size:
 * results are then bit-identical across batch sizes (slower for small launches: 31-35 us instead of 13-15 us per layer of the
 * deepest hourglass level of one 256x512 pair).
 * ---------------------------------------------------------------------------------------- */
#define DMB_CONV_SINGLE_CHAIN 0x100

/* Number of floats of the packed-weight buffer for a k=3 convolution / transposed convolution (input channels are
 * zero-padded to a multiple of 8 inside the packed stream, so any Ci >= 1 is accepted). */
long long dmb_conv3d_packed_floats(int Co, int Ci);
long long dmb_deconv3d_packed_floats(int Ci, int Co);

/* Re-order nn.Conv3d weights [Co, Ci, 3, 3, 3] into the MFMA B-fragment stream the kernels read. */
int dmb_conv3d_pack_weights_f32(const float* w, float* wpack, int Co, int Ci, void* stream);
/* Re-order nn.ConvTranspose3d weights [Ci, Co, 3, 3, 3] (stride 2, pad 1, output_padding 1). */
int dmb_deconv3d_pack_weights_f32(const float* w, float* wpack, int Ci, int Co, void* stream);

/* Conv3d, kernel 3, padding 1, stride 1 or 2 (all three axes).  x: [B, Ci, D, H, W];
 * y: [B, Co, Do, Ho, Wo] with Do = (D - 1) / stride + 1 etc.  Co in {32, 64, 128}: MFMA implicit GEMM using
 * wpack from dmb_conv3d_pack_weights_f32.  Any Ci >= 1.  8 channels of one batch item must stay below 2 GiB
 * (buffer resources cover one channel chunk at a time, so the tensors themselves may be larger). */
int dmb_conv3d_k3_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                      const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W,
                      int stride, int relu, void* stream);
/* What dmb_conv3d_k3_f32 would run for a launch, without launching anything or touching a device: a pure function of its
 * arguments.  Pointers enter as their alignment in bytes (a power of two; 16 or more = 16-byte aligned; 16 for a NULL residual);
 * single_chain: whether DMB_CONV_SINGLE_CHAIN is set; ncu: the device's compute units, or <= 0 for the current device's (256 where
 * there is none).  Returns
 *   (form << 8) | index  with form 1 = split-K over the eight waves of a workgroup (small launches, Co 32 or 64, Ci % 16 == 0, 16-byte
 *                          rows): index = variant + 4 at stride 2; variant 1 = 16 x 2 output voxels and one 32-channel row tile per
 *                          workgroup, 3 = 32 x 2 voxels and both row tiles (stride 2, 32 -> 64 only): 0x101, 0x105, 0x107;
 *                        form 2 = stride 1, 16-byte rows (W % 4 == 0, 16-byte aligned x / y / residual, one batch item of the output
 *                          below 2 GiB).  32 output channels: index 0 = 48 columns x 4 rows, 1 = 24 x 8, 2 = 32 x 4, 3 = 32 x 2 (four
 *                          z-slices each; the tile dmb_conv3d_k3_bnstats_f32 takes too); 64 output channels: 4 = runs of 64 voxels of
 *                          the (y, x) plane in memory order, 5 = 40 x 4, 6 = 24 x 4, 7 = 32 x 4, 8 = 16 x 2 (two z-slices each);
 *                        form 3 = stride 1, flattened tiles with dword staging (any W, 4-byte aligned operands): index 0 / 1 = 32
 *                          output channels, 60 / 52 columns x 4 rows x 4 z-slices; 2 / 3 = 64 output channels, 60 / 52 x 4 x 2;
 *                        form 4 = stride 1, 128 output channels: index 0 (60 columns x 2 rows x 2 z-slices, dword staging);
 *                        form 5 = stride 2.  64 output channels with 16-byte input rows (W % 4 == 0, 16-byte aligned x), in OUTPUT
 *                          voxels, two z-slices each: index 0 / 1 / 2 = 30 columns x 1 / 2 / 4 rows with the 8-byte epilogue (8-byte
 *                          aligned y / residual), 3 = 22 columns x 4 rows, 4 = 30 x 4 with the dword epilogue; dword staging, 30
 *                          columns x 4 rows: 5 = 64, 6 = 32 (four z-slices), 7 = 128 output channels (one z-slice);
 *   or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused with that code (dmb_last_error() then names the reason).
 * Every form is ONE k-ordered fma chain per output -- the same bits whatever the tile -- except split-K, which is planned for small
 * launches only and never under single_chain. */
int dmb_conv3d_k3_plan(int B, int Ci, int Co, int D, int H, int W, int stride, int x_align, int y_align, int residual_align,
                       int single_chain, int ncu);

/* Conv3d kernel 3 pad 1 stride 1 with ONE output channel (classifier heads: PSMNet.py:46,50,54,
 * StereoNet.py:39).  w: raw [1, Ci, 3, 3, 3]; bias_host: scalar added to every output; residual may be
 * NULL (PSMNet.py:71-72 adds the previous level's cost).  y: [B, 1, D, H, W].  flags: 0 or DMB_CONV_SINGLE_CHAIN. */
int dmb_conv3d_k3_c1_f32(const float* x, const float* w, float bias, const float* residual, float* y,
                         int B, int Ci, int D, int H, int W, int flags, void* stream);

/* The classifier tail of PSMNet.py:44-54 as one convolution launch + one finishing pass:
 *   y = conv3d_c1(act(scale * conv3d(x, w) + shift), w_head) + bias (+ residual),   x: [B, Ci, D, H, W] -> y: [B, 1, D, H, W]
 * The 32-channel tensor between the two layers never reaches memory: the 32 -> 32 kernel applies the head to its accumulator
 * tiles on the matrix cores and leaves, per 4 x 4 x 48 tile of voxels, the head's partial sums over the 6 x 6 x 50 voxels that
 * tile reaches in workspace[tile]; the finishing pass adds the (at most eight) partial sums covering a voxel in ascending tile
 * order.  Reproducible run to run and independent of workgroup placement, but NOT the single fma chain of dmb_conv3d_k3_f32 +
 * dmb_conv3d_k3_c1_f32 (per tap a chain over channels, then taps, then tiles: the last bits differ); with DMB_CONV_SINGLE_CHAIN
 * in `relu` the call returns DMB_EUNSUPPORTED.
 * wpack: dmb_conv3d_pack_weights_f32(w, 32, Ci); head_wpack: DMB_CONV3D_HEAD_PACKED_FLOATS floats from
 * dmb_conv3d_head_pack_weights_f32 (w_head: raw [1, 32, 3, 3, 3]); scale / shift: 32 floats or NULL; relu: 0 or 1.
 * workspace: dmb_conv3d_k3_head_workspace_floats(B, D, H, W) floats of caller-owned device memory, 8-byte aligned, fully
 * overwritten by the launch (the library allocates nothing; calls that may overlap in time need different workspaces).  That
 * function returns 0 -- and the launch DMB_EUNSUPPORTED -- for volumes without 16-byte rows (W % 4 != 0, x not 16-byte aligned) or
 * with 32 channels of one batch item at 2 GiB or more.  The kernel's tile is 4 x 4 x 48 voxels whatever the volume;
 * dmb_conv3d_k3_head_preferred returns 1 where dmb_conv3d_k3_f32 would pick that tile for the 32 -> 32 layer on its own (elsewhere
 * another tile shape covers the volume in fewer rounds and the two separate launches are the better choice). */
#define DMB_CONV3D_HEAD_PACKED_FLOATS 1024
long long dmb_conv3d_k3_head_workspace_floats(int B, int D, int H, int W);
int dmb_conv3d_k3_head_preferred(int B, int D, int H, int W);
int dmb_conv3d_head_pack_weights_f32(const float* w_head, float* head_wpack, void* stream);
int dmb_conv3d_k3_head_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                           const float* head_wpack, float bias, const float* residual, float* y, float* workspace,
                           int B, int Ci, int D, int H, int W, int relu, void* stream);
/* The two halves of dmb_conv3d_k3_head_f32 as calls of their own (that entry point IS the first followed by the second with one
 * level), for a chain of classifier tails whose costs accumulate (PSMNet.py:70-72: cost_k = classif_k(out_k) + cost_{k-1}):
 * dmb_conv3d_k3_head_partial_f32: the convolution launch alone; it leaves the head's partial sums in `workspace` (same size,
 *   alignment and "fully overwritten" rule as above) and writes nothing else.
 * dmb_conv3d_head_chain_finish_f32: ONE finishing pass for nlevels (1 .. 4) such workspaces of the same B, D, H, W.
 *   workspaces / y: HOST arrays of nlevels device pointers; bias_host: nlevels floats on the host; residual: NULL or [B, 1, D, H, W].
 *     y[0] = (sum of workspaces[0]'s tiles in ascending tile order) + bias_host[0] (+ residual)
 *     y[k] = ((sum of workspaces[k]'s tiles) + bias_host[k]) + y[k - 1]
 *   -- bit for bit what nlevels calls of dmb_conv3d_k3_head_f32 with residual = the previous level's y give, without reading
 *   any y back.  The y[k] may be the consecutive parts of one buffer; 16-byte aligned y / residual take 16-byte accesses,
 *   4-byte aligned ones are accepted. */
int dmb_conv3d_k3_head_partial_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                                   const float* head_wpack, float* workspace, int B, int Ci, int D, int H, int W, int relu,
                                   void* stream);
int dmb_conv3d_head_chain_finish_f32(int nlevels, const float* const* workspaces, const float* bias_host, const float* residual,
                                     float* const* y, int B, int D, int H, int W, void* stream);

/* ConvTranspose3d kernel 3, stride 2, padding 1, output_padding 1 (hourglass.py:52-60):
 * x: [B, Ci, D, H, W] -> y: [B, Co, 2D, 2H, Wout];  y[o] += x[i] * w[k] with o = 2i - 1 + k.  Co = 64 or any Co <= 32
 * (fewer than 32: zero-padded weight rows, e.g. GC-Net's 1-channel output layer, aggregators/GCNet.py:63-67).
 * Wout: the output (and residual) row length: 2W -- or, for an input whose rows are ZERO-PADDED on the right to a 16-byte multiple
 * (an image of Wi columns stored with W = Wi rounded up to a multiple of 4: the hourglass's deepest level at the KITTI shape is
 * 78 columns wide), Wout = 2 Wi < 2W with Wout % 4 == 0: only output columns below Wout exist.  Such a padded input must
 * hold zeros in its padding columns (dmb_copy_window_f32 / dmb_zero_columns_f32); it keeps the layer on the 16-byte paths.
 * Wout < 2W needs the workspace form (Co = 32 or 64, Ci % 16 == 0, aligned operands), otherwise DMB_EUNSUPPORTED.
 * workspace: DMB_DECONV3D_WORKSPACE_BYTES of device memory, 4-byte aligned, holding ZEROS (the caller zeroes it once, e.g.
 * at allocation); the launch uses it for its work-item counters and leaves it zeroed again, so the same workspace serves
 * every later call on that stream, eager or replayed from a captured graph.  Launches that may be in flight at the same
 * time (different streams) need different workspaces.  NULL selects the kernel form without counters (static tile walk:
 * same results bit for bit, slower). */
#define DMB_DECONV3D_WORKSPACE_BYTES 2048
int dmb_deconv3d_k3s2_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                          const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int Wout,
                          int relu, void* workspace, void* stream);
/* What dmb_deconv3d_k3s2_f32 would run for a launch, without launching anything or touching a device: a pure function of its
 * arguments.  Pointers enter as their alignment in bytes (a power of two; 16 or more = 16-byte aligned; 16 for a NULL residual;
 * workspace_align 0 = no workspace); single_chain: whether DMB_CONV_SINGLE_CHAIN is set; ncu: the device's compute units, or
 * <= 0 for the current device's (256 where there is none).  Returns
 *   (form << 8) | tile   with form 1 = split-K over the waves of a workgroup: tile 0 (16 x 2 input positions, four waves);
 *                        form 2 = work queue (needs the workspace; the only form besides split-K that takes Wout < 2 W):
 *                          tile 0 = 28, 1 = 32, 2 = 64 real input columns per item (+ 4 for 64 output channels);
 *                        form 3 = two-parity items, static walk: tile 0 = 60 columns with dword staging, 1 = 60 columns with 16-byte
 *                          staging and the 8-byte epilogue, 2 = 60 columns with the 16-byte epilogue, 3 / 4 = 2 rows x 28 columns with
 *                          the 8- / 16-byte epilogue (+ 5 for 64 output channels);
 *   or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused with that code (dmb_last_error() then names the reason).
 * Every form computes the same fma chain per output except split-K, which dmb_deconv3d_k3s2_f32 picks for small launches only. */
int dmb_deconv3d_k3s2_plan(int B, int Ci, int Co, int D, int H, int W, int Wout, int x_align, int y_align, int residual_align,
                           int workspace_align, int single_chain, int ncu);

/* Conv3d, kernel 3, padding 1, stride 1 along D and stride_hw along H and W (DeepPruner's HWHourglass,
 * cost_processors/utils/hw_hourglass.py:31-74).  x: [B, Ci, D, H, W]; y: [B, Co, D, (H - 1) / stride_hw + 1,
 * (W - 1) / stride_hw + 1].  stride_hw == 2 with Co in {16, 32, 64, 128}, or stride_hw == 1 with Co == 16 (the 32 -> 16 layer of
 * aggregators/DeepPruner.py:36; the other stride-1 widths are dmb_conv3d_k3_f32's).  wpack from dmb_conv3d_pack_weights_f32 (Co =
 * 16 is its 32-row stream with 16 zero rows).  Any Ci >= 1, any D, H, W >= 1, operands 4-byte aligned.  Epilogue as above.  Every
 * launch is ONE fma chain per output voxel in the packed stream's order (DMB_CONV_SINGLE_CHAIN is accepted and changes nothing):
 * a stride-(1, 2, 2) result equals the single-chain stride-1 result at even (y, x) bit for bit, and batch item i equals the item
 * run alone.  DMB_EINVAL on NULL / non-positive arguments, DMB_EUNSUPPORTED outside the sets above, both before any device call. */
int dmb_conv3d_k3_hw_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                         const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W,
                         int stride_hw, int relu, void* stream);

/* ConvTranspose3d kernel 3, stride (1, 2, 2), padding 1, output_padding (0, 1, 1) (hw_hourglass.py:41-44,56-59,71-74):
 * x: [B, Ci, D, H, W] -> y: [B, Co, D, 2H, 2W];  y[od, oy, ox] += x[id, iy, ix] * w[kd, ky, kx] with od = id - 1 + kd,
 * oy = 2 iy - 1 + ky, ox = 2 ix - 1 + kx.  Co in {16, 32, 64}; any Ci >= 1, any D, H, W >= 1, operands 4-byte aligned.  wpack from
 * dmb_deconv3d_pack_weights_f32.  No workspace: a static tile walk, one fma chain per output voxel (channel pair ascending, the
 * taps of the voxel's parity class ascending), reproducible and batch-invariant.  Epilogue and error codes as above. */
int dmb_deconv3d_k3_hw_f32(const float* x, const float* wpack, const float* scale, const float* shift,
                           const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int relu,
                           void* stream);

/* ------------------------------------------------------------------------------------------
 * Cost up-sampling
 * ---------------------------------------------------------------------------------------- */

/* F.interpolate(mode='trilinear', align_corners=True) of a 1-channel volume (PSMNet.py:77-93):
 * x: [B, Di, Hi, Wi] -> y: [B, Do, Ho, Wo];  src = dst * (in-1)/(out-1) per axis. */
int dmb_trilinear_ac_f32(const float* x, float* y, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                         void* stream);

/* nn.ConvTranspose3d(1, 1, kernel 8, stride 4, padding 2, bias=False) called with output_size =
 * [4D, 4H, 4W] (AcfNet.py:55-57,81-83): y[o] = sum x[i] * w[k], o = 4i - 2 + k.  w: [8, 8, 8]. */
int dmb_deconv3d_k8s4_c1_f32(const float* x, const float* w, float* y, int B, int D, int H, int W,
                             void* stream);

/* The same up-sampling with the standard soft-argmin of the volume it writes folded in (what dmb_trilinear_ac_soft_argmin_f32 is
 * to the tri-linear up-sampling): y [B, 4D, 4H, 4W] and disp [B, 1, 4H, 4W] = soft_argmin(y, samples, alpha, normalize) bit
 * for bit, one pass.  disp may be NULL (up-sampling only, z-column form).  Per-output arithmetic = dmb_deconv3d_k8s4_c1_f32. */
int dmb_deconv3d_k8s4_c1_soft_argmin_f32(const float* x, const float* w, float* y, float* disp, int B, int D, int H, int W,
                                         float alpha, const float* disp_sample_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * Disparity regression
 * ---------------------------------------------------------------------------------------- */

/* SoftArgmin / FasterSoftArgmin with the module's own linspace samples
 * (disp_predictors/soft_argmin.py:45-75, faster_soft_argmin.py:51-75):
 *   p = softmax(alpha * cost, dim=1) if normalize else alpha * cost;  disp = sum_k p_k * (start + k*step)
 * with the sample values passed as a host array (they are linspace(start, end, D) in FP32).
 * cost: [B, D, H, W] -> disp: [B, 1, H, W]. */
int dmb_soft_argmin_f32(const float* cost, float* disp, int B, int D, int H, int W, float alpha,
                        int normalize, const float* disp_sample_host, void* stream);

/* SoftArgmin with a per-pixel disparity-sample tensor (soft_argmin.py:67-72): sample: [B, D, H, W]. */
int dmb_soft_argmin_sampled_f32(const float* cost, const float* sample, float* disp, int B, int D, int H,
                                int W, float alpha, int normalize, void* stream);

/* LocalSoftArgmin (disp_predictors/local_soft_argmin.py:48-105).  argidx (may be NULL) receives the
 * arg-max index per pixel as int64 [B, 1, H, W] -- the bit-exact "index path" (first maximal index,
 * torch.argmax semantics). */
int dmb_local_soft_argmin_f32(const float* cost, float* disp, long long* argidx, int B, int D, int H, int W,
                              int radius, int radius_dilation, int start_disp, int dilation, float alpha,
                              void* stream);

/* Producer-fused form of the two calls above: F.interpolate(..., 'trilinear', align_corners=True) AND the soft-argmin
 * (normalize=True, disp_sample given per plane) of the up-sampled volume in one pass: y [B, Do, Ho, Wo] is written as
 * by dmb_trilinear_ac_f32 and disp [B, 1, Ho, Wo] equals dmb_soft_argmin_f32(y) bit for bit, without re-reading y
 * (aggregators/PSMNet.py:75-88 followed by disp_predictors/faster_soft_argmin.py:51-71). */
int dmb_trilinear_ac_soft_argmin_f32(const float* x, float* y, float* disp, int B, int Di, int Hi, int Wi, int Do,
                                     int Ho, int Wo, float alpha, const float* disp_sample_host, void* stream);

/* Opt-in fused fast path: trilinear(align_corners=True) up-sampling of the 1/4-resolution cost
 * [B, Di, Hi, Wi] to [B, Do, Ho, Wo] + soft-argmin, without materialising the full-resolution volume.
 * Legal only when the caller does not need `costs` back (SURVEY 7.3 "costs are part of the return
 * contract"). */
int dmb_trilinear_soft_argmin_f32(const float* x, float* disp, int B, int Di, int Hi, int Wi, int Do, int Ho,
                                  int Wo, float alpha, const float* disp_sample_host, void* stream);

/* What the up-sampling entry points above would launch, without launching anything: a pure function of its arguments, in the
 * conventions of dmb_deconv3d_k3s2_plan (csrc/upsample_plan.h).  entry: which entry point --
 *   DMB_UPSAMPLE_TRILINEAR_AC               dmb_trilinear_ac_f32
 *   DMB_UPSAMPLE_TRILINEAR_AC_SOFT_ARGMIN   dmb_trilinear_ac_soft_argmin_f32
 *   DMB_UPSAMPLE_TRILINEAR_SOFT_ARGMIN      dmb_trilinear_soft_argmin_f32
 *   DMB_UPSAMPLE_K8S4                       dmb_deconv3d_k8s4_c1_soft_argmin_f32 with disp == NULL
 *   DMB_UPSAMPLE_K8S4_SOFT_ARGMIN           dmb_deconv3d_k8s4_c1_soft_argmin_f32 with disp
 * (the k8 / s4 entries read B and Di, Hi, Wi = D, H, W; the output is exactly 4x and Do, Ho, Wo are not read).
 * ncu: compute units to plan for, <= 0 = the current device's (256 where there is none); only form 3 depends on them.
 * Returns (kernel << 8) | index:
 *   kernel 1  z-column walk, four output columns per thread (dmb_trilinear_ac_f32 with Ho <= 65535):
 *             index = (flat layout ? 8 : 0) + log2(zsplit).  flat (Wo % 4 == 0): the (row, 4-column word) pairs of a plane are one
 *             linear range dealt to the threads; row layout otherwise: grid y = the output row.  zsplit = 1, 2, 4, 8, 16 parts of the
 *             plane walk: doubled while the grid has fewer than 2048 workgroups, zsplit * 2 <= Do and zsplit < 16
 *   kernel 2  one thread per four outputs of one (plane, row) pair (dmb_trilinear_ac_f32 with Ho > 65535):  0
 *   kernel 3  z-column walk with the soft-argmin folded in:  index = (flat ? 2 : 0) + (four columns per thread ? 1 : 0);  ONE column per
 *             thread while B * Ho * ceil(Wo / 4) < 4 * 64 * ncu (four columns would leave less than a wave per SIMD)
 *   kernel 4  one thread per output pixel, no volume written (dmb_trilinear_soft_argmin_f32):  0
 *   kernel 5  k8 / s4 z-column walk:  index = (with the regression ? 4 : 0) + threads / 64 - 1;  a row's W threads in ceil(W / 256)
 *             workgroups of equal size, rounded up to whole waves: 64, 128, 192 or 256 threads
 * or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused with that code (dmb_last_error() then names the reason):
 * a non-positive extent; more disparity samples (Do; k8 / s4: 4 D) than DMB_MAX_DISP_SAMPLES for the entries with a regression; a
 * grid out of range (B > 65535; Ho > 65535 for every entry but the first; ceil(Wo / 1024) * Do * Ho > 2^31 - 1 for the first).
 * detail_host: NULL, or 7 host ints that receive the rest of the plan: output columns per thread, flat (1) or row (0), zsplit, the
 * grid's x, y, z, threads per workgroup. */
#define DMB_UPSAMPLE_TRILINEAR_AC 1
#define DMB_UPSAMPLE_TRILINEAR_AC_SOFT_ARGMIN 2
#define DMB_UPSAMPLE_TRILINEAR_SOFT_ARGMIN 3
#define DMB_UPSAMPLE_K8S4 4
#define DMB_UPSAMPLE_K8S4_SOFT_ARGMIN 5
int dmb_upsample_plan(int entry, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int ncu, int* detail_host);

/* ------------------------------------------------------------------------------------------
 * AcfNet confidence head (cmn/cmn.py:10-36,57-69)
 *   h = relu(conv2d_3x3(cost, w1) * scale + shift)   w1: [Cm, D, 3, 3], pad 1, no bias, BN folded
 *   conf = sigmoid(sum_m h_m * w2[m])                w2: [Cm]
 * cost: [B, D, H, W] -> conf: [B, 1, H, W].  w1pack from dmb_conf_head_pack_weights_f32.
 * ---------------------------------------------------------------------------------------- */
long long dmb_conf_head_packed_floats(int Cm, int D);
int dmb_conf_head_pack_weights_f32(const float* w1, float* w1pack, int Cm, int D, void* stream);
int dmb_conf_head_f32(const float* cost, const float* w1pack, const float* scale, const float* shift,
                      const float* w2, float* conf, int B, int D, int Cm, int H, int W, void* stream);

/* The same head when `cost` is AcfNet's learned 4x up-sampling (ConvTranspose3d(1, 1, 8, 4, 2), aggregators/AcfNet.py:
 * 55-57,81-83) of a quarter-resolution volume c [B, Dq, Hq, Wq]: the head's 3x3 convolution composed with the up-sampling
 * is, per output phase (Y mod 4, X mod 4), a 3x3 convolution of c (Dq channels) -- 4x fewer multiplications, run on
 * dmb_conv2d_f32 with the composed weights (host side: ops.conf_head_k8s4_pack) into hq [B, 16*M, Hq, Wq], channel =
 * (phase_y*4 + phase_x)*M + m, BatchNorm + ReLU applied.
 * dmb_conf_gather_f32: conf[b, 0, 4y'+py, 4x'+px] = sigmoid(sum_m hq[b, (py*4+px)*M + m, y', x'] * w2[m]).
 * dmb_conf_ring_f32: the outermost pixel ring of conf recomputed directly from the up-sampled volume cost [B, D, H, W]
 *   (there the head zero-pads the volume, which the composed form cannot see); w1t = w1 transposed to [D, 3, 3, M], M = 64. */
int dmb_conf_gather_f32(const float* hq, const float* w2, float* conf, int B, int M, int Hq, int Wq, void* stream);

/* The same composed head WITHOUT the hidden tensor, in one launch: for each of the nsets weight sets laid out one after the
 * other in wpack (set p = the sub-pixel phases 2 p and 2 p + 1 x 64 hidden channels, weights of ops.conf_head_k8s4_pack), the
 * 3x3 convolution Ci -> 128 of the quarter-resolution volume c [B, Ci, Hq, Wq] with BN scale/shift and ReLU, each pixel's
 * 64-vector reduced against w2 [64] in the kernel's epilogue, sigmoid, scattered to conf[b, 0, 4 y + by, 4 x + bx]
 * (phase = 4 by + bx).  Replaces conv2d + dmb_conf_gather_f32 on the composed path (cmn/cmn.py:27-43 on
 * aggregators/AcfNet.py:55-57,81-83); nsets = 8 covers all 16 phases. */
int dmb_conf_phase_conv2d_f32(const float* c, const float* wpack, const float* scale, const float* shift, const float* w2,
                              float* conf, int B, int Ci, int Hq, int Wq, int nsets, void* stream);
int dmb_conf_ring_f32(const float* cost, const float* w1t, const float* scale, const float* shift, const float* w2,
                      float* conf, int B, int D, int M, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation accumulator (data/datasets/evaluation/stereo/pixel_error.py:6-73 + eval.py:12-31 crop +
 * tools/test.py:304-307 averaging).  For every image b: crop est/gt [Hp, Wp] to rows [Hp-H0, Hp) and
 * columns [0, W0); mask = gt > lb && gt < ub; if the mask is non-empty
 *     acc[0] += 1; acc[1] += mean|gt-est|; acc[2..5] += 100 * mean(|gt-est| > {1,2,3,5})
 * (an empty mask contributes an image with all-zero errors, pixel_error.py:48-55).  acc: 6 doubles on
 * the device, updated in stream order (no atomics); the caller zeroes it and all-reduces it across
 * ranks.  workspace: DMB_EPE_WORKSPACE_DOUBLES * B doubles of caller-owned device scratch, fully overwritten by the
 * call: every image is reduced in 64 slices whose sums are added in a fixed order, so the per-image means are
 * reproducible bit for bit (since ABI version 3; version 2 took 6*B doubles and summed the slices atomically). */
#define DMB_EPE_WORKSPACE_DOUBLES 384
int dmb_epe_accum_f64(const float* est, const float* gt, double* acc, double* workspace, int B, int Hp, int Wp,
                      int H0, int W0, float lb, float ub, void* stream);

/* The same for up to 4 estimates against ONE ground truth in a single pass (the disparity maps of one forward:
 * tools/test.py evaluates every entry of results['disps'] against the same batch['leftDisp']): est: HOST array of
 * nmaps device pointers; acc: [nmaps, 6] doubles, row i accumulated from est[i]; workspace: DMB_EPE_WORKSPACE_DOUBLES*B*nmaps doubles.
 * Per estimate the arithmetic is dmb_epe_accum_f64's. */
int dmb_epe_accum_multi_f64(int nmaps, const float* const* est, const float* gt, double* acc, double* workspace, int B,
                            int Hp, int Wp, int H0, int W0, float lb, float ub, void* stream);

/* ------------------------------------------------------------------------------------------
 * Data-side conventions in front of the path: dmb/data/transforms/stereo_trans.py:20-44 (CenterCrop), :92-119 (StereoPad),
 * :78-90 (Normalize), composed in the order of dmb/data/datasets/stereo/builder.py:22-28 and dmb/apis/inference.py:120-129
 * (pad BEFORE normalise: a padded pixel holds (0 - mean[c]) / std[c]).  One pass:
 *   dst[b, c, y, x] = n(src[b, c, y - (th - h) + y0, x + x0])   for y >= th - h and x < w,   n(0) elsewhere;
 *   n(v) = (v - mean[c]) / std[c]  (FP32 subtract, correctly rounded FP32 divide -- torchvision's sub_().div_()), or v when
 *   mean_host / std_host are NULL (pad / crop only).
 * src: planar FP32 [B, Cs, sh, sw] (_f32) or the decoder's interleaved bytes [B, sh, sw, Cs] (_u8; imread's layout, the first
 * C <= Cs channels are taken as stereo/scene_flow/base.py:17-23 does); (y0, x0, h, w) = the window of the source that is kept
 * (the whole image: 0, 0, sh, sw); dst [B, C, th, tw] with th >= h, tw >= w, tw % 4 == 0, C <= 4. */
int dmb_stereo_pad_normalize_f32(const float* src, float* dst, int B, int C, int Cs, int sh, int sw, int y0, int x0, int h, int w,
                                 int th, int tw, const float* mean_host, const float* std_host, void* stream);
int dmb_stereo_pad_normalize_u8(const unsigned char* src_hwc, float* dst, int B, int C, int Cs, int sh, int sw, int y0, int x0,
                                int h, int w, int th, int tw, const float* mean_host, const float* std_host, void* stream);

/* ------------------------------------------------------------------------------------------
 * "Next" rows: the 2-D networks either side of the path.
 * dmb/modeling/stereo/backbones/PSMNet.py:8-129 and backbones/StereoNet.py:7-106 with
 * layers/basic_layers.py:31-46,105-123,219-243; disp_refinement/StereoNet.py:7-62 with
 * disp_refinement/utils/edge_aware.py:8-70.
 * ---------------------------------------------------------------------------------------- */

/* nn.Conv2d weights [Co, Ci, k, k] (k = 1, 3 or 5) -> MFMA A-fragment stream; Co <= 128, any Ci. */
long long dmb_conv2d_packed_floats(int Co, int Ci, int ksize);
int dmb_conv2d_pack_weights_f32(const float* w, float* wpack, int Co, int Ci, int ksize, void* stream);

/* Conv2d with padding = dilation * (k/2) + folded BatchNorm / bias (scale, shift: each may be NULL).  Supported:
 * stride 1 with kernel 1 | 3, dilation 1 | 2 (4 | 8 when Co <= 32), Co <= 128; stride 2 with kernel 1 | 3 (Co <= 64) or
 * 5 (Co <= 32), dilation 1; anything else returns DMB_EUNSUPPORTED.  Then + residual (may be NULL; added after the affine,
 * basic_layers.py:236-241) + ReLU.  x, y and residual may be channel windows of wider tensors: x points at the first input channel of batch item 0 of
 * a tensor with in_channels_total channels per item (likewise y / out_channels_total, residual / res_channels_total).
 * x: [B, Ci (of in_channels_total), H, W] -> y: [B, Co (of out_channels_total), Ho, Wo], Ho = (H - 1) / stride + 1. */
int dmb_conv2d_f32(const float* x, const float* wpack, const float* scale, const float* shift, const float* residual,
                   float* y, int B, int Ci, int Co, int H, int W, int ksize, int stride, int dilation, int relu,
                   int in_channels_total, int out_channels_total, int res_channels_total, void* stream);
/* What dmb_conv2d_f32 would run for a launch, without launching anything or touching a device: a pure function of its arguments, in
 * the conventions of dmb_conv3d_k3_plan.  The three pointers enter as the alignment in bytes of the WINDOW pointers the launch would
 * be given (16 for a NULL residual); res_channels_total: 0 for a launch without residual.  Returns
 *   (form << 8) | index  with form 1 = split-K over the eight waves of a workgroup (csrc/conv3d_sk.hip; 3x3, stride 1, dilation 1 | 2,
 *                          16-byte rows, Ci % 16 == 0 and Ci <= 128, Co % 32 == 0, at most 5 units of 16 x 2 pixels x 32 channels per
 *                          compute unit, never under single_chain): index = (dilation 2 ? 2 : 0) + (both 32-channel row tiles of a pair
 *                          in one workgroup: Co % 64 == 0 and Ci <= 64 ? 1 : 0): 0x100 .. 0x103;
 *                        form 2 = persistent tiles of 48 columns x (rows per wave x 4 / 2 / 1 waves for Co <= 32 / 64 / 128) rows; rows
 *                          per wave: 4 at stride 1, 2 at stride 2, "two-row": 2 at stride 1.  Of each pair of indices below the first =
 *                          "scalar", dword staging and stores (any W, 4-byte aligned operands), the second = 16-byte rows (W and Wo
 *                          multiples of 4, 16-byte aligned x / y / residual windows):
 *                            stride 1, 3x3:       0 / 1 = Co <= 32: scalar / two-row;  2 / 3 / 4 = Co <= 64: scalar / four rows per wave /
 *                                                 two-row, by rounds of the grid x rows, four on a tie;  5 / 6 = Co <= 128: scalar / two-row
 *                            ... dilation 2:      7 / 8 = Co <= 32,  9 / 10 = Co <= 64,  11 / 12 = Co <= 128: scalar / two-row
 *                            ... dilation 4, 8:   13 / 14,  15 / 16 (Co <= 32)
 *                            stride 1, 1x1:       17 / 18 = Co <= 32,  19 / 20 = Co <= 64,  21 / 22 = Co <= 128
 *                            stride 2, 3x3:       23 / 24 = Co <= 32,  25 / 26 = Co <= 64
 *                            stride 2, 1x1:       27 / 28 = Co <= 32,  29 / 30 = Co <= 64
 *                            stride 2, 5x5:       31 / 32 (Co <= 32)
 *                          (33 .. 35, development build only: four rows per wave for indices 1, 6 and 12, which no launch is planned)
 *   or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused with that code (dmb_last_error() then names the reason).
 * Form 2 is ONE k-ordered fma chain per output, the same bits whatever the tile, vector or scalar. */
int dmb_conv2d_plan(int B, int Ci, int Co, int H, int W, int ksize, int stride, int dilation, int in_channels_total,
                    int out_channels_total, int res_channels_total, int x_align, int y_align, int residual_align, int single_chain,
                    int ncu);

/* njobs (<= 6) independent 3x3 stride-1 convolutions of ONE layer shape (B, Ci -> Co, H) in one launch: job q convolves
 * x[q] [B, Ci, H, W[q]] with wpack[q] into y[q] (a channel window of a tensor with out_channels_total[q] channels); no affine,
 * no residual, no ReLU; W[q] % 4 == 0 and 16-byte aligned bases.  The arrays are HOST arrays of device pointers / sizes.
 * Used by the volume-free first layer (cat_fms.py:7-48 + aggregators/PSMNet.py:31-33 without the volume): its five 2-D
 * convolutions, three of them 52-column border maps that would each take a round of the chip on their own. */
int dmb_conv2d_k3_multi_f32(int njobs, const float* const* x, const float* const* wpack, float* const* y, const int* W,
                            const int* out_channels_total, int B, int Ci, int Co, int H, void* stream);

/* nn.AvgPool2d(k, stride=k) (PSMNet.py:43-58): channels [in_ch_offset, in_ch_offset + C) of x [B, in_channels_total,
 * H, W] -> y [B, C, H/k, W/k]. */
int dmb_avgpool2d_f32(const float* x, float* y, int B, int C, int H, int W, int k, int in_channels_total,
                      int in_ch_offset, void* stream);

/* F.interpolate(mode='bilinear', align_corners=True) (PSMNet.py:95-117): x [B, C, Hi, Wi] -> channels
 * [out_ch_offset, out_ch_offset + C) of y [B, out_channels_total, Ho, Wo]. */
int dmb_bilinear_ac_f32(const float* x, float* y, int B, int C, int Hi, int Wi, int Ho, int Wo, int out_channels_total,
                        int out_ch_offset, void* stream);

/* F.interpolate(mode='bilinear', align_corners=False) * mult: the coarse disparity map brought to image size and
 * rescaled by the resolution ratio (disp_refinement/StereoNet.py:49-50, disp_refinement/utils/edge_aware.py:49-50).
 * x [B, C, Hi, Wi] -> channels [out_ch_offset, out_ch_offset + C) of y [B, out_channels_total, Ho, Wo]. */
int dmb_bilinear_scale_f32(const float* x, float* y, int B, int C, int Hi, int Wi, int Ho, int Wo, float mult,
                           int out_channels_total, int out_ch_offset, void* stream);

/* ------------------------------------------------------------------------------------------
 * "Next" row (first part): the training-side loss terms of AcfNet's cost filtering, forward and
 * backward, each ONE pass over what it reads.
 * ---------------------------------------------------------------------------------------- */

/* Doubles of reduction workspace for a loss over n_elements pixels (per-block partial sums, deterministic). */
long long dmb_loss_workspace_doubles(long long n_elements);

/* StereoFocalLoss.loss_per_level with LaplaceDisp2Prob (losses/stereo_focal_loss.py:63-101, losses/utils/
 * disp2prob.py:107-173) at the cost volume's own resolution:
 *   m1 = lower < gt < upper;  g = gt*m1;  m2 = start_disp < g < end_disp;  p = softmax_d(-|s_d - g*m2| / variance);
 *   P = p*m2 + 1e-40;  loss = -sum(P * (1-P)^(-focal_coefficient) * log_softmax_d(cost) * m1) / max(sum(m1), 1).
 * cost [B, D, H, W]; gt [B, 1, H, W]; variance: per-pixel map [B, 1, H, W] or NULL (then variance_scalar);
 * disp_sample_host: D host floats (s_d).  stats: 2*B*H*W floats saved for the backward pass; loss_out: 2 floats
 * (the loss, the divisor). */
int dmb_stereo_focal_loss_fwd_f32(const float* cost, const float* gt, const float* variance, float variance_scalar,
                                  const float* disp_sample_host, float* stats, double* workspace, float* loss_out,
                                  int B, int D, int H, int W, float lower, float upper, float start_disp,
                                  float end_disp, float focal_coefficient, void* stream);
/* d loss / d cost [B, D, H, W] and (if grad_variance != NULL) d loss / d variance [B, 1, H, W], scaled by
 * grad_out[0] (device scalar, may be NULL = 1) * grad_scale. */
int dmb_stereo_focal_loss_bwd_f32(const float* cost, const float* gt, const float* variance, float variance_scalar,
                                  const float* disp_sample_host, const float* stats, const float* loss_out,
                                  const float* grad_out, float grad_scale, float* grad_cost, float* grad_variance,
                                  int B, int D, int H, int W, float lower, float upper, float start_disp,
                                  float end_disp, float focal_coefficient, void* stream);

/* Masked mean over a [B, 1, H, W] map, mask = lower < gt < upper.  mode 0: ConfidenceNllLoss, -logsigmoid(x)
 * (losses/conf_nll_loss.py:35-56, x = confidence logits); mode 1: DispSmoothL1Loss, smooth_l1(x - gt)
 * (losses/smooth_l1_loss.py:36-58, x = estimated disparity).  loss_out: 2 floats (loss, divisor). */
int dmb_map_loss_fwd_f32(const float* x, const float* gt, double* workspace, float* loss_out, long long n, float lower,
                         float upper, int mode, void* stream);
int dmb_map_loss_bwd_f32(const float* x, const float* gt, const float* loss_out, const float* grad_out,
                         float grad_scale, float* grad_x, long long n, float lower, float upper, int mode,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * "Next" row (second part): backward passes of the 3-D convolution units (autograd of the
 * nn.Sequential(Conv3d | ConvTranspose3d, BatchNorm3d[, ReLU]) factories, layers/basic_layers.py:68-100,160-177).
 * "dc" is the gradient with respect to the raw convolution output (before BatchNorm).
 *
 * Data gradients reuse the forward kernels (scale = shift = residual = NULL, relu = 0) on re-packed weights:
 *   stride-1 Conv3d   dx = dmb_conv3d_k3_f32(dc, pack_dgrad(w), stride 1)           (channels Co -> Ci)
 *   stride-2 Conv3d   dx = dmb_deconv3d_k3s2_f32(dc, dmb_deconv3d_pack_weights_f32(w, Co, Ci))   (even D, H, W of x)
 *   ConvTranspose3d   dx = dmb_conv3d_k3_f32(dy, dmb_conv3d_pack_weights_f32(w, Ci, Co), stride 2)
 * ---------------------------------------------------------------------------------------- */

/* Weights of the data-gradient convolution of a stride-1 nn.Conv3d with weight w [Co, Ci, 3, 3, 3]: channel roles
 * exchanged, taps mirrored.  wpack holds dmb_conv3d_packed_floats(Ci, Co) floats. */
int dmb_conv3d_pack_dgrad_weights_f32(const float* w, float* wpack, int Co, int Ci, void* stream);

/* Many packs in ONE launch (ABI 8).  `jobs_device`: njobs dmb_pack_job records IN DEVICE MEMORY (the caller keeps the table as
 * long as its parameters and pack buffers live; a training step re-packs every unit's forward and data-gradient weights after
 * each optimizer update -- 52 launches of 4.8 us in a PSMNet step).  mode 0: dmb_conv3d_pack_weights_f32(w, wpack, Co, Ci);
 * 1: dmb_deconv3d_pack_weights_f32(w, wpack, Ci, Co) (w = [Ci, Co, 27]); 2: dmb_conv3d_pack_dgrad_weights_f32 of a layer
 * with weight [Ci, Co, 27] (here Co = the DATA GRADIENT's output channels).  wpack: dmb_conv3d_packed_floats(Co, Ci) floats. */
typedef struct {
  const float* w;
  float* wpack;
  int Co, Ci, mode, reserved;
} dmb_pack_job;
int dmb_conv3d_pack_weights_multi_f32(const void* jobs_device, int njobs, void* stream);

/* Weight gradient of a stride-1 nn.Conv3d (kernel 3, padding 1): dw[co, ci, tap] = sum_{b, v} dc[b, co, v] *
 * x[b, ci, v + tap - 1] (torch.nn.grad.conv3d_weight).  x [B, Ci, D, H, W], dc [B, Co, D, H, W], dw [Co, Ci, 27].
 * FP32 MFMA chains per workgroup, partial results added in a fixed order (bit-reproducible, no atomics).
 * workspace: dmb_conv3d_wgrad_workspace_floats(Co, Ci) floats.  32 channels of one batch item must stay below 2 GiB. */
long long dmb_conv3d_wgrad_workspace_floats(int Co, int Ci);
int dmb_conv3d_k3_wgrad_f32(const float* x, const float* dc, float* dw, float* workspace, int B, int Ci, int Co, int D,
                            int H, int W, void* stream);
/* Weight gradient of the stride-2 units: out[cs, cb, tap] = sum_{b, o} small[b, cs, o] * big[b, cb, 2 o + tap - 1].
 *   nn.Conv3d(k 3, s 2, p 1):                 small = dc [B, Co, Ds, Hs, Ws], big = x  [B, Ci, Db, Hb, Wb] -> dW [Co, Ci, 27]
 *   nn.ConvTranspose3d(k 3, s 2, p 1, op 1):  small = x  [B, Ci, ...],        big = dy [B, Co, 2Ds, ...]  -> dW [Ci, Co, 27]
 * Each big extent is 2n or 2n - 1 (16-byte staging when both widths are multiples of 4 and the tensors aligned).
 * Db == Ds with Ds >= 2 selects the units that stride only height and width, out[cs, cb, kz, ky, kx] = sum_{b, z, y, x}
 * small[b, cs, z, y, x] * big[b, cb, z + kz - 1, 2y + ky - 1, 2x + kx - 1] (Hb, Wb: 2n or 2n - 1 as above):
 *   nn.Conv3d(k 3, s (1, 2, 2), p 1):                          small = dc, big = x  -> dW [Co, Ci, 27]
 *   nn.ConvTranspose3d(k 3, s (1, 2, 2), p 1, op (0, 1, 1)):   small = x,  big = dy -> dW [Ci, Co, 27]
 * (Ds == Db == 1 is the same sum in either reading.)  32 channels of one batch item of the big operand must stay below 2 GiB.
 * workspace: dmb_conv3d_wgrad_workspace_floats(Cs, Cb) floats. */
int dmb_conv3d_k3s2_wgrad_f32(const float* small, const float* big, float* dw, float* workspace, int B, int Cs, int Cb,
                              int Ds, int Hs, int Ws, int Db, int Hb, int Wb, void* stream);

/* Weight gradient of a stride-1 nn.Conv2d with kernel 1, or kernel 3 with dilation 1 | 2 | 4 | 8 (padding = dilation * (k / 2)):
 * AcfNet's confidence heads (cmn/cmn.py:21-36) and the stride-1 layers of the 2-D networks.  x [B, Ci, H, W],
 * dc [B, Co, H, W] -> dw [Co, Ci, k*k].  W a multiple of 4, tensors 16-byte aligned.  The data gradient is dmb_conv2d_f32 on
 * mirrored, channel-exchanged weights.  workspace: dmb_conv2d_wgrad_workspace_floats(Co, Ci) floats.
 * Kernel 5 with dilation 1 (padding 2) on 1 .. DMB_CONV2D_K5_MAX_C input and output channels -- DeepPruner's 5x5 heads,
 * dmb_conv2d_k5_small_f32 -- is taken too: dw [Co, Ci, 25], any H, W >= 1, any width, operands 4-byte aligned, the same workspace;
 * its data gradient is dmb_conv2d_k5_small_f32 on mirrored, channel-exchanged weights.
 * Kernel 3 with dilation 1 and ONE output channel on 1 .. DMB_REFINE_HEAD_MAX_C input channels -- the classifier of DeepPruner's
 * refinement head -- has a kernel of its own (plan form 7 below): any H, W >= 1, any width, operands 4-byte aligned. */
long long dmb_conv2d_wgrad_workspace_floats(int Co, int Ci);
int dmb_conv2d_wgrad_f32(const float* x, const float* dc, float* dw, float* workspace, int B, int Ci, int Co, int H, int W,
                         int ksize, int dilation, void* stream);

/* What the three weight-gradient entry points above would run for a launch, without launching anything or touching a device: a pure
 * function of its arguments, in the conventions of dmb_conv3d_k3_plan (csrc/wgrad_plan.h).  kind: which entry point --
 *   DMB_WGRAD_S1  dmb_conv3d_k3_wgrad_f32:    Co / Ci = channels of dc / x, D, H, W their extents (Db, Hb, Wb, ksize, dilation unused)
 *   DMB_WGRAD_S2  dmb_conv3d_k3s2_wgrad_f32:  Co / Ci = Cs / Cb, D, H, W = the small operand's extents, Db, Hb, Wb the big one's
 *   DMB_WGRAD_2D  dmb_conv2d_wgrad_f32:       Co / Ci = channels of dc / x, H, W, ksize, dilation (D, Db, Hb, Wb unused)
 * align: the alignment in bytes of the two operands together (of the bitwise OR of their addresses; 16 or more = 16-byte aligned);
 * ncu: compute units to plan for, <= 0 = the current device's (256 where there is none).  Returns (form << 8) | index:
 *   form 1  stride 1, tiles of 4 rows x TX columns walked along z:  0 = 24 columns, 16-byte staging;  1 = 32 columns, 16-byte staging
 *           (where 32-column tiles cover W with fewer computed columns);  2 = 24 columns, dword staging (W % 4 != 0 or align < 16)
 *   form 2  stride 2, tiles of TY x TX voxels of the small operand:  0 / 1 = 2 x 12 with 16-byte / dword staging,  2 / 3 = 4 x 8 with
 *           16-byte / dword staging (dword: either width % 4 != 0 or align < 16); 4 x 8 where its estimated cost -- rounds of the grid
 *           x (planes per segment + 1) x tile voxels / 1.1 -- is below that of 2 x 12
 *   form 3  stride 1 with ONE output channel (Co == 1):  0
 *   form 4  2-D, strips of 64 columns walked along y:  0 .. 3 = kernel 3 with dilation 1, 2, 4, 8;  4 = kernel 1
 *   form 5  DMB_WGRAD_S2 with Db == D >= 2 (stride (1, 2, 2)), tiles of 4 x 8 voxels of the small operand walked along z in segments of
 *           one plane or more:  0 / 1 = 16-byte / dword staging (dword: either width % 4 != 0 or align < 16)
 *   form 6  DMB_WGRAD_2D with ksize 5, dilation 1 and 1 .. DMB_CONV2D_K5_MAX_C channels on both sides (decided before the width and
 *           alignment rule of form 4, which it does not have):  0 = tiles of 8 rows x 32 columns, one thread per (co, ci) pair with its
 *           25 taps in registers.  detail: column tiles, 1, 8 (a tile's rows), row tiles; a slot's partial result is Co x Ci x 25 floats
 *   form 7  DMB_WGRAD_2D with ksize 3, dilation 1, ONE output channel (Co == 1) and 1 .. DMB_REFINE_HEAD_MAX_C input channels -- the
 *           classifier of DeepPruner's refinement head (decided before the width and alignment rule of form 4, which it does not
 *           have: any H, W >= 1, operands 4-byte aligned):  0 = tiles of 8 rows x 32 columns, one thread per input channel and group
 *           of pixels with its 9 taps in registers.  detail: column tiles, 1, 8 (a tile's rows), row tiles; a slot's partial result
 *           is Ci x 9 floats
 * or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused with that code (dmb_last_error() then names the reason).
 * detail_host: NULL, or 6 host ints that receive the rest of the plan: tiles along x, tiles along y (2-D: the row classes = the dilation),
 * planes (2-D: rows of a class) per segment, segments (form 3: 1 and D), workgroup slots per channel block (grid x; form 3: the
 * workgroups), 32 x 32 channel blocks (grid y).  items = B x tiles x segments; slots x blocks x taps x 1024 floats (form 3: slots x Ci x 27; form 6: slots x Co x Ci x 25; form 7: slots x Ci x 9) never
 * exceed dmb_*_wgrad_workspace_floats(Co, Ci). */
#define DMB_WGRAD_S1 1
#define DMB_WGRAD_S2 2
#define DMB_WGRAD_2D 4
int dmb_conv_wgrad_plan(int kind, int B, int Co, int Ci, int D, int H, int W, int Db, int Hb, int Wb, int ksize, int dilation, int align,
                        int ncu, int* detail_host);

/* BatchNorm (training mode) + skip add + ReLU of a convolution unit, layout [B, C, S] (S = voxels or pixels per channel).
 * relu: 0 none, 1 after the skip add, 2 before it -- the same epilogue the inference kernels fuse.
 *
 * dmb_bn_train_stats_f32: batch mean / biased variance per channel (FP64 sums, fixed order) ->
 *   mean_out, invstd_out = 1/sqrt(var + eps), scale_out = gamma*invstd, shift_out = beta - mean*scale_out (C floats each);
 *   running_mean / running_var (may be NULL) are updated as nn.BatchNorm does (momentum, unbiased variance).
 *   gamma / beta may be NULL (1 / 0).  workspace: dmb_bn_workspace_doubles(C, S) doubles.
 * dmb_bn_act_f32: y = act(c*scale + shift (+ residual)).
 * dmb_bn_train_fwd_f32 (ABI 8): both of the above for a batch-statistics unit in TWO launches instead of four -- the block
 *   sums, then one kernel whose workgroups finish their channel's statistics themselves (same arithmetic, same bits as
 *   dmb_bn_train_stats_f32), write mean / invstd / scale / shift, update the running buffers, add 1 to *num_batches_tracked (an
 *   int64 on the device, may be NULL: nn.BatchNorm's counter, basic_layers.py:68-83 under train()) and normalise.
 * dmb_bn_act_bwd_f32: dpre = dy * [ReLU mask];  dbeta = sum dpre;  dgamma = sum dpre * (c - mean)*invstd;
 *   dc = scale*(dpre - dbeta/N - xhat*dgamma/N) if training else scale*dpre;  dres (may be NULL) = the gradient flowing
 *   into the skip branch (dpre for relu 1, dy otherwise) + dres_acc (may be NULL; ABI 8: what the skip operand has already
 *   collected from its other consumers, so that autograd's own addition -- three tensor passes -- is one extra read here).
 *   y (the unit's output) is only read for relu == 1.  Two launches (block sums; apply, which finishes the sums itself). */
/* Batch statistics from the convolution's epilogue (ABI 8): dmb_conv3d_k3_bnstats_f32 is the RAW stride-1 convolution Ci -> 32
 * (no affine, skip or ReLU: what a training-mode unit computes before its BatchNorm, basic_layers.py:68-83 under train()) that also
 * writes, per workgroup and channel, the FP64 sum of its outputs and of their squares: stats[(ch * P + p) * 2 + {0, 1}], P =
 * dmb_conv3d_k3_bnstats_partials(...) (0: the shape is not covered -- call dmb_conv3d_k3_f32 and dmb_bn_train_fwd_f32).
 * dmb_bn_train_act_f32 then is dmb_bn_train_fwd_f32 without its pass over c for the block sums: it finishes the statistics from
 * those partials (mean = sum / N, var = sumsq / N - mean^2 in FP64), updates the buffers and the counter, and normalises. */
long long dmb_conv3d_k3_bnstats_partials(int B, int Ci, int Co, int D, int H, int W);
int dmb_conv3d_k3_bnstats_f32(const float* x, const float* wpack, float* y, double* stats, int B, int Ci, int Co, int D, int H, int W,
                              void* stream);
int dmb_bn_train_act_f32(const float* c, const double* partials, int nparts, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, long long* num_batches_tracked, float momentum, float eps,
                         float* mean_out, float* invstd_out, float* scale_out, float* shift_out, const float* residual, float* y,
                         int B, int C, long long S, int relu, void* stream);
long long dmb_bn_workspace_doubles(int C, long long S);
int dmb_bn_train_stats_f32(const float* c, const float* gamma, const float* beta, float* running_mean,
                           float* running_var, float momentum, float eps, float* mean_out, float* invstd_out,
                           float* scale_out, float* shift_out, double* workspace, int B, int C, long long S, void* stream);
int dmb_bn_act_f32(const float* c, const float* scale, const float* shift, const float* residual, float* y, int B, int C,
                   long long S, int relu, void* stream);
int dmb_bn_train_fwd_f32(const float* c, const float* gamma, const float* beta, float* running_mean, float* running_var,
                         long long* num_batches_tracked, float momentum, float eps, float* mean_out, float* invstd_out,
                         float* scale_out, float* shift_out, const float* residual, float* y, double* workspace, int B, int C,
                         long long S, int relu, void* stream);
int dmb_bn_act_bwd_f32(const float* dy, const float* c, const float* y, const float* scale, const float* shift,
                       const float* mean, const float* invstd, double* workspace, float* dgamma, float* dbeta, float* dc,
                       float* dres, const float* dres_acc, int B, int C, long long S, int relu, int training, void* stream);

/* out[c] = sum_{b, s} a[b, c, s] * g[b, 0, s] (FP64 sums): the weight gradient of a 1x1 convolution with one output channel
 * (second layer of AcfNet's confidence heads, cmn/cmn.py:30).  workspace: dmb_bn_workspace_doubles(C, S) doubles. */
int dmb_channel_dot_f32(const float* a, const float* g, double* workspace, float* out, int B, int C, long long S, void* stream);

/* Weight gradient of the aggregators' first convolution (aggregators/PSMNet.py:31-33 on cat_fms.py:7-48, d_k = k) WITHOUT the volume
 * (ABI 8; the backward twin of dmb_catconv_*): one pass over dc [B, Co, D, H, W] folds z into 2 x 9 maps per output channel,
 *   maps_left [B, 9 Co, H, W] (channel (dz*3 + dx)*Co + co) = sum_z dc[co, z, y, x]               over 0 <= z+dz-1 < D, x+dx-1 >= z+dz-1
 *   maps_right[B, 9 Co, H, W]                               = sum_z dc[co, z, y, u + z + dz - dx]  over 0 <= z+dz-1 < D, u+z+dz-1 < W
 * and the layer's weight gradient is two 2-D weight gradients against them (dmb_conv2d_wgrad_f32 with x = the left / right feature
 * map): dW[co, ci, dz, dy, dx] = dWL[(dz*3+dx)*Co + co, ci, dy, dx], dW[co, C + ci, dz, dy, dx] = dWR[(dz*3+dx)*Co + co, ci, dy, 1]
 * (a difference volume, dif_fms.py:7-46: dW = the left term minus the right one). */
int dmb_cat_first_wgrad_maps_f32(const float* dc, float* maps_left, float* maps_right, int B, int Co, int D, int H, int W, void* stream);

/* Backward of the cost-volume builders: dvol [B, 2C (cat) or C (dif), D, H, W] -> dL, dR [B, C, H, W]; sums over the
 * valid columns of every disparity plane (cat_fms.py:36-44), FP32 in ascending plane order.  B * C and 2 H are grid dimensions:
 * at most 65535 each, DMB_EUNSUPPORTED beyond. */
int dmb_cat_fms_bwd_f32(const float* dvol, float* dL, float* dR, int B, int C, int H, int W, int D,
                        const int* disp_idx_host, void* stream);
int dmb_dif_fms_bwd_f32(const float* dvol, float* dL, float* dR, int B, int C, int H, int W, int D,
                        const int* disp_idx_host, void* stream);

/* Backward of the soft-argmin (normalize = True): grad_cost[k] = grad_disp * alpha * p_k * (s_k - disp),
 * p = softmax(alpha * cost).  cost, grad_cost [B, D, H, W]; disp (the forward result), grad_disp [B, 1, H, W]. */
int dmb_soft_argmin_bwd_f32(const float* cost, const float* disp, const float* grad_disp, float* grad_cost, int B,
                            int D, int H, int W, float alpha, const float* disp_sample_host, void* stream);

/* Backward of dmb_trilinear_ac_soft_argmin_f32 with respect to the low-resolution cost x [B, Di, Hi, Wi]: the gradient of
 * the disparity is propagated without the [B, Do, Ho, Wo] volume (re-created per pixel in registers); grad_y (may be NULL) is
 * a gradient that arrives on the volume itself (a loss on the costs) and is added.  scratch: B*Di*Ho*Wo floats. */
int dmb_trilinear_ac_soft_argmin_bwd_f32(const float* x, const float* disp, const float* grad_disp, const float* grad_y,
                                         float* scratch, float* grad_x, int B, int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                                         float alpha, const float* disp_sample_host, void* stream);
/* Backward of dmb_trilinear_ac_f32 alone (F.interpolate(trilinear, align_corners=True)): grad_y [B, Do, Ho, Wo] ->
 * grad_x [B, Di, Hi, Wi].  scratch: B*Di*Ho*Wo floats. */
int dmb_trilinear_ac_bwd_f32(const float* grad_y, float* scratch, float* grad_x, int B, int Di, int Hi, int Wi, int Do, int Ho,
                             int Wo, void* stream);

/* Backward of dmb_avgpool2d_f32 and dmb_bilinear_ac_f32 on plain [B, C, ., .] tensors (the SPP branches of the PSMNet
 * backbone under training): grad_y -> grad_x. */
int dmb_avgpool2d_bwd_f32(const float* grad_y, float* grad_x, int B, int C, int H, int W, int k, void* stream);
int dmb_bilinear_ac_bwd_f32(const float* grad_y, float* grad_x, int B, int C, int Hi, int Wi, int Ho, int Wo, void* stream);

/* Which kernel contracts the (y, x) neighbourhoods in the three adjoints of an align_corners up-sampling above, without launching
 * anything (csrc/upsample_plan.h; the z fold before it has one form).  entry: DMB_UPSAMPLE_BWD_TRILINEAR_AC (dmb_trilinear_ac_bwd_f32),
 * DMB_UPSAMPLE_BWD_TRILINEAR_AC_SOFT_ARGMIN (dmb_trilinear_ac_soft_argmin_bwd_f32), DMB_UPSAMPLE_BWD_BILINEAR_AC
 * (dmb_bilinear_ac_bwd_f32: planes_or_Di = C, Do not read).  ncu is not read: no adjoint form depends on the device.  Returns
 *   1  row groups: a workgroup contracts the output rows that 8 input rows blend into LDS row sums, then those along y -- where
 *      both scales (in - 1) / (out - 1) are positive, Hi, Wi >= 2, the column window bound ceil(2 / sw) + 5 is at most 16 and
 *      nrmax = ceil(9 / sh) + 6 rows of Wi floats fit 64 KiB
 *   2  one thread per input voxel, every voxel's window of output columns narrower than 16: the register-window path throughout
 *   3  one thread per input voxel, some window 16 columns or wider: those voxels take the general loop
 *   4  one wave per input element (the bilinear entry with Hi * Wi * 64 <= Ho * Wo), decided before the others
 * or -DMB_EINVAL / -DMB_EUNSUPPORTED where the launch would be refused (a non-positive extent; Do outside 1 .. DMB_MAX_DISP_SAMPLES
 * for the entry with a regression; B, Ho or planes * Hi above 65535).
 * detail_host: NULL, or 6 host ints: nrmax and the LDS bytes of form 1 (else 0, 0), the grid's x, y, z, threads per workgroup. */
#define DMB_UPSAMPLE_BWD_TRILINEAR_AC 1
#define DMB_UPSAMPLE_BWD_TRILINEAR_AC_SOFT_ARGMIN 2
#define DMB_UPSAMPLE_BWD_BILINEAR_AC 3
int dmb_upsample_bwd_plan(int entry, int B, int planes_or_Di, int Hi, int Wi, int Do, int Ho, int Wo, int ncu, int* detail_host);
/* Backward of dmb_bilinear_scale_f32 (half-pixel bilinear * mult, edge_aware.py:49-50) on plain tensors. */
int dmb_bilinear_scale_bwd_f32(const float* grad_y, float* grad_x, int B, int C, int Hi, int Wi, int Ho, int Wo, float mult,
                               void* stream);

/* Backward of dmb_deconv3d_k8s4_c1_f32 (AcfNet's learned up-sampling, aggregators/AcfNet.py:55-57): dx [B, D, H, W] =
 * sum_k dy[4 i - 2 + k] w[k], dw [8, 8, 8] = sum_{b, i} x[b, i] dy[b, 4 i - 2 + k]; dy [B, 4D, 4H, 4W].  Either output may be
 * NULL.  workspace: dmb_deconv3d_k8s4_bwd_workspace_doubles() doubles (needed for dw). */
long long dmb_deconv3d_k8s4_bwd_workspace_doubles(void);
int dmb_deconv3d_k8s4_c1_bwd_f32(const float* x, const float* w, const float* dy, float* dx, float* dw,
                                 double* workspace, int B, int D, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * EXPERIMENTAL, OPT-IN (never selected by the default path): the stride-1
 * convolution (32 or 64 output channels) with every FP32 operand split exactly into three bf16 pieces and the six largest cross products issued on
 * the bf16 matrix cores with FP32 accumulation.  At least as close to the real-number result as the FP32 fma chain of
 * dmb_conv3d_k3_f32 (tests compare both with FP64), but not bit-identical to it.  Same arguments as dmb_conv3d_k3_f32
 * with stride 1; Co = 32 with W a multiple of 48, or Co = 64 with W a multiple of 24; tensors 16-byte aligned.
 * ---------------------------------------------------------------------------------------- */
long long dmb_conv3d_x6_packed_bytes(int Co, int Ci);
int dmb_conv3d_x6_pack_weights_f32(const float* w, void* wpack, int Co, int Ci, void* stream);
int dmb_conv3d_k3_x6_f32(const float* x, const void* wpack, const float* scale, const float* shift,
                         const float* residual, float* y, int B, int Ci, int Co, int D, int H, int W, int relu,
                         void* stream);

/* ------------------------------------------------------------------------------------------
 * AnyNet (models/AnyNet.py): pre-activation small-channel convolutions and the stage arithmetic
 * ---------------------------------------------------------------------------------------- */

#define DMB_PREACT_MAX_CI 64
#define DMB_PREACT_MAX_CO 32
#define DMB_PREACT_POOL 0x1     /* 2x2/2 max-pool of the input first (2-D; odd sizes floor, nn.MaxPool2d(2, 2)) */
#define DMB_PREACT_RELU_IN 0x2  /* ReLU on the (pooled, scaled) input: bn_relu_conv's ReLU */
#define DMB_PREACT_RELU_OUT 0x4 /* ReLU after the epilogue affine: conv_bn_relu's ReLU */
#define DMB_PREACT_GATE 0x8     /* gate normalisation of a 3P-channel output (disp_refinement/AnyNet.py:75-78) */

/* Direct 3x3 (ndim 2) / 3x3x3 (ndim 3) convolution, padding 1, dilation 1, stride 1 or 2 (2-D only), on 1 .. 64 input and
 * 1 .. 32 output channels: bn_relu_conv / bn_relu_conv3d (layers/basic_layers.py:122-138,180-197), conv_bn_relu
 * (:102-119) and plain nn.Conv2d.  w: the nn weight [Co, Ci, (3,) 3, 3] as it is.
 *   prologue, per staged input element and only inside the image (padding stays 0): [max-pool] -> [x * pre_scale[c] +
 *     pre_shift[c]] (both or neither: the folded eval-mode BatchNorm) -> [ReLU (DMB_PREACT_RELU_IN)];
 *   each output: ONE ascending (ci, kz, ky, kx) fmaf chain from 0 -- independent of the launch size, so batch item i equals the
 *     same item run alone bit for bit;
 *   epilogue: [acc * post_scale[co] + post_shift[co] | acc + post_shift[co] (post_scale NULL: a bias)] -> [ReLU] ->
 *     [relu(. + residual)] (residual [B, Co, Ho, Wo], disp_refinement/AnyNet.py:90);
 *   DMB_PREACT_GATE: Co = 3P; y, y2, y3 receive G_k / ((|G1| + |G2|) + |G3| + 1e-8) as three [B, P, Ho, Wo] tensors
 *     (out_channels_total = P, out_ch_offset = 0); otherwise y2, y3 are unused.
 * x (the tensor's base): channels [in_ch_offset, in_ch_offset + Ci) of [B, in_channels_total, D, H, W] (D = 1 for 2-D) are
 * read; items [B2, B) come from x2 (same layout, item 0 = item B2) when x2 is not NULL: both views of a pair in one launch.
 * y (the tensor's base): channels [out_ch_offset, out_ch_offset + Co) of [B, out_channels_total, D, Ho, Wo] are written,
 * Ho = (H' - 1) / stride + 1 with H' = H / 2 when pooling, else H. */
int dmb_preact_conv_f32(const float* x, const float* x2, int B2, const float* w, const float* pre_scale, const float* pre_shift,
                        const float* post_scale, const float* post_shift, const float* residual, float* y, float* y2, float* y3,
                        int B, int Ci, int Co, int D, int H, int W, int ndim, int stride, int flags, int in_channels_total,
                        int in_ch_offset, int out_channels_total, int out_ch_offset, void* stream);

/* The up-sampled coarse disparity of a warp stage (models/AnyNet.py:84,103 = cost_processors/AnyNet.py:64-70):
 * up = F.interpolate(low * scale, (H, W), bilinear, align_corners=False), low [B, 1, h, w] -> up [B, 1, H, W]; and, when
 * samples is not NULL, samples [B, D, H, W] = lin[k] + up (lin: DEVICE [D], the stage's linspace). */
int dmb_anynet_stage_samples_f32(const float* low, const float* lin, float* up, float* samples, int B, int h, int w, int H,
                                 int W, int D, float scale, void* stream);

/* c = a + b over n elements (models/AnyNet.py:85,104: up_low_d + high_d). */
int dmb_add_f32(const float* a, const float* b, float* c, long long n, void* stream);

/* The final maps (models/AnyNet.py:117-118,137-140): d0 .. d3 [B, 1, h_k, w_k] -> out [7, B, 1, H, W]:
 * out[k] = F.interpolate((d_k * W) / w_k, (H, W), bilinear, align_corners=False) for k < 4, out[3 + k] = out[k - 1] - out[k]. */
int dmb_anynet_final_maps_f32(const float* d0, const float* d1, const float* d2, const float* d3, const int* h_host,
                              const int* w_host, float* out, int B, int H, int W, void* stream);

/* ------------------------------------------------------------------------------------------
 * DeepPruner's disparity sampler (disp_samplers/DeepPruner.py, disp_samplers/utils/patch_match.py), forward and backward
 * ---------------------------------------------------------------------------------------- */

#define DMB_PATCH_MATCH_MAX_SAMPLES 85 /* intervals P of one PatchMatch step: 3P planes <= DMB_MAX_DISP_SAMPLES */

/* One propagate + evaluate half-iteration of differentiable PatchMatch with a propagation filter of size 3
 * (patch_match.py:119-174, 218-253, 329-356).  Per pair b, interval p < P and pixel:
 *   n_j   = noise_in[b, p] at x-1, x, x+1 (vertical == 0) or y-1, y, y+1 (vertical != 0); 0 outside the image
 *   s_j   = (max - min) * (float)(1 / (P + 1)) * n_j + (min + (max - min) * ((float)(p + 1) / (float)(P + 1)))
 *   c_j   = mean_c(L[b, c] * T_j[c]) * temperature,  T_j = the warp of dmb_fast_cat_fms_f32 at sample s_j on plane
 *           k = 3p + j of a volume of D = 3P planes (so the first and last plane keep half their weight)
 *   prob  = softmax_j(c_j);  sample = sum_j prob_j * s_j;  noise = sum_j prob_j * n_j
 * L, R: [B, C, H, W];  noise_in: [B, P, H, W];  min_disp, max_disp: [B, 1, H, W], or both NULL: the constants min_const,
 * max_const on every pixel (the "pre" stage's full range).  noise_out: [B, P, H, W] or NULL, never noise_in (neighbours
 * read the previous half-iteration).  out: NULL, or the base of [B, out_channels_total, H, W] whose channels
 * [out_ch_offset, out_ch_offset + P) receive the samples; write_ends != 0: channel out_ch_offset - 1 receives min and
 * channel out_ch_offset + P receives max (patch_match.py:359 without the concatenation).
 * The sampler's arithmetic is the reference's FP32 operation for operation; the channel sum is four interleaved ascending
 * chains, the same for any B and launch size.  1 <= P <= DMB_PATCH_MATCH_MAX_SAMPLES, any C >= 1, H, W >= 2:
 * DMB_EUNSUPPORTED otherwise. */
int dmb_patch_match_step_f32(const float* L, const float* R, const float* noise_in, const float* min_disp,
                             const float* max_disp, float min_const, float max_const, float* noise_out, float* out, int B,
                             int C, int P, int H, int W, int vertical, float temperature, int out_channels_total,
                             int out_ch_offset, int write_ends, void* stream);

/* DeepPruner.py:99-115 (UniformSampler): out [B, N, H, W], out[:, 0] = min, out[:, N - 1] = max,
 * out[:, k] = min + (max - min) * ((float)k / (float)(N - 1)); range_head != 0: preceded by DeepPruner.py:48-66, stage
 * "post" -- order the two maps, stretch ranges narrower than N by their shortfall, halve, clamp to [0, max_disp_limit].
 * Elementwise FP32 in the reference's order of operations: bit-exact.  2 <= N <= DMB_MAX_DISP_SAMPLES. */
int dmb_deeppruner_uniform_samples_f32(const float* min_disp, const float* max_disp, float* out, int B, int H, int W, int N,
                                       int range_head, float max_disp_limit, void* stream);

#define DMB_PATCH_MATCH_BWD_MAX_W 1024 /* columns of dmb_patch_match_step_bwd_f32: 8 channel rows of W floats in LDS (32 KiB) */

/* Backward of dmb_patch_match_step_f32 for the same L, R, noise_in, range and vertical.  With prob, s_j, n_j, T_j as there,
 * gS = g_samples (the gradient of the samples: channels [gs_ch_offset, gs_ch_offset + P) of [B, gs_channels_total, H, W]),
 * gN = g_noise (the gradient of noise_out, [B, P, H, W]); either may be NULL (= 0), not both; tc = temperature / C:
 *   a_j   = gS * s_j + gN * n_j;  gc_j = prob_j * (a_j - sum_j prob_j * a_j)
 *   dL[b, c, i] = dL_acc + tc * sum over p, j of gc_j * T_j[c]                 (ascending plane 3p + j: the same bits for any B)
 *   dR          = dR_acc + the sampler's adjoint of tc * gc_j * L[b, c, i] on plane 3p + j: the forward's taps and weights,
 *                 zero padding, half weight on the first and last plane (row sums in LDS in the hardware's order, then the
 *                 partial rows of a source row in ascending y, as dmb_fast_fms_bwd_f32)
 *   gs_j  = prob_j * gS + tc * gc_j * sum_c L[b, c, i] * dT_j[c] / ds,  dT / ds = the sampler's column derivative times
 *           -W / (W - 1) as dmb_fast_fms_bwd_f32 takes it for d_samples; taps outside the image count 0
 *   d_noise_in[b, p, i] = gn_1 at i + gn_0 at the next pixel + gn_2 at the previous one (along x, or y if vertical), in this
 *           order, gn_j = prob_j * gN + (max - min) * (float)(1 / (P + 1)) * gs_j: the same bits from run to run and for any B
 * The candidates, taps and costs are recomputed by the forward's own device functions (the cell floor(ix) of a candidate is the
 * forward's).  The range maps are constants: they receive no gradient.  dL_acc, dR_acc: [B, C, H, W] or NULL (= 0); each may be
 * the output it is added into.  dL, dR: [B, C, H, W]; d_noise_in: [B, P, H, W]; every element is written once.
 * workspace: 6 * B * P * H * W + 2 * B * C * H * W floats (gc, gn, the partial rows), left undefined.
 * The forward's range of sizes and W <= DMB_PATCH_MATCH_BWD_MAX_W: DMB_EUNSUPPORTED otherwise; operands 4-byte aligned. */
int dmb_patch_match_step_bwd_f32(const float* L, const float* R, const float* noise_in, const float* min_disp,
                                 const float* max_disp, float min_const, float max_const, const float* g_samples,
                                 const float* g_noise, const float* dL_acc, const float* dR_acc, float* dL, float* dR,
                                 float* d_noise_in, float* workspace, int B, int C, int P, int H, int W, int vertical,
                                 float temperature, int gs_channels_total, int gs_ch_offset, void* stream);

/* Backward of dmb_deeppruner_uniform_samples_f32: d_out [B, N, H, W] -> d_min, d_max [B, 1, H, W], every element written once.
 * d min = sum_k d_out_k * (1 - f_k), d max = sum_k d_out_k * f_k, f_k = (float)k / (float)(N - 1), ascending k; range_head != 0:
 * then through the clamps, the halving, the shortfall and the ordering of DeepPruner.py:48-66 with torch's subgradients
 * (minimum / maximum split a tie in halves, clamp passes the gradient at its bounds).  min_disp, max_disp: the forward's inputs,
 * read only when range_head != 0. */
int dmb_deeppruner_uniform_samples_bwd_f32(const float* min_disp, const float* max_disp, const float* d_out, float* d_min,
                                           float* d_max, int B, int H, int W, int N, int range_head, float max_disp_limit,
                                           void* stream);

/* ------------------------------------------------------------------------------------------
 * DeepPruner's cost processor (cost_processors/DeepPruner.py), forward only: csrc/deeppruner_heads.hip
 * ---------------------------------------------------------------------------------------- */

/* The raw cost volume of DeepPruner.py:192-195,204-208 in one pass; every element of out is written exactly once.
 * L, R: [B, C, H, W];  sample: [B, D, H, W];  out: [B, 2C + 1 + 2P, D, H, W]:
 *   channels [0, 2C)            what dmb_fast_cat_fms_f32(per_pixel = 1) writes: L * (T > 0) and T, T = R warped by -sample
 *   channel  2C                 sample[b, k, y, x]
 *   channels [2C + 1, +P)       min_feat[b, p, y, x] on every plane k            (min_feat, max_feat: [B, P, H, W])
 *   the next P                  max_feat[b, p, y, x] on every plane k
 * P == 0 with min_feat == max_feat == NULL: stage "pre", 2C + 1 channels.  The sampler arithmetic is warp_taps.h's, the rest
 * are copies: bit-identical to the composition.  Any C >= 1; D, H, W >= 2 and P <= DMB_PATCH_MATCH_MAX_SAMPLES
 * (DMB_EUNSUPPORTED otherwise); operands 4-byte aligned. */
int dmb_deeppruner_volume_f32(const float* L, const float* R, const float* sample, const float* min_feat, const float* max_feat,
                              float* out, int B, int C, int D, int H, int W, int P, void* stream);

#define DMB_CONV2D_K5_MAX_C 16

/* nn.Conv2d(Ci, Co, 5, stride 1, padding 2) on 1 .. DMB_CONV2D_K5_MAX_C input and output channels (DMB_EUNSUPPORTED otherwise).
 * x: [B, Ci, H, W];  w: the nn weight [Co, Ci, 5, 5] as it is;  y: [B, Co, H, W];  any H, W >= 1; operands 4-byte aligned.
 *   each output: ONE ascending (ci, ky, kx) fmaf chain from 0 -- independent of the launch size, so batch item i equals the
 *     same item run alone bit for bit;
 *   epilogue: acc * scale[co] + shift[co] | acc + shift[co] (scale NULL: a bias) | acc (both NULL), then ReLU if relu != 0. */
int dmb_conv2d_k5_small_f32(const float* x, const float* w, const float* scale, const float* shift, float* y, int B, int Ci,
                            int Co, int H, int W, int relu, void* stream);

#define DMB_REFINE_HEAD_MAX_C 16

/* The tail of a DeepPruner refinement stage (disp_refinement/DeepPruner.py:36,40-42,87) in one launch:
 *   y[B, 1, 2H, 2W] = up2(2 * relu(conv3x3(x[B, Ci, H, W], w[1, Ci, 3, 3]) + init[B, 1, H, W]))
 * a 3x3 convolution to one channel (no bias, padding 1), the residual add, the ReLU, the doubling and the half-pixel bilinear
 * up-sampling by two (F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)).
 * 1 <= Ci <= DMB_REFINE_HEAD_MAX_C (DMB_EUNSUPPORTED otherwise);  w: the nn weight as it is;  any H, W >= 1; operands 4-byte
 * aligned; a batch item of x and of y below 2 GiB.
 *   each refined value: ONE ascending (ci, ky, kx) fmaf chain from 0, then + init, max(., 0) -- independent of the launch size, so
 *     batch item i equals the same item run alone bit for bit;
 *   the interpolation is dmb_bilinear_scale_f32's with mult = 2, bit for bit; each output element is written once. */
int dmb_refine_head_up2_f32(const float* x, const float* w, const float* init, float* y, int B, int Ci, int H, int W, void* stream);

/* The output tail of the DeepPruner model (models/DeepPruner.py:82-94,115) in one launch.  With
 *   up(d) = F.interpolate((d * W) / w_d, (H, W), mode='bilinear', align_corners=False)
 * -- the multiply and the IEEE division are two FP32 roundings applied to each tap before the blend, which is
 * dmb_bilinear_scale_f32's with mult = 1 -- and d0 .. d{K-1}: [B, 1, h_host[k], w_host[k]] the refinement's list (better first, the
 * last one the cost processor's own disparity), min_disp, max_disp: [B, 1, h, w], out: [K + 4, B, 1, H, W]:
 *   out[k] = up(d_k), k < K;  D = out[K - 1], Mn = up(min_disp), Mx = up(max_disp)
 *   out[K] = (Mn * W) / W,  out[K + 1] = (Mx * W) / W      (the reference interpolates the full-size maps a second time)
 *   out[K + 2] = |D - Mn|,  out[K + 3] = |Mx - D|          (from the un-rescaled Mn and Mx)
 * bit-identical to the composition of dmb_bilinear_scale_f32 and elementwise launches; each element of out is written once.
 * 1 <= K <= 3 (DMB_EUNSUPPORTED otherwise; d_k with k >= K is not read and may be NULL); every extent >= 1; operands 4-byte
 * aligned; a batch item of every map below 2 GiB (DMB_EUNSUPPORTED otherwise).  Nothing depends on the launch size: batch item i
 * equals the same item run alone bit for bit. */
int dmb_deeppruner_final_maps_f32(const float* d0, const float* d1, const float* d2, const int* h_host, const int* w_host,
                                  const float* min_disp, const float* max_disp, float* out, int K, int B, int h, int w, int H,
                                  int W, void* stream);

/* Doubles of workspace the four loss entry points below use at most (a fixed number of blocks strides over the maps). */
#define DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES 9216

/* The training losses of the DeepPruner model (models/DeepPruner.py:82-108) on the maps as the model holds them, one launch plus
 * the finalising block; no full-size tensor is written.  With up(), d0 .. d{K-1}, min_disp, max_disp as for
 * dmb_deeppruner_final_maps_f32, gt: [B, 1, H, W], Mn = up(min_disp), Mx = up(max_disp) -- bit for bit that entry point's maps:
 *   loss_out[k]     = mean smooth_l1(up(d_k) - gt), k < K            over l1_lower < gt < l1_upper; 0 where no pixel is valid
 *   loss_out[K]     = mean smooth_l1((Mn * W) / W - gt),  loss_out[K + 1] the same of Mx
 *   loss_out[K + 2] = mean (gt - Mn) * (theta - [gt - Mn < 0])        over q_lower < gt < q_upper; NaN where no pixel is valid
 *   loss_out[K + 3] = mean (gt - Mx) * ((1 - theta) - [gt - Mx < 0])  (losses/utils/quantile_loss.py:25-37; 1 - theta in FP64)
 * Per-pixel terms FP32, sums FP64 in a fixed order (identical from run to run), no atomics.  stats: 2 doubles, the two counts,
 * for the backward pass.  workspace: DMB_DEEPPRUNER_LOSS_WORKSPACE_DOUBLES doubles, need not be initialised.
 * 1 <= K <= 3 and a batch item of every map below 2 GiB (DMB_EUNSUPPORTED otherwise); 0 < theta < 1; operands 4-byte aligned. */
int dmb_deeppruner_loss_fwd_f32(const float* d0, const float* d1, const float* d2, const int* h_host, const int* w_host,
                                const float* min_disp, const float* max_disp, const float* gt, double* workspace, float* loss_out,
                                double* stats, int K, int B, int h, int w, int H, int W, float l1_lower, float l1_upper,
                                float q_lower, float q_upper, double theta, void* stream);

/* Backward of the above in one launch: grad_out is a DEVICE pointer to the K + 4 weights of loss_out (no host read), stats the
 * forward's.  grad_d0 .. grad_d{K-1}, grad_min, grad_max have the shapes of the maps; each element is written exactly once (a
 * gather over the full-size pixels whose taps include it, FP64 accumulation in a fixed order: identical from run to run).
 * grad_min and grad_max collect the smooth-L1 term and the quantile term.  An empty mask gives zero gradients. */
int dmb_deeppruner_loss_bwd_f32(const float* d0, const float* d1, const float* d2, const int* h_host, const int* w_host,
                                const float* min_disp, const float* max_disp, const float* gt, const double* stats,
                                const float* grad_out, float* grad_d0, float* grad_d1, float* grad_d2, float* grad_min,
                                float* grad_max, int K, int B, int h, int w, int H, int W, float l1_lower, float l1_upper,
                                float q_lower, float q_upper, double theta, void* stream);

/* The two quantile terms alone on maps already at the ground truth's size (no rescaling: (d * W) / W is not the identity in FP32).
 * min_disp, max_disp, gt: [B, 1, H, W];  loss_out[0], loss_out[1]: the means of the two terms as above;  stats, workspace as above. */
int dmb_quantile_loss_fwd_f32(const float* min_disp, const float* max_disp, const float* gt, double* workspace, float* loss_out,
                              double* stats, int B, int H, int W, float q_lower, float q_upper, double theta, void* stream);

/* Backward of the above: grad_out is a device pointer to 2 floats; grad_min, grad_max: [B, 1, H, W], every element written once. */
int dmb_quantile_loss_bwd_f32(const float* min_disp, const float* max_disp, const float* gt, const double* stats,
                              const float* grad_out, float* grad_min, float* grad_max, int B, int H, int W, float q_lower,
                              float q_upper, double theta, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMB_HIP_H */
