"""Launching wrappers of csrc/deeppruner_heads.hip (DeepPruner's cost processor), csrc/refine_head.hip (the tail of its
refinement) and csrc/deeppruner_final_maps.hip (the model's output tail): thin, in the manner of ``ops.fast_cat_fms``.  They live next to ``ops`` and not in it: ``ops``'s public launching
functions are an enumerated set (each has its memory-contract cases in tests/test_memory_contract_gpu.py); the first two have
theirs in tests/test_memory_contract_deeppruner_gpu.py, ``refine_head_up2`` in tests/test_memory_contract_refine_gpu.py,
``deeppruner_final_maps`` in tests/test_memory_contract_deeppruner_model_gpu.py.  The four wrappers of csrc/deeppruner_loss.hip (the
model's training losses, forward and backward, and the elementwise quantile pair) have theirs in
tests/test_memory_contract_deeppruner_loss_gpu.py.
No fallback."""
import torch

from . import _lib
from ._lib import launch, opt
from .ops import _f32c, _feature_pair, _range_maps, _same_shape

K5_MAX_C = _lib.DEFINES["DMB_CONV2D_K5_MAX_C"]
MAX_FEATURE_PLANES = _lib.DEFINES["DMB_PATCH_MATCH_MAX_SAMPLES"]
REFINE_HEAD_MAX_C = _lib.DEFINES["DMB_REFINE_HEAD_MAX_C"]
FINAL_MAPS_MAX_K = 3             # include/dmb_hip.h: dmb_deeppruner_final_maps_f32 takes 1 .. 3 list maps


def _list_maps(maps):
    """The FINAL_MAPS_MAX_K pointer slots an entry point has for a list of 1 .. 3 maps: the maps, then NULLs."""
    return list(maps) + [_lib.NULL] * (FINAL_MAPS_MAX_K - len(maps))


def deeppruner_volume(left, right, disp_sample, min_feature=None, max_feature=None):
    """DeepPruner.py:192-195,204-208 in one launch: [B, C, H, W] x 2, samples [B, D, H, W] and, for stage "post", the two range
    feature maps [B, P, H, W] -> [B, 2C + 1 + 2P, D, H, W] = cat(fast_cat_fms(left, right, samples), samples, min_feature on every
    plane, max_feature on every plane), bit for bit, each element written once."""
    left, right = _feature_pair(left, right, "deeppruner_volume")
    B, C, H, W = left.shape
    ds = _f32c(disp_sample, "disp_sample")
    if ds.dim() != 4 or ds.shape[0] != B or tuple(ds.shape[2:]) != (H, W):
        raise _lib.DmbLibraryError("deeppruner_volume: disp_sample must be [B, D, H, W] matching the features, got %s" % (tuple(ds.shape),))
    D, P = ds.shape[1], 0
    if (min_feature is None) != (max_feature is None):
        raise _lib.DmbLibraryError("deeppruner_volume: min_feature and max_feature come together or not at all")
    if min_feature is not None:
        min_feature, max_feature = _f32c(min_feature, "min_feature"), _f32c(max_feature, "max_feature")
        _same_shape(min_feature, max_feature, "deeppruner_volume features")
        if min_feature.dim() != 4 or min_feature.shape[0] != B or tuple(min_feature.shape[2:]) != (H, W) or min_feature.shape[1] < 1:
            raise _lib.DmbLibraryError("deeppruner_volume: the range features must be [B, P, H, W] matching the image features, got %s"
                                       % (tuple(min_feature.shape),))
        P = min_feature.shape[1]
    out = torch.empty((B, 2 * C + 1 + 2 * P, D, H, W), dtype=torch.float32, device=left.device)
    launch("dmb_deeppruner_volume_f32", left, right, ds, opt(min_feature), opt(max_feature), out, B, C, D, H, W, P)
    return out


def conv2d_k5_small(x, w, scale=None, shift=None, relu=False):
    """nn.Conv2d(Ci, Co, 5, stride 1, padding 2) on 1 .. 16 channels: x [B, Ci, H, W], w [Co, Ci, 5, 5] as it is -> [B, Co, H, W];
    epilogue acc * scale[co] + shift[co] (``scale`` None: acc + shift[co], a bias; both None: acc), then ReLU if ``relu``."""
    x, w = _f32c(x, "x"), _f32c(w, "w")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape[1:]) != (x.shape[1], 5, 5):
        raise _lib.DmbLibraryError("conv2d_k5_small: x [B, Ci, H, W] and w [Co, Ci, 5, 5] expected, got %s and %s"
                                   % (tuple(x.shape), tuple(w.shape)))
    B, Ci, H, W = x.shape
    Co = w.shape[0]
    for t, n in ((scale, "scale"), (shift, "shift")):
        if t is not None and (t.dtype != torch.float32 or t.numel() != Co):
            raise _lib.DmbLibraryError("conv2d_k5_small: %s must hold %d float32 values" % (n, Co))
    scale = scale.contiguous() if scale is not None else None
    shift = shift.contiguous() if shift is not None else None
    y = torch.empty((B, Co, H, W), dtype=torch.float32, device=x.device)
    launch("dmb_conv2d_k5_small_f32", x, w, opt(scale), opt(shift), y, B, Ci, Co, H, W, 1 if relu else 0)
    return y


def refine_head_up2(x, w, init):
    """The tail of a DeepPruner refinement stage (disp_refinement/DeepPruner.py:36,40-42,87) in one launch: x [B, Ci, H, W]
    (1 <= Ci <= 16), w [1, Ci, 3, 3] as it is, init [B, 1, H, W] -> [B, 1, 2H, 2W] =
    F.interpolate(2 * relu(conv3x3(x, w, padding 1) + init), scale_factor 2, bilinear, align_corners=False)."""
    x, w, init = _f32c(x, "x"), _f32c(w, "w"), _f32c(init, "init")
    if x.dim() != 4 or w.dim() != 4 or tuple(w.shape) != (1, x.shape[1], 3, 3):
        raise _lib.DmbLibraryError("refine_head_up2: x [B, Ci, H, W] and w [1, Ci, 3, 3] expected, got %s and %s"
                                   % (tuple(x.shape), tuple(w.shape)))
    B, Ci, H, W = x.shape
    if Ci < 1 or Ci > REFINE_HEAD_MAX_C:
        raise _lib.DmbLibraryError("refine_head_up2: 1 .. %d input channels, got %d" % (REFINE_HEAD_MAX_C, Ci))
    if tuple(init.shape) != (B, 1, H, W):
        raise _lib.DmbLibraryError("refine_head_up2: init must be [B, 1, H, W] = %s, got %s" % ((B, 1, H, W), tuple(init.shape)))
    y = torch.empty((B, 1, 2 * H, 2 * W), dtype=torch.float32, device=x.device)
    launch("dmb_refine_head_up2_f32", x, w, init, y, B, Ci, H, W)
    return y


def deeppruner_final_maps(disps, min_disparity, max_disparity, size):
    """The output tail of the DeepPruner model (models/DeepPruner.py:82-94,115) in one launch: ``disps``, the refinement's list of
    K = 1 .. 3 maps [B, 1, h_k, w_k] (better first, the last one the processor's own disparity), and the two range maps
    [B, 1, h, w] brought to ``size`` = (H, W) as up(d) = F.interpolate((d * W) / w_d, size, bilinear, align_corners=False).
    Returns K + 4 contiguous [B, 1, H, W] views of one tensor: up(d_0) .. up(d_{K-1}) = D, (Mn * W) / W, (Mx * W) / W with
    Mn = up(min_disparity) and Mx = up(max_disparity), |D - Mn| and |Mx - D|."""
    ds = [_f32c(d, "disp") for d in disps]
    K = len(ds)
    if K < 1 or K > FINAL_MAPS_MAX_K:
        raise _lib.DmbLibraryError("deeppruner_final_maps: 1 .. %d maps in the list, got %d" % (FINAL_MAPS_MAX_K, K))
    lo, hi = _f32c(min_disparity, "min_disparity"), _f32c(max_disparity, "max_disparity")
    _same_shape(lo, hi, "deeppruner_final_maps range maps")
    B = ds[0].shape[0]
    if any(t.dim() != 4 or t.shape[0] != B or t.shape[1] != 1 or t.shape[2] < 1 or t.shape[3] < 1 for t in ds + [lo]):
        raise _lib.DmbLibraryError("deeppruner_final_maps: every map must be [B, 1, h, w] with one B, got %s"
                                   % ([tuple(t.shape) for t in ds + [lo]],))
    H, W = (int(v) for v in size)
    if H < 1 or W < 1:
        raise _lib.DmbLibraryError("deeppruner_final_maps: the output size must be positive, got %s" % ((H, W),))
    out = torch.empty((K + 4, B, 1, H, W), dtype=torch.float32, device=ds[0].device)
    launch("dmb_deeppruner_final_maps_f32", *_list_maps(ds), [d.shape[2] for d in ds], [d.shape[3] for d in ds], lo, hi, out, K, B,
           lo.shape[2], lo.shape[3], H, W)
    return list(out.unbind(0))


def _loss_operands(disps, min_disparity, max_disparity, gt, theta, what):
    ds = [_f32c(d, "disp") for d in disps]
    K = len(ds)
    if K < 1 or K > FINAL_MAPS_MAX_K:
        raise _lib.DmbLibraryError("%s: 1 .. %d maps in the list, got %d" % (what, FINAL_MAPS_MAX_K, K))
    lo, hi, gt = _f32c(min_disparity, "min_disparity"), _f32c(max_disparity, "max_disparity"), _f32c(gt, "gt")
    _same_shape(lo, hi, what + " range maps")
    if gt.dim() != 4 or gt.shape[1] != 1 or gt.shape[2] < 1 or gt.shape[3] < 1:
        raise _lib.DmbLibraryError("%s: the ground truth must be [B, 1, H, W], got %s" % (what, tuple(gt.shape)))
    B = gt.shape[0]
    if any(t.dim() != 4 or t.shape[0] != B or t.shape[1] != 1 or t.shape[2] < 1 or t.shape[3] < 1 for t in ds + [lo]):
        raise _lib.DmbLibraryError("%s: every map must be [B, 1, h, w] with the ground truth's B, got %s"
                                   % (what, [tuple(t.shape) for t in ds + [lo]]))
    if any(t.device != gt.device for t in ds + [lo, hi]):
        raise _lib.DmbLibraryError("%s: the maps and the ground truth live on different devices" % what)
    if not 0.0 < float(theta) < 1.0:
        raise _lib.DmbLibraryError("%s: theta must lie inside (0, 1), got %r" % (what, theta))
    return ds, lo, hi, gt


def deeppruner_loss_fwd(disps, min_disparity, max_disparity, gt, l1_lower, l1_upper, q_lower, q_upper, theta):
    """The training losses of the DeepPruner model (models/DeepPruner.py:82-108) in one launch plus the finalising block, on the
    maps as the model holds them: ``disps`` K = 1 .. 3 maps [B, 1, h_k, w_k], the two range maps [B, 1, h, w], ``gt`` [B, 1, H, W].
    Returns (``out`` [K + 4] float32, ``stats`` [2] float64): the K + 2 smooth-L1 means of up(d_k), (Mn * W) / W and (Mx * W) / W
    under l1_lower < gt < l1_upper (0 for an empty mask), the two quantile means of Mn and Mx under q_lower < gt < q_upper (NaN for
    an empty mask), and the two counts for ``deeppruner_loss_bwd``.  No full-size tensor is written."""
    ds, lo, hi, gt = _loss_operands(disps, min_disparity, max_disparity, gt, theta, "deeppruner_loss_fwd")
    K = len(ds)
    out = torch.empty((K + 4,), dtype=torch.float32, device=gt.device)
    stats = torch.empty((2,), dtype=torch.float64, device=gt.device)
    ws = torch.empty((_lib.DEEPPRUNER_LOSS_WORKSPACE_DOUBLES,), dtype=torch.float64, device=gt.device)
    launch("dmb_deeppruner_loss_fwd_f32", *_list_maps(ds), [d.shape[2] for d in ds], [d.shape[3] for d in ds], lo, hi, gt, ws, out, stats,
           K, gt.shape[0], lo.shape[2], lo.shape[3], gt.shape[2], gt.shape[3], l1_lower, l1_upper, q_lower, q_upper, theta)
    return out, stats


def _loss_stats(stats, grad_out, n, device, what):
    if stats.dtype != torch.float64 or stats.numel() != 2 or stats.device != device or not stats.is_contiguous():
        raise _lib.DmbLibraryError("%s: stats must be the forward's 2 float64 counts on the maps' device" % what)
    go = _f32c(grad_out, "grad_out")
    if go.numel() != n or go.device != device:
        raise _lib.DmbLibraryError("%s: grad_out must hold %d float32 values on the maps' device, got %s" % (what, n, tuple(go.shape)))
    return go


def deeppruner_loss_bwd(disps, min_disparity, max_disparity, gt, stats, grad_out, l1_lower, l1_upper, q_lower, q_upper, theta):
    """Backward of ``deeppruner_loss_fwd`` in one launch: ``grad_out`` [K + 4] on the device (never read on the host), ``stats`` the
    forward's.  Returns ([grad_d0 .. grad_d{K-1}], grad_min, grad_max) with the shapes of the maps, every element written once."""
    ds, lo, hi, gt = _loss_operands(disps, min_disparity, max_disparity, gt, theta, "deeppruner_loss_bwd")
    K = len(ds)
    go = _loss_stats(stats, grad_out, K + 4, gt.device, "deeppruner_loss_bwd")
    gds = [torch.empty(tuple(d.shape), dtype=torch.float32, device=gt.device) for d in ds]
    glo = torch.empty(tuple(lo.shape), dtype=torch.float32, device=gt.device)
    ghi = torch.empty(tuple(hi.shape), dtype=torch.float32, device=gt.device)
    launch("dmb_deeppruner_loss_bwd_f32", *_list_maps(ds), [d.shape[2] for d in ds], [d.shape[3] for d in ds], lo, hi, gt, stats, go,
           *_list_maps(gds), glo, ghi, K, gt.shape[0], lo.shape[2], lo.shape[3], gt.shape[2], gt.shape[3], l1_lower, l1_upper, q_lower,
           q_upper, theta)
    return gds, glo, ghi


def _quantile_operands(min_disparity, max_disparity, gt, theta, what):
    lo, hi, gt = _f32c(min_disparity, "minEstDisp"), _f32c(max_disparity, "maxEstDisp"), _f32c(gt, "gtDisp")
    _same_shape(lo, gt, what)
    _same_shape(hi, gt, what)
    if gt.dim() != 4 or gt.shape[1] != 1 or gt.numel() < 1:
        raise _lib.DmbLibraryError("%s: the maps must be [B, 1, H, W], got %s" % (what, tuple(gt.shape)))
    if lo.device != gt.device or hi.device != gt.device:
        raise _lib.DmbLibraryError("%s: the maps and the ground truth live on different devices" % what)
    if not 0.0 < float(theta) < 1.0:
        raise _lib.DmbLibraryError("%s: theta must lie inside (0, 1), got %r" % (what, theta))
    return lo, hi, gt


def quantile_loss_fwd(min_disparity, max_disparity, gt, q_lower, q_upper, theta):
    """The two terms of losses/utils/quantile_loss.py:25-37 on maps at the ground truth's size, [B, 1, H, W] each: returns
    (``out`` [2] float32 = the means of (gt - min) * (theta - [gt - min < 0]) and (gt - max) * ((1 - theta) - [gt - max < 0]) under
    q_lower < gt < q_upper, NaN for an empty mask; ``stats`` [2] float64 for ``quantile_loss_bwd``)."""
    lo, hi, gt = _quantile_operands(min_disparity, max_disparity, gt, theta, "quantile_loss_fwd")
    out = torch.empty((2,), dtype=torch.float32, device=gt.device)
    stats = torch.empty((2,), dtype=torch.float64, device=gt.device)
    ws = torch.empty((_lib.DEEPPRUNER_LOSS_WORKSPACE_DOUBLES,), dtype=torch.float64, device=gt.device)
    launch("dmb_quantile_loss_fwd_f32", lo, hi, gt, ws, out, stats, gt.shape[0], gt.shape[2], gt.shape[3], q_lower, q_upper, theta)
    return out, stats


def quantile_loss_bwd(min_disparity, max_disparity, gt, stats, grad_out, q_lower, q_upper, theta):
    """Backward of ``quantile_loss_fwd``: ``grad_out`` [2] on the device; returns (grad_min, grad_max), every element written once."""
    lo, hi, gt = _quantile_operands(min_disparity, max_disparity, gt, theta, "quantile_loss_bwd")
    go = _loss_stats(stats, grad_out, 2, gt.device, "quantile_loss_bwd")
    glo = torch.empty(tuple(gt.shape), dtype=torch.float32, device=gt.device)
    ghi = torch.empty(tuple(gt.shape), dtype=torch.float32, device=gt.device)
    launch("dmb_quantile_loss_bwd_f32", lo, hi, gt, stats, go, glo, ghi, gt.shape[0], gt.shape[2], gt.shape[3], q_lower, q_upper, theta)
    return glo, ghi


# ---------------------------------------------------------------------------------------------- the sampler's backward
# csrc/patch_match.hip; ``ops.patch_match_step_bwd`` and ``ops.deeppruner_uniform_samples_bwd`` resolve to these two (ops.__getattr__).
# Their memory-contract cases are in tests/test_memory_contract_deeppruner_sampler_bwd_gpu.py.
PATCH_MATCH_BWD_MAX_W = _lib.DEFINES["DMB_PATCH_MATCH_BWD_MAX_W"]


def patch_match_step_bwd(left, right, noise, min_disparity=None, max_disparity=None, grad_samples=None, grad_noise=None,
                         vertical=False, temperature=7.0, bounds=(0.0, 0.0), grad_left_acc=None, grad_right_acc=None):
    """Backward of ``ops.patch_match_step`` for the same ``left``, ``right``, ``noise`` (the step's INPUT noise), range and
    ``vertical``: returns (d left, d right, d noise), [B, C, H, W] x 2 and [B, P, H, W].  ``grad_samples``: the gradient of the
    step's samples, [B, P, H, W] or the [B, P + 2, H, W] of ``patch_match_step(out=)`` (channels 1 .. P are read);
    ``grad_noise``: the gradient of the step's new noise, [B, P, H, W]; either may be None (zero), not both.
    ``grad_left_acc`` / ``grad_right_acc``: [B, C, H, W] added into the two feature gradients (read, not modified).  The range
    maps are constants here: they get no gradient.  No host copy, no synchronisation."""
    left, right = _feature_pair(left, right, "patch_match_step_bwd")
    noise = _f32c(noise, "noise")
    B, C, H, W = left.shape
    if noise.dim() != 4 or noise.shape[0] != B or tuple(noise.shape[2:]) != (H, W):
        raise _lib.DmbLibraryError("patch_match_step_bwd: noise must be [%d, P, %d, %d], got %s" % (B, H, W, tuple(noise.shape)))
    P = noise.shape[1]
    if W > PATCH_MATCH_BWD_MAX_W:
        raise NotImplementedError("patch_match_step_bwd: feature maps wider than %d columns have no backward on the HIP path, got %d"
                                  % (PATCH_MATCH_BWD_MAX_W, W))
    if (min_disparity is None) != (max_disparity is None):
        raise _lib.DmbLibraryError("patch_match_step_bwd: give both range maps or neither")
    lo = hi = None
    if min_disparity is not None:
        lo, hi = _range_maps(min_disparity, max_disparity, B, H, W, "patch_match_step_bwd")
    if grad_samples is None and grad_noise is None:
        raise _lib.DmbLibraryError("patch_match_step_bwd: neither grad_samples nor grad_noise")
    ctot = coff = 0
    if grad_samples is not None:
        grad_samples = _f32c(grad_samples, "grad_samples")
        if tuple(grad_samples.shape) == (B, P, H, W):
            ctot, coff = P, 0
        elif tuple(grad_samples.shape) == (B, P + 2, H, W):
            ctot, coff = P + 2, 1
        else:
            raise _lib.DmbLibraryError("patch_match_step_bwd: grad_samples must be [%d, %d | %d, %d, %d], got %s"
                                       % (B, P, P + 2, H, W, tuple(grad_samples.shape)))
    if grad_noise is not None:
        grad_noise = _f32c(grad_noise, "grad_noise")
        _same_shape(grad_noise, noise, "patch_match_step_bwd grad_noise")
    for t, n in ((grad_left_acc, "grad_left_acc"), (grad_right_acc, "grad_right_acc")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (B, C, H, W)):
            raise _lib.DmbLibraryError("patch_match_step_bwd: %s must be a contiguous float32 [%d, %d, %d, %d]" % (n, B, C, H, W))
    dl = torch.empty((B, C, H, W), dtype=torch.float32, device=left.device)
    dr = torch.empty((B, C, H, W), dtype=torch.float32, device=left.device)
    dn = torch.empty((B, P, H, W), dtype=torch.float32, device=left.device)
    ws = torch.empty((6 * B * P * H * W + 2 * B * C * H * W,), dtype=torch.float32, device=left.device)
    launch("dmb_patch_match_step_bwd_f32", left, right, noise, opt(lo), opt(hi), bounds[0], bounds[1], opt(grad_samples),
           opt(grad_noise), opt(grad_left_acc), opt(grad_right_acc), dl, dr, dn, ws, B, C, P, H, W, int(bool(vertical)), temperature,
           ctot, coff)
    return dl, dr, dn


def deeppruner_uniform_samples_bwd(min_disparity, max_disparity, grad_out, max_disp=None):
    """Backward of ``ops.deeppruner_uniform_samples``: ``grad_out`` [B, N, H, W] -> (d min_disparity, d max_disparity),
    [B, 1, H, W] each, through the uniform sampler and -- with ``max_disp`` -- the range head, with torch's subgradients at ties
    and clamp edges.  One launch, every element written once."""
    lo = _f32c(min_disparity, "min_disparity")
    if lo.dim() != 4 or lo.shape[1] != 1:
        raise _lib.DmbLibraryError("deeppruner_uniform_samples_bwd: min_disparity must be [B, 1, H, W], got %s" % (tuple(lo.shape),))
    B, _, H, W = lo.shape
    lo, hi = _range_maps(lo, max_disparity, B, H, W, "deeppruner_uniform_samples_bwd")
    go = _f32c(grad_out, "grad_out")
    if go.dim() != 4 or go.shape[0] != B or tuple(go.shape[2:]) != (H, W):
        raise _lib.DmbLibraryError("deeppruner_uniform_samples_bwd: grad_out must be [%d, N, %d, %d], got %s" % (B, H, W, tuple(go.shape)))
    glo = torch.empty((B, 1, H, W), dtype=torch.float32, device=lo.device)
    ghi = torch.empty((B, 1, H, W), dtype=torch.float32, device=lo.device)
    launch("dmb_deeppruner_uniform_samples_bwd_f32", lo, hi, go, glo, ghi, B, H, W, go.shape[1], max_disp is not None,
           max_disp if max_disp is not None else 0.0)
    return glo, ghi
