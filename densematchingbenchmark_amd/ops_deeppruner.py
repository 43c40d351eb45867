"""Launching wrappers of csrc/deeppruner_heads.hip (DeepPruner's cost processor), csrc/refine_head.hip (the tail of its
refinement) and csrc/deeppruner_final_maps.hip (the model's output tail): thin, in the manner of ``ops.fast_cat_fms``.  They live next to ``ops`` and not in it: ``ops``'s public launching
functions are an enumerated set (each has its memory-contract cases in tests/test_memory_contract_gpu.py); the first two have
theirs in tests/test_memory_contract_deeppruner_gpu.py, ``refine_head_up2`` in tests/test_memory_contract_refine_gpu.py,
``deeppruner_final_maps`` in tests/test_memory_contract_deeppruner_model_gpu.py.
No fallback."""
import torch

from . import _lib
from .ops import _f32c, _feature_pair, _same_shape, check, dev_ptr, host_ints, stream_ptr

K5_MAX_C = 16                    # include/dmb_hip.h: DMB_CONV2D_K5_MAX_C
MAX_FEATURE_PLANES = 85          # include/dmb_hip.h: DMB_PATCH_MATCH_MAX_SAMPLES
REFINE_HEAD_MAX_C = 16           # include/dmb_hip.h: DMB_REFINE_HEAD_MAX_C
FINAL_MAPS_MAX_K = 3             # include/dmb_hip.h: dmb_deeppruner_final_maps_f32 takes 1 .. 3 list maps


def deeppruner_volume(left, right, disp_sample, min_feature=None, max_feature=None):
    """DeepPruner.py:192-195,204-208 in one launch: [B, C, H, W] x 2, samples [B, D, H, W] and, for stage "post", the two range
    feature maps [B, P, H, W] -> [B, 2C + 1 + 2P, D, H, W] = cat(fast_cat_fms(left, right, samples), samples, min_feature on every
    plane, max_feature on every plane), bit for bit, each element written once."""
    lib = _lib.load()
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
    check(lib.dmb_deeppruner_volume_f32(dev_ptr(left), dev_ptr(right), dev_ptr(ds), dev_ptr(min_feature, allow_none=True),
                                        dev_ptr(max_feature, allow_none=True), dev_ptr(out), B, C, D, H, W, P,
                                        stream_ptr(left.device)), "dmb_deeppruner_volume_f32")
    return out


def conv2d_k5_small(x, w, scale=None, shift=None, relu=False):
    """nn.Conv2d(Ci, Co, 5, stride 1, padding 2) on 1 .. 16 channels: x [B, Ci, H, W], w [Co, Ci, 5, 5] as it is -> [B, Co, H, W];
    epilogue acc * scale[co] + shift[co] (``scale`` None: acc + shift[co], a bias; both None: acc), then ReLU if ``relu``."""
    lib = _lib.load()
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
    check(lib.dmb_conv2d_k5_small_f32(dev_ptr(x), dev_ptr(w), dev_ptr(scale, allow_none=True), dev_ptr(shift, allow_none=True),
                                      dev_ptr(y), B, Ci, Co, H, W, 1 if relu else 0, stream_ptr(x.device)),
          "dmb_conv2d_k5_small_f32")
    return y


def refine_head_up2(x, w, init):
    """The tail of a DeepPruner refinement stage (disp_refinement/DeepPruner.py:36,40-42,87) in one launch: x [B, Ci, H, W]
    (1 <= Ci <= 16), w [1, Ci, 3, 3] as it is, init [B, 1, H, W] -> [B, 1, 2H, 2W] =
    F.interpolate(2 * relu(conv3x3(x, w, padding 1) + init), scale_factor 2, bilinear, align_corners=False)."""
    lib = _lib.load()
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
    check(lib.dmb_refine_head_up2_f32(dev_ptr(x), dev_ptr(w), dev_ptr(init), dev_ptr(y), B, Ci, H, W, stream_ptr(x.device)),
          "dmb_refine_head_up2_f32")
    return y


def deeppruner_final_maps(disps, min_disparity, max_disparity, size):
    """The output tail of the DeepPruner model (models/DeepPruner.py:82-94,115) in one launch: ``disps``, the refinement's list of
    K = 1 .. 3 maps [B, 1, h_k, w_k] (better first, the last one the processor's own disparity), and the two range maps
    [B, 1, h, w] brought to ``size`` = (H, W) as up(d) = F.interpolate((d * W) / w_d, size, bilinear, align_corners=False).
    Returns K + 4 contiguous [B, 1, H, W] views of one tensor: up(d_0) .. up(d_{K-1}) = D, (Mn * W) / W, (Mx * W) / W with
    Mn = up(min_disparity) and Mx = up(max_disparity), |D - Mn| and |Mx - D|."""
    lib = _lib.load()
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
    ptrs = [dev_ptr(d) for d in ds] + [None] * (FINAL_MAPS_MAX_K - K)
    check(lib.dmb_deeppruner_final_maps_f32(*ptrs, host_ints([d.shape[2] for d in ds]), host_ints([d.shape[3] for d in ds]),
                                            dev_ptr(lo), dev_ptr(hi), dev_ptr(out), K, B, lo.shape[2], lo.shape[3], H, W,
                                            stream_ptr(out.device)), "dmb_deeppruner_final_maps_f32")
    return list(out.unbind(0))
