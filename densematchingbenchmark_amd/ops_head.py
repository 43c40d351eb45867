"""Launching wrappers of the fused classifier tail (csrc/conv3d_s1s2.hip: conv3d_s1_kernel on S1HeadCfg + conv3d_head_finish_kernel).
They live next to ``ops`` and not in it, like ``ops_deeppruner``: ``ops``'s public launching functions are an enumerated set with
their memory-contract cases in tests/test_memory_contract_gpu.py; these have theirs in tests/test_memory_contract_head_gpu.py.
No fallback."""
import torch

from . import _lib, ops
from ._lib import launch, opt
from .ops import _affine_ok, _f32c, _relu_mode, _same_shape


# The 32 -> 32 classifier convolution with the 32 -> 1 head inside its launch (include/dmb_hip.h: dmb_conv3d_k3_head_f32): the
# 32-channel tensor between them is never written.  Reproducible run to run, but its sum order (per tap a chain over channels,
# then taps, then tiles) is not the single chain of conv3d_k3 + conv3d_k3_c1: the last bits differ.  Same policy as split-K --
# on by default, and ``set_split_k(False)`` keeps the two separate launches.
def pack_conv3d_head_weights(w):
    """HeadConv3d weight [1, 32, 3, 3, 3] -> the 16 MFMA A fragments of the fused head."""
    w = _f32c(w, "weight")
    if tuple(w.shape) != (1, 32, 3, 3, 3):
        raise _lib.DmbLibraryError("pack_conv3d_head_weights: weight must be [1, 32, 3, 3, 3], got %s" % (tuple(w.shape),))
    wp = torch.empty((_lib.CONV3D_HEAD_PACKED_FLOATS,), dtype=torch.float32, device=w.device)
    launch("dmb_conv3d_head_pack_weights_f32", w, wp)
    return wp


def conv3d_k3_head_applicable(x):
    """Whether a 32 -> 32 launch on ``x`` [B, Ci, D, H, W] would take the tile the fused head is built for."""
    if x.dim() != 5 or x.dtype != torch.float32 or x.device.type != "cuda" or not ops.split_k() or ops.conv3d_mode() != "exact":
        return False
    B, _, D, H, W = x.shape
    return x.data_ptr() % 16 == 0 and _lib.load().dmb_conv3d_k3_head_preferred(B, D, H, W) == 1


def conv3d_k3_head(x, wpack, head_wpack, scale=None, shift=None, bias=0.0, residual=None, relu=True):
    """conv3d_k3_c1(act(scale * conv3d_k3(x) + shift), w_head) + bias (+ residual): [B, Ci, D, H, W] -> [B, 1, D, H, W]."""
    tag = "conv3d_k3_head_%dto32to1" % x.shape[1]
    sh = _lib.shim()
    if sh is not None:
        if ops._kernel_timer is not None:
            ops._kernel_timer.start(tag)
        y = sh.conv3d_k3_head(x if x.is_contiguous() else x.contiguous(), wpack, scale, shift, head_wpack, float(bias), residual,
                              _relu_mode(relu) | ops._conv_flags())
        if ops._kernel_timer is not None:
            ops._kernel_timer.stop(tag)
        return y
    lib = _lib.load()
    x = _f32c(x, "x")
    B, Ci, D, H, W = x.shape
    _affine_ok(scale, shift, 32, "conv3d_k3_head")
    if wpack.numel() != lib.dmb_conv3d_packed_floats(32, Ci) or head_wpack.numel() != _lib.CONV3D_HEAD_PACKED_FLOATS:
        raise _lib.DmbLibraryError("conv3d_k3_head: packed weights do not belong to %d -> 32 -> 1 channels" % Ci)
    wsf = lib.dmb_conv3d_k3_head_workspace_floats(B, D, H, W)
    if wsf <= 0:
        raise _lib.DmbLibraryError("conv3d_k3_head: shape %s does not take the fused form (use conv3d_k3 + conv3d_k3_c1)" % (tuple(x.shape),))
    y = torch.empty((B, 1, D, H, W), dtype=torch.float32, device=x.device)
    if residual is not None:
        _same_shape(residual, y, "conv3d_k3_head residual")
    ws = torch.empty((wsf,), dtype=torch.float32, device=x.device)
    if ops._kernel_timer is not None:
        ops._kernel_timer.start(tag)
    launch("dmb_conv3d_k3_head_f32", x, wpack, opt(scale), opt(shift), head_wpack, bias, opt(residual), y, ws, B, Ci, D, H, W,
           _relu_mode(relu) | ops._conv_flags())
    if ops._kernel_timer is not None:
        ops._kernel_timer.stop(tag)
    return y
