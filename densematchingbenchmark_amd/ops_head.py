"""Launching wrappers of the fused classifier tail (csrc/conv3d_s1s2.hip: conv3d_s1_kernel on S1HeadCfg + conv3d_head_chain_finish_kernel).
They live next to ``ops`` and not in it, like ``ops_deeppruner``: ``ops``'s public launching functions are an enumerated set with
their memory-contract cases in tests/test_memory_contract_gpu.py; these have theirs in tests/test_memory_contract_head_gpu.py and
tests/test_memory_contract_head_chain_gpu.py.
No fallback."""
import ctypes

import torch

from . import _lib, ops
from ._lib import dev_ptr, launch, opt
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


# The two halves of conv3d_k3_head as calls of their own (dmb_conv3d_k3_head_partial_f32 / dmb_conv3d_head_chain_finish_f32): a
# chain of classifier tails whose costs accumulate (PSMNet.py:70-72) runs its convolutions into one workspace each and ONE
# finishing pass that keeps the running cost in registers -- bit for bit the chained conv3d_k3_head calls.
def conv3d_k3_head_partial(x, wpack, head_wpack, scale=None, shift=None, relu=True):
    """The convolution launch of conv3d_k3_head alone: returns the workspace holding the head's partial sums per tile."""
    tag = "conv3d_k3_head_%dto32to1" % x.shape[1]
    sh = _lib.shim()
    if sh is not None:
        if ops._kernel_timer is not None:
            ops._kernel_timer.start(tag)
        ws = sh.conv3d_k3_head_partial(x if x.is_contiguous() else x.contiguous(), wpack, scale, shift, head_wpack,
                                       _relu_mode(relu) | ops._conv_flags())
        if ops._kernel_timer is not None:
            ops._kernel_timer.stop(tag)
        return ws
    lib = _lib.load()
    x = _f32c(x, "x")
    B, Ci, D, H, W = x.shape
    _affine_ok(scale, shift, 32, "conv3d_k3_head_partial")
    if wpack.numel() != lib.dmb_conv3d_packed_floats(32, Ci) or head_wpack.numel() != _lib.CONV3D_HEAD_PACKED_FLOATS:
        raise _lib.DmbLibraryError("conv3d_k3_head_partial: packed weights do not belong to %d -> 32 -> 1 channels" % Ci)
    wsf = lib.dmb_conv3d_k3_head_workspace_floats(B, D, H, W)
    if wsf <= 0:
        raise _lib.DmbLibraryError("conv3d_k3_head_partial: shape %s does not take the fused form (use conv3d_k3 + conv3d_k3_c1)" % (tuple(x.shape),))
    ws = torch.empty((wsf,), dtype=torch.float32, device=x.device)
    if ops._kernel_timer is not None:
        ops._kernel_timer.start(tag)
    launch("dmb_conv3d_k3_head_partial_f32", x, wpack, opt(scale), opt(shift), head_wpack, ws, B, Ci, D, H, W,
           _relu_mode(relu) | ops._conv_flags())
    if ops._kernel_timer is not None:
        ops._kernel_timer.stop(tag)
    return ws


def conv3d_head_chain_finish(workspaces, biases, shape, residual=None):
    """One finishing pass over the workspaces of N <= 4 conv3d_k3_head_partial calls on volumes of ``shape`` = (B, D, H, W):
    returns y [N, B, 1, D, H, W] with y[0] = finish(ws_0) + bias_0 (+ residual) and y[k] = (finish(ws_k) + bias_k) + y[k - 1]."""
    B, D, H, W = (int(v) for v in shape)
    n = len(workspaces)
    if n < 1 or n > 4 or len(biases) != n:
        raise _lib.DmbLibraryError("conv3d_head_chain_finish: 1 .. 4 workspaces and one bias per workspace")
    sh = _lib.shim()
    if sh is not None:
        return sh.conv3d_head_chain_finish(list(workspaces), [float(b) for b in biases], residual, B, D, H, W)
    wsf = _lib.load().dmb_conv3d_k3_head_workspace_floats(B, D, H, W)
    if wsf <= 0:
        raise _lib.DmbLibraryError("conv3d_head_chain_finish: shape %s does not take the fused form" % ((B, D, H, W),))
    for ws in workspaces:
        if _f32c(ws, "workspace").numel() != wsf:
            raise _lib.DmbLibraryError("conv3d_head_chain_finish: a workspace of %d floats does not belong to shape %s" % (ws.numel(), (B, D, H, W)))
    y = torch.empty((n, B, 1, D, H, W), dtype=torch.float32, device=workspaces[0].device)
    if residual is not None:
        _same_shape(residual, y[0], "conv3d_head_chain_finish residual")
    PA = ctypes.c_void_p * n
    launch("dmb_conv3d_head_chain_finish_f32", n, PA(*[dev_ptr(ws, "workspace").value for ws in workspaces]), biases, opt(residual),
           PA(*[dev_ptr(y[k], "y").value for k in range(n)]), B, D, H, W, device=y.device)
    return y
