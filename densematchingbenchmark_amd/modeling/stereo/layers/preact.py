"""AnyNet's small-channel units on csrc/preact_conv.hip: ``bn_relu_conv`` / ``bn_relu_conv3d`` (layers/basic_layers.py:122-138,
180-197: BatchNorm -> ReLU -> Conv, the BatchNorm on the conv's INPUT) and the small ``conv_bn_relu`` of AnyNet's refinement
(:102-119).  Same Sequential keys as the reference (``0.*`` BatchNorm, ``2.*`` conv; ``1.*`` conv without BatchNorm); each forward
is ONE launch of dmb_preact_conv_f32 with the eval-mode BatchNorm folded (fold_batch_norm).  Inference only: training mode, or a
call where anything can receive a gradient, raises NotImplementedError."""
import torch
import torch.nn as nn

from .... import ops, param_state
from .basic_layers import bn_parts, fold_batch_norm

__all__ = ["PreActConv", "SmallConvBnRelu", "bn_relu_conv", "bn_relu_conv3d", "refuse_grad", "check_preact_shape"]


def refuse_grad(module, *tensors):
    """AnyNet runs inference only (its backward is not built): never return a silently detached result."""
    if module.training:
        raise NotImplementedError("%s: AnyNet on the HIP path is inference only; call eval()" % type(module).__name__)
    if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in tensors)
                                    or any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError("%s: AnyNet on the HIP path has no backward; run it under torch.no_grad() (as init_model / "
                                  "inference_stereo do)" % type(module).__name__)


def check_preact_shape(in_planes, out_planes, kernel_size, stride, padding, dilation, ndim):
    if kernel_size != 3 or padding != 1 or dilation != 1 or stride not in ((1, 2) if ndim == 2 else (1,)):
        raise NotImplementedError("HIP pre-activation conv: kernel 3, padding 1, dilation 1, stride 1 (or 2 in 2-D) only")
    if in_planes > ops.PREACT_MAX_CI or out_planes > ops.PREACT_MAX_CO:
        raise NotImplementedError("HIP pre-activation conv: at most %d input and %d output channels, got %d -> %d"
                                  % (ops.PREACT_MAX_CI, ops.PREACT_MAX_CO, in_planes, out_planes))


class PreActConv(nn.Sequential):
    """Sequential([BatchNorm2d|3d], ReLU, Conv2d|3d) as one launch: conv(relu(bn(x))) with the folded BatchNorm applied to each
    staged input element (padding stays 0).  ``run`` adds the backbone's fusions: a 2x2/2 max-pool of the input first, an input
    channel window, a second view and an output channel window."""

    def __init__(self, batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True, ndim=2,
                 bn_kwargs=None):
        check_preact_shape(in_planes, out_planes, kernel_size, stride, padding, dilation, ndim)
        BN, Conv = (nn.BatchNorm2d, nn.Conv2d) if ndim == 2 else (nn.BatchNorm3d, nn.Conv3d)
        conv = Conv(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation, bias=bias)
        mods = [BN(in_planes, **(bn_kwargs or {}))] if batch_norm else []
        super().__init__(*(mods + [nn.ReLU(inplace=True), conv]))
        self.has_bn, self.stride = bool(batch_norm), stride
        if batch_norm and not self[0].track_running_stats:
            fold_batch_norm(self[0], None, in_planes, None)     # raises: no folded form without running statistics

    @property
    def conv(self):
        return self[-1]

    def _folded(self):
        bn, conv = (self[0] if self.has_bn else None), self.conv
        return param_state.cached(self, "_dmb_folded", (conv.weight, conv.bias) + bn_parts(bn), lambda: (
            fold_batch_norm(bn, None, conv.in_channels, conv.weight.device) if bn is not None else (None, None),
            conv.weight.detach().float().contiguous(),
            conv.bias.detach().float().contiguous() if conv.bias is not None else None))

    def run(self, x, pool=False, in_window=None, x2=None, out=None, out_ch_offset=0):
        (ps, pt), w, bias = self._folded()
        return ops.preact_conv(x, w, self.stride, pool, ps, pt, True, None, bias, False, None, False, in_window, x2, out,
                               out_ch_offset)

    def forward(self, x):
        refuse_grad(self, x)
        return self.run(x)


class SmallConvBnRelu(nn.Sequential):
    """conv_bn_relu (layers/basic_layers.py:102-119) on few channels: Sequential(Conv2d, [BatchNorm2d], ReLU) as one launch, the
    BatchNorm (and bias) folded into the epilogue."""

    def __init__(self, batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
        check_preact_shape(in_planes, out_planes, kernel_size, stride, padding, dilation, 2)
        conv = nn.Conv2d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding, dilation=dilation,
                         bias=bias)
        super().__init__(*([conv] + ([nn.BatchNorm2d(out_planes)] if batch_norm else []) + [nn.ReLU(inplace=True)]))
        self.has_bn, self.stride = bool(batch_norm), stride
        if batch_norm and not self[1].track_running_stats:
            fold_batch_norm(self[1], None, out_planes, None)

    def _folded(self):
        conv, bn = self[0], (self[1] if self.has_bn else None)
        return param_state.cached(self, "_dmb_folded", (conv.weight, conv.bias) + bn_parts(bn), lambda: (
            fold_batch_norm(bn, conv.bias, conv.out_channels, conv.weight.device), conv.weight.detach().float().contiguous()))

    def forward(self, x):
        refuse_grad(self, x)
        (sc, sh), w = self._folded()
        return ops.preact_conv(x, w, self.stride, post_scale=sc, post_shift=sh, relu=True)


def bn_relu_conv(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """layers/basic_layers.py:122-138."""
    return PreActConv(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, ndim=2)


def bn_relu_conv3d(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """layers/basic_layers.py:180-197."""
    return PreActConv(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, ndim=3)
