"""2-D conv + BatchNorm (+ReLU) units and BasicBlock of the feature backbones on the fused HIP conv2d kernel.

Mirrors dmb/modeling/stereo/layers/basic_layers.py:31-46 (conv_bn), :105-123 (conv_bn_relu), :219-243 (BasicBlock):
same factory names, argument order and ``state_dict`` keys; torch.nn modules are parameter containers only."""
import torch
import torch.nn as nn

from .... import ops, param_state
from . import train_fn
from .basic_layers import bn_parts, epoch_on_mode_switch, fold_batch_norm

__all__ = ["FusedConv2d", "conv_bn", "conv_bn_relu", "BasicBlock"]


class FusedConv2d(nn.Sequential):
    """Sequential(Conv2d, [BatchNorm2d], [ReLU]) as ONE kernel launch: conv (k 1 or 3, stride 1 or 2, dilation 1, 2,
    4 or 8) + folded BN + optional residual + ReLU; may read / write channel windows of wider tensors.

    One form is TWO launches: stride 2 with exactly 128 output channels (kernel 1 or 3; layer3 of DeepPruner's fast backbone).
    The kernel launches stride 2 up to 64 output channels, so the weight rows are split before packing, scale and shift sliced,
    and the two halves written into the two channel halves of one output.  Inference only."""

    def __init__(self, batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True,
                 relu=False):
        # basic_layers.py:14-28: padding follows the dilation when dilation > 1
        pad = dilation if dilation > 1 else padding
        # (what dmb_conv2d_f32 launches: 32-channel output tiles, 1, 2 or 4 of them at stride 1, 1 or 2 at stride 2)
        if kernel_size not in (1, 3, 5) or stride not in (1, 2) or dilation not in (1, 2, 4, 8) \
                or pad != dilation * (kernel_size // 2) or (dilation > 2 and out_planes > 32) \
                or out_planes > 128 or 64 < out_planes <= 96 \
                or (stride == 2 and (dilation != 1 or (out_planes > 64 and (out_planes != 128 or kernel_size == 5)))) \
                or (kernel_size == 5 and (stride != 2 or dilation != 1 or out_planes > 32)):
            raise NotImplementedError("HIP conv2d: kernel 1|3, stride 1 (up to 64 or 97..128 output channels) with dilation 1|2 "
                                      "(4|8 up to 32 output channels), stride 2 (up to 64 output channels, or 128) without dilation, or "
                                      "kernel 5 with stride 2 (up to 32 output channels); 'same' padding")
        layers = [nn.Conv2d(in_planes, out_planes, kernel_size, stride=stride, padding=pad, dilation=dilation, bias=bias)]
        if batch_norm:
            layers.append(nn.BatchNorm2d(out_planes))
        if relu:
            layers.append(nn.ReLU(inplace=True))
        super().__init__(*layers)
        self.in_planes, self.out_planes = in_planes, out_planes
        self.kernel_size, self.stride, self.dilation = kernel_size, stride, dilation
        self.has_bn, self.has_relu = bool(batch_norm), bool(relu)
        self.split_halves = stride == 2 and out_planes == 128

    def train(self, mode=True):
        epoch_on_mode_switch(self, mode)
        return super().train(mode)

    def _prepacked(self):
        conv = self[0]
        bn = self[1] if self.has_bn else None

        def make():
            w = conv.weight.detach()
            scale, shift = fold_batch_norm(bn, conv.bias, self.out_planes, w.device)
            if self.split_halves:   # per half of the output channels: (packed rows, scale, shift)
                h = self.out_planes // 2
                return tuple((ops.pack_conv2d_weights(w[o:o + h]), None if scale is None else scale[o:o + h].contiguous(),
                              None if shift is None else shift[o:o + h].contiguous()) for o in (0, h))
            return ops.pack_conv2d_weights(w), scale, shift
        return param_state.cached(self, "_dmb_packed", (conv.weight, conv.bias) + bn_parts(bn), make)

    def forward(self, x, residual=None, relu=None, in_window=None, out=None, out_ch_offset=0, res_ch_offset=0):
        if train_fn.wants_grad(self, x, residual):
            # training / differentiable path: plain tensors (no channel windows), separate launches under torch.autograd
            if in_window is not None or out is not None or res_ch_offset:
                raise ValueError("FusedConv2d: channel windows are an inference-path feature")
            if self.split_halves:
                raise NotImplementedError("FusedConv2d: stride 2 with 128 output channels is inference-only (no backward)")
            return train_fn.conv2d_unit(self, x, residual, self.has_relu if relu is None else relu)
        if self.split_halves:
            return self._forward_halves(x, residual, self.has_relu if relu is None else relu, in_window, out, out_ch_offset,
                                        res_ch_offset)
        wp, scale, shift = self._prepacked()
        return ops.conv2d(x, wp, self.out_planes, self.kernel_size, self.stride, self.dilation, scale, shift, residual,
                          self.has_relu if relu is None else relu, in_window, out, out_ch_offset, res_ch_offset)

    def _forward_halves(self, x, residual, relu, in_window, out, out_ch_offset, res_ch_offset):
        h = self.out_planes // 2
        if out is None:
            B, _, H, W = x.shape
            out = torch.empty((B, self.out_planes, (H - 1) // 2 + 1, (W - 1) // 2 + 1), dtype=torch.float32, device=x.device)
            out_ch_offset = 0
        for i, (wp, scale, shift) in enumerate(self._prepacked()):
            ops.conv2d(x, wp, h, self.kernel_size, self.stride, self.dilation, scale, shift, residual, relu, in_window, out,
                       out_ch_offset + i * h, res_ch_offset + i * h)
        return out


def conv_bn(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """basic_layers.py:31-46."""
    return FusedConv2d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, relu=False)


def conv_bn_relu(batchNorm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True):
    """basic_layers.py:105-123."""
    return FusedConv2d(batchNorm, in_planes, out_planes, kernel_size, stride, padding, dilation, bias, relu=True)


class BasicBlock(nn.Module):
    """basic_layers.py:219-243: out = conv2(conv1(x)) + (downsample(x) | x), no ReLU after the add.  Two launches
    (three with a down-sampling 1x1 conv): the skip add runs in conv2's epilogue."""
    expansion = 1

    def __init__(self, batchNorm, in_planes, out_planes, stride, downsample, padding, dilation):
        super().__init__()
        self.conv1 = conv_bn_relu(batchNorm, in_planes, out_planes, 3, stride, padding, dilation, bias=False)
        self.conv2 = conv_bn(batchNorm, out_planes, out_planes, 3, 1, padding, dilation, bias=False)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x, out=None, out_ch_offset=0, in_window=None):
        """``in_window=(offset, channels)`` reads the block input from a channel window of a wider tensor."""
        if self.downsample is not None:
            skip, roff = self.downsample(x, in_window=in_window), 0
        else:
            skip, roff = x, (in_window[0] if in_window is not None else 0)
        return self.conv2(self.conv1(x, in_window=in_window), residual=skip, res_ch_offset=roff, out=out,
                          out_ch_offset=out_ch_offset)
