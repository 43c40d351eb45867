"""The stride-1 5x5 2-D convolution of DeepPruner's cost processor on csrc/deeppruner_heads.hip: the three 1 -> 1 disparity
convolutions (cost_processors/DeepPruner.py:69-78,180-183: Conv2d with a bias, ReLU) and the three N -> N feature convolutions
(:80-84,184-188: ``conv_bn_relu``, layers/basic_layers.py:102-119) on 1 .. 16 channels.  Same Sequential keys as the reference
(``0.*`` the convolution, ``1.*`` the BatchNorm if there is one); each forward is ONE launch of dmb_conv2d_k5_small_f32 with the
bias or the eval-mode BatchNorm folded into the epilogue (fold_batch_norm).  The module's own ``forward`` is inference only; the
differentiable forward is ``train_fn.small_conv5x5(unit, x)`` (the same kernel for the raw convolution and, on mirrored weights, for
the data gradient; plan form 6 of csrc/wgrad.hip for the weight gradient)."""
import torch
import torch.nn as nn

from .... import ops_deeppruner, param_state
from .basic_layers import bn_parts, epoch_on_mode_switch, fold_batch_norm

__all__ = ["SmallConv5x5"]


class SmallConv5x5(nn.Sequential):
    """Sequential(Conv2d(in_planes, out_planes, 5, 1, 2), [BatchNorm2d], [ReLU]) as one launch."""

    def __init__(self, batch_norm, in_planes, out_planes, bias=True, relu=True):
        if not (1 <= in_planes <= ops_deeppruner.K5_MAX_C and 1 <= out_planes <= ops_deeppruner.K5_MAX_C):
            raise NotImplementedError("HIP 5x5 conv: 1 .. %d input and output channels, got %d -> %d"
                                      % (ops_deeppruner.K5_MAX_C, in_planes, out_planes))
        layers = [nn.Conv2d(in_planes, out_planes, kernel_size=5, stride=1, padding=2, dilation=1, bias=bias)]
        if batch_norm:
            layers.append(nn.BatchNorm2d(out_planes))
        if relu:
            layers.append(nn.ReLU(inplace=True))
        super().__init__(*layers)
        self.has_bn, self.has_relu = bool(batch_norm), bool(relu)
        self.in_planes, self.out_planes = in_planes, out_planes      # (what the unit skeleton of layers/train_fn.py reads)

    def train(self, mode=True):
        epoch_on_mode_switch(self, mode)
        return super().train(mode)

    def _folded(self):
        conv, bn = self[0], (self[1] if self.has_bn else None)

        def make():
            w = conv.weight.detach().float().contiguous()
            if bn is None:      # a plain bias: acc + bias[co], no multiply by one
                return w, None, (conv.bias.detach().float().contiguous() if conv.bias is not None else None)
            return (w,) + fold_batch_norm(bn, conv.bias, conv.out_channels, w.device)
        return param_state.cached(self, "_dmb_folded", (conv.weight, conv.bias) + bn_parts(bn), make)

    def forward(self, x):
        if self.training or (torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters()))):
            raise NotImplementedError("SmallConv5x5 is inference-only (no backward: the 5x5 kernel has none); call eval() and run "
                                      "under torch.no_grad()")
        w, scale, shift = self._folded()
        return ops_deeppruner.conv2d_k5_small(x, w, scale, shift, self.has_relu)
