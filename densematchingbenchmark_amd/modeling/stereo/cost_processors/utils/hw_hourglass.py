"""DeepPruner's hourglass over the (y, x) plane: drop-in for cost_processors/utils/hw_hourglass.py:8-105."""
import torch.nn as nn

from ...layers import train_fn
from ...layers.basic_layers import conv3d_bn_relu, deconv3d_bn


class HWHourglass(nn.Module):
    """Three levels of (stride-(1, 2, 2) conv, stride-1 conv) down and three stride-(1, 2, 2) transposed convs up: nine fused
    launches (csrc/conv3d_hw.hip for the strided and 16-channel ones, conv3d.hip for the stride-1 layers of 32 / 64 / 128
    channels).  Every add of hw_hourglass.py:79-103 runs in the producing kernel's epilogue: ``conv*_b(x) + x`` as a skip after
    the ReLU, ``conv3_d(..) + out2_b`` and ``conv2_d(..) + out1_b`` as residuals without one.  The depth axis is never strided:
    [B, C, D, H, W] -> [B, C, D, H, W], H and W multiples of 8.  The extra keyword ``skip`` fuses a caller's ``hourglass(x) + x``
    (aggregators/DeepPruner.py:54) into conv1_d.  Inference only."""

    def __init__(self, in_planes, batch_norm=True):
        super().__init__()
        if in_planes != 16:
            raise NotImplementedError("HWHourglass on the HIP path: in_planes must be 16 (channel ladder 16 / 32 / 64 / 128: 8 would "
                                      "need 8-channel and 32 would need 256-channel kernels), got %r" % (in_planes,))
        self.in_planes, self.batch_norm = in_planes, batch_norm
        c, hw = in_planes, (1, 2, 2)
        for level, (ci, co) in enumerate(((c, 2 * c), (2 * c, 4 * c), (4 * c, 8 * c)), start=1):
            setattr(self, "conv%d_a" % level, conv3d_bn_relu(batch_norm, ci, co, kernel_size=3, stride=hw, padding=1, bias=False))
            setattr(self, "conv%d_b" % level, conv3d_bn_relu(batch_norm, co, co, kernel_size=3, stride=(1, 1, 1), padding=1, bias=False))
            setattr(self, "conv%d_d" % level, deconv3d_bn(batch_norm, co, ci, kernel_size=3, padding=1, output_padding=(0, 1, 1),
                                                          stride=hw, bias=False))

    def forward(self, raw_cost, skip=None):
        if train_fn.wants_grad(self, raw_cost, skip):
            raise NotImplementedError("HWHourglass is inference-only (no backward: the stride-(1, 2, 2) kernels have none); call "
                                      "eval() and run under torch.no_grad()")
        if raw_cost.dim() != 5 or raw_cost.shape[1] != self.in_planes or raw_cost.shape[3] % 8 or raw_cost.shape[4] % 8:
            # the reference fails here too: at a skip add, with a size mismatch (hw_hourglass.py:97-100)
            raise ValueError("HWHourglass: input must be [B, %d, D, H, W] with H and W multiples of 8, got %s"
                             % (self.in_planes, tuple(raw_cost.shape)))
        x, levels = raw_cost, []
        for k in (1, 2, 3):                                   # down (hw_hourglass.py:79-94): relu(bn(conv)) + its own input
            down = getattr(self, "conv%d_a" % k)(x)
            x = getattr(self, "conv%d_b" % k)(down, skip=down)
            levels.append(x)
        for k in (3, 2):                                      # up (:97-100): bn(deconv) + the level above, no ReLU
            x = getattr(self, "conv%d_d" % k)(x, residual=levels[k - 2])
        return self.conv1_d(x, residual=skip)                 # :103 (+ the caller's skip)
