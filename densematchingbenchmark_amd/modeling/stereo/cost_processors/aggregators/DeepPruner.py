"""DeepPruner cost aggregation: drop-in for cost_processors/aggregators/DeepPruner.py:8-59."""
import torch.nn as nn

from ...layers import train_fn
from ...layers.basic_layers import HeadConv3d, conv3d_bn_relu
from ..utils.hw_hourglass import HWHourglass


class DeepPrunerAggregator(nn.Module):
    """dres0 (in_planes -> 64 -> 32) and dres1 (32 -> 32 -> hourglass_in_planes) at stride 1, one ``HWHourglass`` whose output is
    added to its input (in conv1_d's epilogue), and the classifier hourglass_in_planes -> 2x -> 1.  Returns ``[cost]`` at the
    volume's own resolution, [B, D, H, W] (DeepPruner.py:47-59).  14 launches.  Inference only."""

    def __init__(self, in_planes, hourglass_in_planes, batch_norm=True):
        super().__init__()
        self.in_planes, self.hourglass_in_planes, self.batch_norm = in_planes, hourglass_in_planes, batch_norm
        hp = hourglass_in_planes
        self.dres0 = nn.Sequential(
            conv3d_bn_relu(batch_norm, in_planes, 64, kernel_size=3, stride=1, padding=1, bias=False),
            conv3d_bn_relu(batch_norm, 64, 32, kernel_size=3, stride=1, padding=1, bias=False))
        self.dres1 = nn.Sequential(
            conv3d_bn_relu(batch_norm, 32, 32, kernel_size=3, stride=1, padding=1, bias=False),
            conv3d_bn_relu(batch_norm, 32, hp, kernel_size=3, stride=1, padding=1, bias=False))
        self.dres2 = HWHourglass(hp, batch_norm=batch_norm)
        self.classify = nn.Sequential(
            conv3d_bn_relu(batch_norm, hp, hp * 2, kernel_size=3, stride=1, padding=1, bias=False),
            HeadConv3d(hp * 2, bias=False))

    def forward(self, raw_cost):
        if hasattr(raw_cost, "materialize"):   # the sampled volume of DeepPruner has no 2-D form: a lazy one is written out
            raw_cost = raw_cost.materialize()
        if train_fn.wants_grad(self, raw_cost):
            raise NotImplementedError("DeepPrunerAggregator is inference-only (no backward: the stride-(1, 2, 2) and 16-channel "
                                      "kernels have none); call eval() and run under torch.no_grad()")
        trunk = self.dres1(self.dres0(raw_cost))                                  # DeepPruner.py:49-51
        return [self.classify(self.dres2(trunk, skip=trunk)).squeeze(1)]          # :54 (the add in conv1_d's epilogue), :57
