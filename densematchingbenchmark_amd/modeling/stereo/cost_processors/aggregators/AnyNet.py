"""cost_processors/aggregators/AnyNet.py:7-50: 2 + num bn_relu_conv3d units (bias=True), same ``agg.<i>.*`` keys; each unit is
one launch of csrc/preact_conv.hip."""
import torch.nn as nn

from ...layers.preact import bn_relu_conv3d, refuse_grad


class AnyNetAggregator(nn.Module):
    def __init__(self, in_planes=1, agg_planes=4, num=4, batch_norm=True):
        super().__init__()
        self.in_planes, self.agg_planes, self.num, self.batch_norm = in_planes, agg_planes, num, batch_norm
        agg_list = [bn_relu_conv3d(batch_norm, in_planes, agg_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True)]
        agg_list += [bn_relu_conv3d(batch_norm, agg_planes, agg_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=True)
                     for _ in range(num)]
        agg_list += [bn_relu_conv3d(batch_norm, agg_planes, 1, kernel_size=3, stride=1, padding=1, dilation=1, bias=True)]
        self.agg = nn.Sequential(*agg_list)

    def forward(self, raw_cost):
        """[B, in_planes, D, H, W] -> [[B, D, H, W]]."""
        refuse_grad(self, raw_cost)
        cost = raw_cost
        for unit in self.agg:
            cost = unit.run(cost)
        return [cost.squeeze(dim=1)]
