"""DeepPruner's refinement cascade: drop-in for dmb/modeling/stereo/disp_refinement/DeepPruner.py:8-94 (``RefinementHeand`` --
the reference's spelling -- and ``DeepPrunerRefinement``), same constructor arguments, attribute names and ``state_dict`` keys.

Launches per stage: two copies into the guide buffer (cat(low_ref_group_fms[i], init_disp), :83), the six conv + BatchNorm + ReLU
layers on the fused conv2d kernel (Ci -> 32, 32 -> 32, 32 -> 32, 32 -> 16 dilation 2, 16 -> 16 dilation 4, 16 -> 16) and ONE launch
of csrc/refine_head.hip for the rest: classify (16 -> 1), + init_disp, ReLU (:40-42), * 2 and the bilinear up-sampling by two
(:87).  Inference only; the differentiable forward is ``train_fn.deeppruner_refinement`` (docs/design/22), which runs the six
layers on the training units' launches and the tail as two launches with the same bits, one autograd node per stage."""
import torch
import torch.nn as nn

from .... import ops_deeppruner
from ..layers import train_fn
from ..layers.basic_layers_2d import conv_bn_relu

_NO_BACKWARD = "%s is inference-only (no backward: the fused refinement head has none); call eval() and run under torch.no_grad()"


class _FusedClassify(nn.Conv2d):
    """nn.Conv2d(16, 1, 3, padding=1, bias=False) (DeepPruner.py:36) whose forward is the whole tail of the stage:
    up2(2 * relu(conv(x) + init_disp)).  The kernel takes the weight as it is: nothing is packed, so nothing can be stale."""

    def __init__(self, in_planes):
        super().__init__(in_planes, 1, kernel_size=3, padding=1, stride=1, bias=False)

    def forward(self, x, init_disp):
        if train_fn.wants_grad(self, x, init_disp):
            raise NotImplementedError(_NO_BACKWARD % "RefinementHeand.classify")
        return ops_deeppruner.refine_head_up2(x, self.weight.detach(), init_disp)


class RefinementHeand(nn.Module):
    """DeepPruner.py:8-44.  ``forward(init_disp, input)`` returns the reference's refined map ALREADY doubled and up-sampled,
    [B, 1, 2H, 2W]: the one consumer of the reference's return value (DeepPruner.py:85-87) does exactly that to it."""

    def __init__(self, in_planes, batch_norm=True):
        super().__init__()
        self.in_planes, self.batch_norm = in_planes, batch_norm
        # (input channels, output channels, dilation) of the six 3x3 conv + BatchNorm + ReLU layers
        table = ((in_planes, 32, 1), (32, 32, 1), (32, 32, 1), (32, 16, 2), (16, 16, 4), (16, 16, 1))
        self.conv = nn.Sequential(*[conv_bn_relu(batch_norm, ci, co, 3, 1, d, d, bias=False) for ci, co, d in table])
        self.classify = _FusedClassify(16)

    def forward(self, init_disp, input):
        if train_fn.wants_grad(self, init_disp, input):
            raise NotImplementedError(_NO_BACKWARD % type(self).__name__)
        return self.classify(self.conv(input), init_disp)


class DeepPrunerRefinement(nn.Module):
    """DeepPruner.py:47-94.  ``forward(disps, low_ref_group_fms)``: ``disps`` (a list) gains one map per stage, each twice the
    size of the last, and is returned reversed, the better map first."""

    def __init__(self, in_planes_list, batch_norm=True, num=1):
        super().__init__()
        self.in_planes_list, self.batch_norm, self.num = in_planes_list, batch_norm, num
        self.refine_blocks = nn.ModuleList([RefinementHeand(self.in_planes_list[i], self.batch_norm) for i in range(self.num)])

    def forward(self, disps, low_ref_group_fms):
        if train_fn.wants_grad(self, *disps, *low_ref_group_fms[:self.num]):
            raise NotImplementedError(_NO_BACKWARD % type(self).__name__)
        for i in range(self.num):
            init_disp, fms = disps[-1], low_ref_group_fms[i]
            B, C, H, W = fms.shape
            # cat(low_ref_group_fms[i], init_disp) (:83): one allocation, two copies; the feature map itself is left alone
            guide = torch.empty((B, C + 1, H, W), dtype=torch.float32, device=fms.device)
            guide[:, :C].copy_(fms)
            guide[:, C:].copy_(init_disp)
            disps.append(self.refine_blocks[i](init_disp, guide))
        disps.reverse()
        return disps
