"""disp_refinement/AnyNet.py:8-98: guidance from the left image (3 conv_bn_relu + a 3P-channel conv whose epilogue normalises the
gates), the disparity features, the left-to-right SPN scan (dmb.ops GateRecurrent2dnoind(True, False), csrc/spn.hip) and the
residual head ``relu(classify(.) + init_disp)``: 8 launches.  The plain convolutions keep their ``nn.Conv2d`` keys."""
import torch.nn as nn

from .... import ops
from ....spn import GateRecurrent2dnoind
from ..layers.preact import SmallConvBnRelu, check_preact_shape, refuse_grad


class AnyNetRefinement(nn.Module):
    def __init__(self, in_planes, spn_planes=8, batch_norm=True):
        super().__init__()
        self.in_planes, self.spn_planes, self.batch_norm = in_planes, spn_planes, batch_norm
        P = spn_planes
        check_preact_shape(2 * P, 3 * P, 3, 1, 1, 1, 2)
        self.img_conv = nn.Sequential(
            SmallConvBnRelu(batch_norm, in_planes, P * 2, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
            SmallConvBnRelu(batch_norm, P * 2, P * 2, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
            SmallConvBnRelu(batch_norm, P * 2, P * 2, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
            nn.Conv2d(P * 2, P * 3, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
        )
        self.disp_conv = nn.Conv2d(1, P, kernel_size=3, stride=1, padding=1, dilation=1, bias=False)
        self.classify = nn.Conv2d(P, 1, kernel_size=3, stride=1, padding=1, dilation=1, bias=False)
        self.spn = GateRecurrent2dnoind(True, False)

    def forward(self, disps, left, right, leftImage, rightImage):
        init_disp = disps[-1]
        refuse_grad(self, init_disp, leftImage)
        h, w = init_disp.shape[-2:]
        x = ops.bilinear_scale(leftImage, (h, w), 1.0)                      # :66
        for unit in self.img_conv[:3]:
            x = unit(x)
        G1, G2, G3 = ops.preact_conv(x, self.img_conv[3].weight.detach(), gate=True)     # :70-78
        disp_feat = ops.preact_conv(init_disp, self.disp_conv.weight.detach())          # :81
        propagated = ops.spn_gaterecurrent2d(disp_feat, G1, G2, G3, True, False)        # :84
        refine_disp = ops.preact_conv(propagated, self.classify.weight.detach(), residual=init_disp)   # :87-90
        disps.append(refine_disp)
        disps.reverse()
        return disps
