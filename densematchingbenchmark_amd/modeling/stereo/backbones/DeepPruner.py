"""DeepPruner's two feature backbones: drop-in for dmb/modeling/stereo/backbones/DeepPruner.py (``DeepPrunerBestBackbone`` :8-133,
``DeepPrunerFastBackbone`` :136-253), same module tree (firstconv, layer1-4, branch1-4 | branch2-4, lastconv) and ``state_dict``
keys.  Per view they return ``(feature, [low-level maps])``.

Best is PSMNet's network with one more return value, layer1's output: it derives from ``PSMNetBackbone`` (its constructor, its
layers, its no-copy 320-channel buffer), asked to keep that map.  Fast shares the layer factory (``PSMNet.make_layer``) only:
it strides by 2 in layer3 as well, has no 64-pixel branch, and concatenates
cat(output_4_1, output_8, branch4, branch3, branch2) = 352 channels at an eighth of the image: layer3's and layer4's last blocks
and the three up-sampled branches write straight into their channel windows of one buffer.  Its two stride-2 64 -> 128 layers
(layer3's first 3x3 and its 1x1 skip) are two launches of 64 output channels each (``FusedConv2d.split_halves``).
Inference only."""
import torch
import torch.nn as nn

from .... import ops
from ..layers import train_fn
from ..layers.basic_layers_2d import conv_bn_relu
from .PSMNet import PSMNetBackbone, _BareConv1x1, make_layer

_NO_BACKWARD = "%s is inference-only (no backward on this path); call eval() and run under torch.no_grad()"


class _TwoViewEval:
    """What the two share beside the layer factories: the refusal of training and the two views on two streams."""

    def forward(self, *input):
        if len(input) != 2:
            raise ValueError("a stereo pair is two images, got %d inputs" % len(input))
        l_img, r_img = input
        if train_fn.wants_grad(self, l_img, r_img):
            raise NotImplementedError(_NO_BACKWARD % type(self).__name__)
        # (feature, [low-level maps]) per view; ops.two_view_forward warms the packed-weight caches before it forks and
        # records the caller's stream on every tensor the side stream returns
        return ops.two_view_forward(self._forward, l_img, r_img, module=self)


class DeepPrunerBestBackbone(_TwoViewEval, PSMNetBackbone):
    """DeepPruner.py:8-133: feature [B, 32, H/4, W/4] and [output_2_1 [B, 32, H/2, W/2]].  PSMNetBackbone's constructor, layers
    and no-copy 320-channel buffer."""

    def _forward(self, x):
        return self._features(x, keep_half=True)


class DeepPrunerFastBackbone(_TwoViewEval, nn.Module):
    """DeepPruner.py:136-253: feature [B, 32, H/8, W/8] and [output_4_0 [B, 64, H/4, W/4], output_2_1 [B, 32, H/2, W/2]]."""

    def __init__(self, in_planes=3, batch_norm=True):
        super().__init__()
        self.in_planes, self.batch_norm = in_planes, batch_norm
        bn = batch_norm
        self.firstconv = nn.Sequential(*[conv_bn_relu(bn, ci, 32, 3, stride, 1, 1, bias=False)
                                         for ci, stride in ((in_planes, 2), (32, 1), (32, 1))])
        self.in_planes = 32
        # (name, output channels, blocks, stride): layer3 strides too, layer4 is not dilated (DeepPruner.py:171-174)
        for name, planes, blocks, stride in (("layer1", 32, 3, 1), ("layer2", 64, 16, 2), ("layer3", 128, 3, 2), ("layer4", 128, 3, 1)):
            setattr(self, name, make_layer(bn, self.in_planes, planes, blocks, stride, 1, 1))
            self.in_planes = planes
        for i, k in ((2, 32), (3, 16), (4, 8)):   # DeepPruner.py:176-187
            setattr(self, "branch%d" % i, nn.Sequential(nn.AvgPool2d((k, k), stride=(k, k)),
                                                        conv_bn_relu(bn, 128, 32, 1, 1, 0, 1, bias=False)))
        self.lastconv = nn.Sequential(conv_bn_relu(bn, 352, 128, 3, 1, 1, 1, bias=False), _BareConv1x1(128, 32))

    def _forward(self, x):
        output_2_1 = self.layer1(self.firstconv(x))
        output_4_0 = self.layer2(output_2_1)
        B, _, H4, W4 = output_4_0.shape
        H8, W8 = (H4 - 1) // 2 + 1, (W4 - 1) // 2 + 1
        # DeepPruner.py:238-239: cat(output_4_1 [128], output_8 [128], branch4, branch3, branch2 [32 each])
        feat = torch.empty((B, 352, H8, W8), dtype=torch.float32, device=x.device)
        x = output_4_0
        for blk in self.layer3[:-1]:
            x = blk(x)
        self.layer3[-1](x, out=feat, out_ch_offset=0)                       # output_4_1 -> channels 0..127
        x = self.layer4[0](feat, in_window=(0, 128))                        # reads that window in place
        for blk in self.layer4[1:-1]:
            x = blk(x)
        self.layer4[-1](x, out=feat, out_ch_offset=128)                     # output_8 -> channels 128..255
        for i, off in ((4, 256), (3, 288), (2, 320)):
            branch = getattr(self, "branch%d" % i)
            pooled = ops.avgpool2d(feat, branch[0].kernel_size[0], in_window=(128, 128))
            ops.bilinear_ac(branch[1](pooled), (H8, W8), out=feat, out_ch_offset=off)
        return self.lastconv[1](self.lastconv[0](feat)), [output_4_0, output_2_1]
