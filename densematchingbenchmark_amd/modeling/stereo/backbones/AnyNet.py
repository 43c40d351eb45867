"""AnyNet's feature extractor: backbones/AnyNet.py:8-113 of the reference, same module tree and ``state_dict`` keys (the
``nn.MaxPool2d`` slots of the down blocks are kept, so indices match), run as 14 launches of csrc/preact_conv.hip and
conv2d.hip's half-pixel resampler for BOTH views at once (the same weights and running statistics apply to the two images in
eval).  Each 2x2 max-pool is fused into the prologue of the conv after it, and the two ``torch.cat`` inputs of the mixing
blocks are written in place: ``output_4x`` / ``output_8x`` and the up-sampled maps land in their channel windows."""
import torch.nn as nn

from .... import ops
from ..layers.preact import PreActConv, bn_relu_conv, check_preact_shape, refuse_grad


class AnyNetBackbone(nn.Module):
    def __init__(self, in_planes=3, C=1, block_num=2, batch_norm=True):
        super().__init__()
        self.in_planes, self.C, self.block_num, self.batch_norm = in_planes, C, block_num, batch_norm
        check_preact_shape(in_planes, C, 3, 1, 1, 1, 2)
        self.conv_4x = nn.Sequential(
            nn.Conv2d(in_planes, C, 3, 1, 1, dilation=1, bias=False),
            bn_relu_conv(batch_norm, C, C, 3, 2, 1, dilation=1, bias=False),
            self._make_down_blocks(batch_norm, C, 2 * C, block_num),
        )
        self.conv_8x = self._make_down_blocks(batch_norm, 2 * C, 4 * C, block_num)
        self.conv_16x = self._make_down_blocks(batch_norm, 4 * C, 8 * C, block_num)
        self.conv_mix_8x = self._make_up_blocks(batch_norm, 12 * C, 4 * C)
        self.conv_mix_4x = self._make_up_blocks(batch_norm, 6 * C, 2 * C)

    def _make_down_blocks(self, batch_norm, in_planes, out_planes, block_num):
        blocks = [nn.MaxPool2d(kernel_size=(2, 2), stride=(2, 2))]
        for _ in range(block_num):
            blocks.append(bn_relu_conv(batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, bias=False))
            in_planes = out_planes
        return nn.Sequential(*blocks)

    def _make_up_blocks(self, batch_norm, in_planes, out_planes):
        return nn.Sequential(
            bn_relu_conv(batch_norm, in_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
            bn_relu_conv(batch_norm, out_planes, out_planes, kernel_size=3, stride=1, padding=1, dilation=1, bias=False),
        )

    @staticmethod
    def _down(blocks, x, in_window, out=None, out_ch_offset=0):
        """MaxPool2d + block_num bn_relu_convs; the pool runs in the first conv's prologue, the last conv writes ``out``."""
        convs = [m for m in blocks if isinstance(m, PreActConv)]
        for i, m in enumerate(convs):
            last = i == len(convs) - 1
            x = m.run(x, pool=i == 0, in_window=in_window if i == 0 else None, out=out if last else None,
                      out_ch_offset=out_ch_offset if last else 0)
        return x

    def features(self, l_img, r_img):
        """Both views in one pass: [2B, 8C, H/16, W/16], [2B, 4C, H/8, W/8], [2B, 2C, H/4, W/4] (left = items [0, B))."""
        C = self.C
        stem = self.conv_4x[0]
        x = ops.preact_conv(l_img, stem.weight.detach(), x2=r_img)                          # nn.Conv2d(3, C), no prologue
        x = self.conv_4x[1].run(x)                                                           # stride 2
        B2, _, h4, w4 = x.shape[0], None, x.shape[2] // 2, x.shape[3] // 2
        cat4 = x.new_empty((B2, 6 * C, h4, w4))                                              # [output_4x | up(output_mix_8x)]
        self._down(self.conv_4x[2], x, None, cat4, 0)
        h8, w8 = h4 // 2, w4 // 2
        cat8 = x.new_empty((B2, 12 * C, h8, w8))                                             # [output_8x | up(output_16x)]
        self._down(self.conv_8x, cat4, (0, 2 * C), cat8, 0)
        out16 = self._down(self.conv_16x, cat8, (0, 4 * C))
        ops.bilinear_scale(out16, (h8, w8), 1.0, out=cat8, out_ch_offset=4 * C)
        mix8 = self.conv_mix_8x[1].run(self.conv_mix_8x[0].run(cat8))
        ops.bilinear_scale(mix8, (h4, w4), 1.0, out=cat4, out_ch_offset=2 * C)
        mix4 = self.conv_mix_4x[1].run(self.conv_mix_4x[0].run(cat4))
        return out16, mix8, mix4

    def forward(self, *input):
        if len(input) != 2:
            raise ValueError('expected input length 2 (got {} length input)'.format(len(input)))
        l_img, r_img = input
        refuse_grad(self, l_img, r_img)
        fms = self.features(l_img, r_img)
        B = l_img.shape[0]
        return [f[:B] for f in fms], [f[B:] for f in fms]
