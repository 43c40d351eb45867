"""Yardstick of the DeepPruner feature tests: ``DeepPrunerBestBackbone``, ``DeepPrunerFastBackbone`` (backbones/DeepPruner.py:8-253)
and ``RefinementHeand`` / ``DeepPrunerRefinement`` (disp_refinement/DeepPruner.py:8-94) restated in plain ``torch.nn`` with the
reference's ``state_dict`` keys.  FP32 and, after ``.double()``, FP64, on any device.

``seeded_state(module, seed)`` fills a module key by key in ``state_dict`` order from one seeded CPU generator: convolution
weights randn * sqrt(2 / (Ci * k * k)) (``classify``: randn * sqrt(1 / (Ci * 9))), BatchNorm weights uniform in [0.4, 0.8) (the
25 residual blocks of a backbone have no ReLU after their add; a gain of one would let the maps grow with depth), running
variances in [0.5, 1.5), biases and running means in [-0.1, 0.1).  Inputs and weights of ``REFINE_CASES`` / ``BACKBONE_CASES`` are
regenerated from seeds, never stored; the real reference's outputs (the backbones': strided sub-samples) are in
tests/golden/deeppruner_features.npz (scripts/gen_golden_deeppruner_features.py, which also asserts that this restatement equals
the reference bit for bit)."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_features.npz")
WEIGHT_SEED = 1701
# name -> (in_planes_list, num, batch, (H, W) of the first stage), input seed
REFINE_CASES = {"r4x": (([32 + 9 + 1], 1, 1, (24, 40)), 41),             # the 4x config's widths
                "r8x": (([64 + 9 + 1, 32 + 1], 2, 2, (8, 20)), 42),      # the 8x config's: two stages, 8 x 20 then 16 x 40; batch 2
                "rodd": (([4 + 2 + 1], 1, 2, (5, 13)), 43)}              # odd sizes below one tile; batch 2
# name -> (class name, image shape, input seed, per returned map the (y, x) stride of the recorded sub-sample): the smallest
# images at which the 64- (Best) and 32-pixel (Fast) average pools still have one window; W / 4 = 66 is no multiple of four
BACKBONE_CASES = {"best": ("DeepPrunerBestBackbone", (1, 3, 256, 264), 51, ((3, 3), (7, 7))),
                  "fast": ("DeepPrunerFastBackbone", (1, 3, 256, 320), 52, ((3, 3), (5, 5), (7, 7)))}


# ------------------------------------------------------------------------------------------------------------ layers
def _conv_bn(bn, ci, co, k=3, stride=1, padding=1, dilation=1, bias=True, relu=False):
    pad = dilation if dilation > 1 else padding                  # basic_layers.py:14-28
    layers = [nn.Conv2d(ci, co, k, stride=stride, padding=pad, dilation=dilation, bias=bias)]
    if bn:
        layers.append(nn.BatchNorm2d(co))
    if relu:
        layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


class BasicBlock(nn.Module):
    """basic_layers.py:219-243: no ReLU after the add."""

    def __init__(self, bn, ci, co, stride, downsample, padding, dilation):
        super().__init__()
        self.conv1 = _conv_bn(bn, ci, co, 3, stride, padding, dilation, bias=False, relu=True)
        self.conv2 = _conv_bn(bn, co, co, 3, 1, padding, dilation, bias=False)
        self.downsample = downsample

    def forward(self, x):
        out = self.conv2(self.conv1(x))
        return out + (self.downsample(x) if self.downsample is not None else x)


# ------------------------------------------------------------------------------------------------------------ backbones
class _Backbone(nn.Module):
    """What backbones/DeepPruner.py:27-85 and :157-211 share; ``layer3_stride``, ``layer4_dilation`` and ``pools`` differ."""

    def __init__(self, in_planes, bn, layer3_stride, layer4_dilation, pools, cat_planes):
        super().__init__()
        self.firstconv = nn.Sequential(_conv_bn(bn, in_planes, 32, 3, 2, 1, 1, bias=False, relu=True),
                                       _conv_bn(bn, 32, 32, 3, 1, 1, 1, bias=False, relu=True),
                                       _conv_bn(bn, 32, 32, 3, 1, 1, 1, bias=False, relu=True))
        self._planes = 32
        self.layer1 = self._make_layer(bn, 32, 3, 1, 1, 1)
        self.layer2 = self._make_layer(bn, 64, 16, 2, 1, 1)
        self.layer3 = self._make_layer(bn, 128, 3, layer3_stride, 1, 1)
        self.layer4 = self._make_layer(bn, 128, 3, 1, layer4_dilation, layer4_dilation)
        for i, k in pools:
            setattr(self, "branch%d" % i, nn.Sequential(nn.AvgPool2d((k, k), stride=(k, k)),
                                                        _conv_bn(bn, 128, 32, 1, 1, 0, 1, bias=False, relu=True)))
        self.lastconv = nn.Sequential(_conv_bn(bn, cat_planes, 128, 3, 1, 1, 1, bias=False, relu=True),
                                      nn.Conv2d(128, 32, kernel_size=1, padding=0, stride=1, dilation=1, bias=False))

    def _make_layer(self, bn, co, blocks, stride, padding, dilation):
        downsample = None
        if stride != 1 or self._planes != co:
            downsample = _conv_bn(bn, self._planes, co, k=1, stride=stride, padding=0, dilation=1)
        layers = [BasicBlock(bn, self._planes, co, stride, downsample, padding, dilation)]
        self._planes = co
        layers += [BasicBlock(bn, co, co, 1, None, padding, dilation) for _ in range(1, blocks)]
        return nn.Sequential(*layers)

    def _branch(self, i, x):
        return F.interpolate(getattr(self, "branch%d" % i)(x), x.shape[2:], mode='bilinear', align_corners=True)

    def forward(self, l_img, r_img):
        return self._forward(l_img), self._forward(r_img)


class DeepPrunerBestBackbone(_Backbone):
    def __init__(self, in_planes=3, batch_norm=True):
        super().__init__(in_planes, batch_norm, 1, 2, ((1, 64), (2, 32), (3, 16), (4, 8)), 320)

    def _forward(self, x):
        output_2_1 = self.layer1(self.firstconv(x))
        output_4_0 = self.layer2(output_2_1)
        output_8 = self.layer4(self.layer3(output_4_0))
        cat = torch.cat([output_4_0, output_8] + [self._branch(i, output_8) for i in (4, 3, 2, 1)], 1)
        return self.lastconv(cat), [output_2_1]


class DeepPrunerFastBackbone(_Backbone):
    def __init__(self, in_planes=3, batch_norm=True):
        super().__init__(in_planes, batch_norm, 2, 1, ((2, 32), (3, 16), (4, 8)), 352)

    def _forward(self, x):
        output_2_1 = self.layer1(self.firstconv(x))
        output_4_0 = self.layer2(output_2_1)
        output_4_1 = self.layer3(output_4_0)
        output_8 = self.layer4(output_4_1)
        cat = torch.cat([output_4_1, output_8] + [self._branch(i, output_8) for i in (4, 3, 2)], 1)
        return self.lastconv(cat), [output_4_0, output_2_1]


# ------------------------------------------------------------------------------------------------------------ refinement
class RefinementHeand(nn.Module):
    def __init__(self, in_planes, batch_norm=True):
        super().__init__()
        bn = batch_norm
        self.conv = nn.Sequential(_conv_bn(bn, in_planes, 32, bias=False, relu=True), _conv_bn(bn, 32, 32, bias=False, relu=True),
                                  _conv_bn(bn, 32, 32, bias=False, relu=True), _conv_bn(bn, 32, 16, dilation=2, bias=False, relu=True),
                                  _conv_bn(bn, 16, 16, dilation=4, bias=False, relu=True), _conv_bn(bn, 16, 16, bias=False, relu=True))
        self.classify = nn.Conv2d(16, 1, kernel_size=3, padding=1, stride=1, bias=False)

    def forward(self, init_disp, input):
        return F.relu(self.classify(self.conv(input)) + init_disp)


def refine_tail(x, w, init):
    """What ``dmb_refine_head_up2_f32`` computes, as the reference composes it (DeepPruner.py:40-42,87)."""
    refined = F.relu(F.conv2d(x, w, padding=1) + init)
    return F.interpolate(refined * 2, scale_factor=(2, 2), mode='bilinear', align_corners=False)


class DeepPrunerRefinement(nn.Module):
    def __init__(self, in_planes_list, batch_norm=True, num=1):
        super().__init__()
        self.num = num
        self.refine_blocks = nn.ModuleList([RefinementHeand(in_planes_list[i], batch_norm) for i in range(num)])

    def stages(self, disps, low_ref_group_fms):
        """Per stage (refined map before the up-sampling, up-sampled map): DeepPruner.py:79-89."""
        out, init_disp = [], disps[-1]
        for i in range(self.num):
            refined = self.refine_blocks[i](init_disp, torch.cat((low_ref_group_fms[i], init_disp), dim=1))
            init_disp = F.interpolate(refined * 2, scale_factor=(2, 2), mode='bilinear', align_corners=False)
            out.append((refined, init_disp))
        return out

    def forward(self, disps, low_ref_group_fms):
        disps = list(disps) + [up for _, up in self.stages(disps, low_ref_group_fms)]
        disps.reverse()
        return disps


# ------------------------------------------------------------------------------------------------------------ weights, inputs
def seeded_state(module, seed):
    g = torch.Generator().manual_seed(seed)
    new = {}
    for key, t in module.state_dict().items():
        if key.endswith("num_batches_tracked"):
            v = torch.zeros(t.shape, dtype=t.dtype)
        elif t.dim() == 4:
            gain = 1.0 if key.endswith("classify.weight") else 2.0
            v = torch.randn(t.shape, generator=g) * (gain / (t.shape[1] * t.shape[2] * t.shape[3])) ** 0.5
        elif key.endswith("running_var"):
            v = torch.rand(t.shape, generator=g) + 0.5
        elif key.endswith(".weight"):                            # BatchNorm
            v = torch.rand(t.shape, generator=g) * 0.4 + 0.4
        else:                                                    # biases, running_mean
            v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
        new[key] = v.to(dtype=t.dtype)
    module.load_state_dict(new)
    return module


def refinement(name, dtype=torch.float32):
    (planes, num, _, _), _ = REFINE_CASES[name]
    return seeded_state(DeepPrunerRefinement(planes, True, num), WEIGHT_SEED).to(dtype).eval()


def refine_inputs(name, dtype=torch.float32):
    """([init_disp [B, 1, H, W]], [guide features of stage i: [B, planes[i] - 1, 2^i H, 2^i W]]): features ~ N(0, 1), the
    disparity ~ N(0, 1): about half of the first stage's refined values are clamped by the ReLU."""
    (planes, num, B, (H, W)), seed = REFINE_CASES[name]
    g = torch.Generator().manual_seed(seed)
    fms = [torch.randn((B, planes[i] - 1, H << i, W << i), generator=g).to(dtype) for i in range(num)]
    return [torch.randn((B, 1, H, W), generator=g).to(dtype)], fms


def backbone(name, dtype=torch.float32):
    return seeded_state(globals()[BACKBONE_CASES[name][0]](3, True), WEIGHT_SEED).to(dtype).eval()


def backbone_input(name, dtype=torch.float32):
    """One image ~ N(0, 1) (a normalised image); the tests feed it as both views."""
    _, shape, seed, _ = BACKBONE_CASES[name]
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype)


def flatten(out):
    """(feature, [low-level maps]) -> [feature, *maps]."""
    return [out[0]] + list(out[1])


def subsample(name, maps):
    return [m[:, :, ::sy, ::sx] for m, (sy, sx) in zip(maps, BACKBONE_CASES[name][3])]


def recording():
    return np.load(GOLDEN)


_fp64 = {}


def fp64_refinement(name):
    """The FP64 restatement's stages [(refined, up-sampled), ...] on the CPU: computed once, shared, never modified."""
    if ("r", name) not in _fp64:
        disps, fms = refine_inputs(name, torch.float64)
        with torch.no_grad():
            _fp64[("r", name)] = refinement(name, torch.float64).stages(disps, fms)
    return _fp64[("r", name)]


def fp64_backbone(name, device="cpu"):
    """The FP64 restatement's sub-sampled maps [feature, *low-level maps], evaluated on ``device`` and kept on the CPU:
    computed once, shared, never modified."""
    if ("b", name) not in _fp64:
        x = backbone_input(name, torch.float64).to(device)
        with torch.no_grad():
            maps = flatten(backbone(name, torch.float64).to(device)._forward(x))
        _fp64[("b", name)] = [m.cpu().contiguous() for m in subsample(name, maps)]
    return _fp64[("b", name)]
