"""Yardstick of the DeepPruner cost-processor tests: ``ConfidenceRangePredictor`` and ``DeepPrunerProcessor``
(cost_processors/DeepPruner.py:11-234) restated in plain ``torch.nn`` with the reference's ``state_dict`` keys, on the restated
``HWHourglass`` / ``DeepPrunerAggregator`` of tests/_hw_ref.py and the warp of tests/_deeppruner_ref.py.  FP32 and, after
``.double()``, FP64, on any device.

``seeded_state(module, seed)`` is ``_hw_ref.seeded_state`` with one more rule, for the 4-D (5x5) weights:
randn * sqrt(2 / (Ci * 25)), the absolute value of it for the three 1 -> 1 filters (a disparity map stays a positive map; the
``rand + 0.5`` that rule set gives every other ``.weight`` would blow the maps up).  Inputs and weights of ``CASES`` are regenerated
from seeds, never stored; the real reference's outputs are in tests/golden/deeppruner_processor.npz
(scripts/gen_golden_deeppruner_processor.py, which also asserts that this restatement equals the reference bit for bit).

The FP64 yardstick (``fp64_outputs``) starts AFTER the volume: it takes the FP32 raw volume -- bit-identical on the CPU, in the
reference and on the HIP path -- cast to double and evaluates the rest in FP64 (an FP64 sampler would flip ``T > 0`` where T ~ 0 and
move outputs by their own size); the post stage is fed the recording's FP32 pre-stage features."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import _hw_ref as HW
from tests._deeppruner_ref import inverse_warp_3d

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_processor.npz")
HOURGLASS_IN_PLANES, WEIGHT_SEED = 16, 1601
# name -> (B, C, P = pre-stage samples, N = post-stage samples, H, W), input seed
CASES = {"a": ((1, 4, 5, 3, 16, 24), 31),      # odd sample counts
         "b": ((2, 6, 14, 9, 8, 40), 32),      # the config's sample counts; the deepest hourglass level is 1 x 5; batch 2
         "c": ((1, 4, 2, 2, 24, 8), 33)}       # the builder's minimum of two planes; taller than wide
PRE_OUTPUTS = ("min_disparity", "max_disparity", "min_feature", "max_feature")
POST_OUTPUTS = ("disparity", "feature")
OUTPUTS = tuple("pre/" + n for n in PRE_OUTPUTS) + tuple("post/" + n for n in POST_OUTPUTS)
# recorded next to the six outputs: what feeds the soft arg-mins (the reference's error there is a yardstick of the GPU tests)
COSTS = ("pre/cost_for_min", "pre/cost_for_max", "post/cost")


def _conv2(bn, ci, co):
    layers = [nn.Conv2d(ci, co, 5, stride=1, padding=2, bias=True)]
    if bn:
        layers.append(nn.BatchNorm2d(co))
    layers.append(nn.ReLU(inplace=True))
    return nn.Sequential(*layers)


def _range_branch(bn, hp):
    return nn.Sequential(HW.HWHourglass(hp, bn), HW._conv(bn, hp, 2 * hp), nn.Conv3d(2 * hp, 1, 3, stride=1, padding=1, bias=False))


def soft_argmin(cost, disparity_sample):
    return torch.sum(F.softmax(cost, dim=1) * disparity_sample, dim=1, keepdim=True)


class ConfidenceRangePredictor(nn.Module):
    def __init__(self, in_planes, hourglass_in_planes, disparity_sample_number, batch_norm=True):
        super().__init__()
        hp, n = hourglass_in_planes, disparity_sample_number
        self.dres0 = nn.Sequential(HW._conv(batch_norm, in_planes, 64), HW._conv(batch_norm, 64, 32))
        self.dres1 = nn.Sequential(HW._conv(batch_norm, 32, 32), HW._conv(batch_norm, 32, hp))
        self.min_disparity_predictor = _range_branch(batch_norm, hp)
        self.max_disparity_predictor = _range_branch(batch_norm, hp)
        self.min_disparity_conv = _conv2(False, 1, 1)
        self.max_disparity_conv = _conv2(False, 1, 1)
        self.min_disparity_feature_conv = _conv2(batch_norm, n, n)
        self.max_disparity_feature_conv = _conv2(batch_norm, n, n)

    def range_costs(self, raw_cost):
        cost = self.dres1(self.dres0(raw_cost))
        return self.min_disparity_predictor(cost).squeeze(1), self.max_disparity_predictor(cost).squeeze(1)

    def heads(self, cost_for_min, cost_for_max, disparity_sample):
        return (self.min_disparity_conv(soft_argmin(cost_for_min, disparity_sample)),
                self.max_disparity_conv(soft_argmin(cost_for_max, disparity_sample)),
                self.min_disparity_feature_conv(cost_for_min), self.max_disparity_feature_conv(cost_for_max))

    def forward(self, raw_cost, disparity_sample):
        return self.heads(*self.range_costs(raw_cost), disparity_sample)


def raw_volume(left, right, disparity_sample, min_feature=None, max_feature=None):
    """DeepPruner.py:192-195,204-208 (cat_fms.py:65-82 for the first 2C channels)."""
    B, C, H, W = left.shape
    D = disparity_sample.shape[1]
    target = inverse_warp_3d(right, -disparity_sample)
    reference = left.unsqueeze(2).expand(B, C, D, H, W) * (target > 0).to(left.dtype)
    parts = [reference, target, disparity_sample.unsqueeze(1)]
    if min_feature is not None:
        parts += [min_feature.unsqueeze(2).expand(-1, -1, D, -1, -1), max_feature.unsqueeze(2).expand(-1, -1, D, -1, -1)]
    return torch.cat(parts, dim=1)


class DeepPrunerProcessor(nn.Module):
    """``channels``: C of the image features; P, N: the sample counts of the two stages."""

    def __init__(self, channels, patch_match_samples, uniform_samples, hourglass_in_planes=HOURGLASS_IN_PLANES, batch_norm=True):
        super().__init__()
        C, P, N = channels, patch_match_samples, uniform_samples
        self.confidence_range_predictor = ConfidenceRangePredictor(2 * C + 1, hourglass_in_planes, P, batch_norm)
        self.cost_aggregator = HW.DeepPrunerAggregator(2 * C + 2 * P + 1, hourglass_in_planes, batch_norm)
        self.disparity_conv = _conv2(False, 1, 1)
        self.disparity_feature_conv = _conv2(batch_norm, N, N)

    def post_heads(self, cost, disparity_sample):
        """DeepPruner.py:216-230 from the aggregated cost."""
        disparity = soft_argmin(cost, disparity_sample)
        disparity = F.interpolate(disparity * 2, scale_factor=(2, 2), mode='bilinear', align_corners=False)
        disparity_feature = F.interpolate(cost, scale_factor=(2, 2), mode='bilinear', align_corners=False)
        return [self.disparity_conv(disparity), self.disparity_feature_conv(disparity_feature)]

    def from_volume(self, stage, raw_cost, disparity_sample):
        if stage == 'pre':
            return self.confidence_range_predictor(raw_cost, disparity_sample)
        return self.post_heads(self.cost_aggregator(raw_cost)[0], disparity_sample)

    def forward(self, stage, left, right, disparity_sample, min_disparity_feature=None, max_disparity_feature=None):
        if stage == 'pre':
            return self.from_volume(stage, raw_volume(left, right, disparity_sample), disparity_sample)
        return self.from_volume(stage, raw_volume(left, right, disparity_sample, min_disparity_feature, max_disparity_feature),
                                disparity_sample)


def seeded_state(module, seed):
    """``_hw_ref.seeded_state`` plus the rule for 4-D weights; fills ``module`` in place key by key from one seeded CPU generator."""
    g = torch.Generator().manual_seed(seed)
    new = {}
    for key, t in module.state_dict().items():
        if key.endswith("num_batches_tracked"):
            v = torch.zeros(t.shape, dtype=t.dtype)
        elif t.dim() == 5:
            v = torch.randn(t.shape, generator=g) * (2.0 / (_fan_in_3d(key, t, module))) ** 0.5
        elif t.dim() == 4:
            v = torch.randn(t.shape, generator=g) * (2.0 / (t.shape[1] * 25)) ** 0.5
            if tuple(t.shape[:2]) == (1, 1):
                v = v.abs()
        elif key.endswith("running_var") or key.endswith(".weight"):
            v = torch.rand(t.shape, generator=g) + 0.5
        else:                                                    # biases, running_mean
            v = torch.rand(t.shape, generator=g) * 0.2 - 0.1
        new[key] = v.to(dtype=t.dtype)
    module.load_state_dict(new)
    return module


def _fan_in_3d(key, t, module):
    """Ci * 27, a quarter of it for the stride-(1, 2, 2) transposed layers (``_hw_ref.seeded_state``'s rule)."""
    owner = module.get_submodule(key.rsplit(".", 1)[0])
    return t.shape[0] * 27 / 4.0 if isinstance(owner, nn.ConvTranspose3d) else t.shape[1] * 27


def case_inputs(name, dtype=torch.float32):
    """left, right [B, C, H, W] ~ N(0, 1); the pre stage's samples [B, P, H, W] and the post stage's [B, N, H, W]: uniform in
    [0, W / 2), ascending along the sample axis."""
    (B, C, P, N, H, W), seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    left, right = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    pre = torch.sort(torch.rand((B, P, H, W), generator=g) * (W / 2.0), dim=1)[0]
    post = torch.sort(torch.rand((B, N, H, W), generator=g) * (W / 2.0), dim=1)[0]
    return tuple(t.to(dtype) for t in (left, right, pre, post))


def processor(name, dtype=torch.float32, seed=WEIGHT_SEED):
    (B, C, P, N, H, W), _ = CASES[name]
    return seeded_state(DeepPrunerProcessor(C, P, N), seed).to(dtype).eval()


def recording():
    return np.load(GOLDEN)


_fp64 = {}


def fp64_outputs(name):
    """{"pre/cost_for_min", ..., "post/feature"} -> the FP64 evaluation from the FP32 volumes on the CPU: computed once, shared,
    never modified."""
    if name not in _fp64:
        z = recording()
        left, right, pre, post = case_inputs(name)
        proc = processor(name, torch.float64)
        out = {}
        with torch.no_grad():
            crp = proc.confidence_range_predictor
            costs = crp.range_costs(raw_volume(left, right, pre).double())
            out["pre/cost_for_min"], out["pre/cost_for_max"] = costs
            for n, t in zip(PRE_OUTPUTS, crp.heads(*costs, pre.double())):
                out["pre/" + n] = t
            fmin, fmax = (torch.from_numpy(z["%s/pre/%s" % (name, n)]) for n in ("min_feature", "max_feature"))
            out["post/cost"] = proc.cost_aggregator(raw_volume(left, right, post, fmin, fmax).double())[0]
            for n, t in zip(POST_OUTPUTS, proc.post_heads(out["post/cost"], post.double())):
                out["post/" + n] = t
        _fp64[name] = out
    return _fp64[name]
