"""DeepPruner's cost processor: drop-in for cost_processors/DeepPruner.py:11-234 (``ConfidenceRangePredictor`` and
``DeepPrunerProcessor``), same constructor arguments, attribute names and ``state_dict`` keys.  Reached by import only (the model,
models/DeepPruner.py, constructs it directly): ``build_cost_processor`` refuses the type.

Launches.  The raw volume of both stages is ONE launch of csrc/deeppruner_heads.hip (``ops_deeppruner.deeppruner_volume``: the
sampled concatenation volume, the samples and -- stage "post" -- the range features on every plane, each element written once).
The 3-D layers are the fused units of the aggregator (layers/basic_layers.py, utils/hw_hourglass.py), the 32 -> 1 ends
``HeadConv3d``, the regressions ``ops.soft_argmin_sampled``, the up-sampling ``ops.bilinear_scale`` and the six 5x5 convolutions
``SmallConv5x5``.  Stage "pre": 1 + 4 + 2 * 11 + 2 + 4 = 33 launches; stage "post": 1 + 14 + 1 + 2 + 2 = 20.

The modules' own ``forward`` is inference only and refuses a call that wants gradients.  The differentiable forwards are functions
of layers/train_fn.py, as for the sampler and the aggregator: ``train_fn.confidence_range_predictor(predictor, raw_cost, samples)``
and ``train_fn.deeppruner_processor(processor, stage, left, right, samples, min_feature, max_feature)``, with gradients for both
feature maps, the samples, the range features and every parameter (the 5x5 convolutions on ``train_fn.small_conv5x5``: weight
gradient = plan form 6 of csrc/wgrad.hip, data gradient = the forward kernel on mirrored weights;
docs/design/21-deeppruner-processor-backward.md)."""
import torch.nn as nn

from .... import ops, ops_deeppruner
from ..layers import train_fn
from ..layers.basic_layers import HeadConv3d, conv3d_bn_relu
from ..layers.small_conv5x5 import SmallConv5x5
from .aggregators import build_cost_aggregator
from .utils.hw_hourglass import HWHourglass

_NO_BACKWARD = ("%s is inference-only (no backward: the stride-(1, 2, 2), 16-channel and 5x5 kernels have none); call eval() and "
                "run under torch.no_grad()")


class ConfidenceRangePredictor(nn.Module):
    """DeepPruner.py:11-119.  raw_cost [B, in_planes, D, H, W] and disparity_sample [B, D, H, W] (D = disparity_sample_number)
    -> min_disparity, max_disparity [B, 1, H, W] and min_disparity_feature, max_disparity_feature [B, D, H, W].
    ``forward`` is ``heads(*range_costs(raw_cost), disparity_sample)``."""

    def __init__(self, in_planes, hourglass_in_planes, disparity_sample_number, batch_norm=True):
        super().__init__()
        self.in_planes = in_planes
        self.hourglass_in_planes = hp = hourglass_in_planes
        self.disparity_sample_number = n = disparity_sample_number
        self.batch_norm = batch_norm
        self.dres0 = nn.Sequential(
            conv3d_bn_relu(batch_norm, in_planes, 64, kernel_size=3, stride=1, padding=1, bias=False),
            conv3d_bn_relu(batch_norm, 64, 32, kernel_size=3, stride=1, padding=1, bias=False))
        self.dres1 = nn.Sequential(
            conv3d_bn_relu(batch_norm, 32, 32, kernel_size=3, stride=1, padding=1, bias=False),
            conv3d_bn_relu(batch_norm, 32, hp, kernel_size=3, stride=1, padding=1, bias=False))
        for name in ("min_disparity_predictor", "max_disparity_predictor"):
            setattr(self, name, nn.Sequential(
                HWHourglass(hp, batch_norm),
                conv3d_bn_relu(batch_norm, hp, hp * 2, kernel_size=3, stride=1, padding=1, bias=False),
                HeadConv3d(hp * 2, bias=False)))
        # no BatchNorm on a disparity map (DeepPruner.py:68-78)
        self.min_disparity_conv = SmallConv5x5(False, 1, 1, bias=True)
        self.max_disparity_conv = SmallConv5x5(False, 1, 1, bias=True)
        self.min_disparity_feature_conv = SmallConv5x5(batch_norm, n, n, bias=True)
        self.max_disparity_feature_conv = SmallConv5x5(batch_norm, n, n, bias=True)

    def _refuse_grad(self, *tensors):
        if train_fn.wants_grad(self, *tensors):
            raise NotImplementedError(_NO_BACKWARD % type(self).__name__)

    def range_costs(self, raw_cost):
        """DeepPruner.py:88-96: the shared trunk and the two (hourglass, 16 -> 32, 32 -> 1) branches -> two [B, D, H, W] costs."""
        self._refuse_grad(raw_cost)
        cost = self.dres1(self.dres0(raw_cost))
        return self.min_disparity_predictor(cost).squeeze(1), self.max_disparity_predictor(cost).squeeze(1)

    def heads(self, cost_for_min, cost_for_max, disparity_sample):
        """DeepPruner.py:98-119: two soft arg-mins over the samples and the four 5x5 convolutions."""
        self._refuse_grad(cost_for_min, cost_for_max, disparity_sample)
        min_disparity = self.min_disparity_conv(ops.soft_argmin_sampled(cost_for_min, disparity_sample, 1.0, True))
        max_disparity = self.max_disparity_conv(ops.soft_argmin_sampled(cost_for_max, disparity_sample, 1.0, True))
        return (min_disparity, max_disparity,
                self.min_disparity_feature_conv(cost_for_min), self.max_disparity_feature_conv(cost_for_max))

    def forward(self, raw_cost, disparity_sample):
        self._refuse_grad(raw_cost, disparity_sample)
        cost_for_min, cost_for_max = self.range_costs(raw_cost)
        return self.heads(cost_for_min, cost_for_max, disparity_sample)


class DeepPrunerProcessor(nn.Module):
    """DeepPruner.py:122-234.  ``forward(stage, left, right, disparity_sample, min_disparity_feature=None,
    max_disparity_feature=None)``: stage "pre" returns the range predictor's four maps, any other stage ("post") returns
    [disparity [B, 1, 2H, 2W], disparity_feature [B, uniform_disparity_sample_number, 2H, 2W]]."""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg.copy()
        self.batch_norm = cfg.model.batch_norm
        self.patch_match_disparity_sample_number = cfg.model.cost_processor.patch_match_disparity_sample_number
        self.uniform_disparity_sample_number = cfg.model.cost_processor.uniform_disparity_sample_number
        # the config node itself, updated in place as the reference does (DeepPruner.py:167-172)
        self.confidence_range_predictor_args = cfg.model.cost_processor.confidence_range_predictor
        self.confidence_range_predictor_args.update(
            disparity_sample_number=self.patch_match_disparity_sample_number, batch_norm=self.batch_norm)
        self.confidence_range_predictor = ConfidenceRangePredictor(**self.confidence_range_predictor_args)
        self.cost_aggregator = build_cost_aggregator(cfg)
        self.disparity_conv = SmallConv5x5(False, 1, 1, bias=True)
        self.disparity_feature_conv = SmallConv5x5(self.batch_norm, self.uniform_disparity_sample_number,
                                                   self.uniform_disparity_sample_number, bias=True)

    def forward(self, stage, left, right, disparity_sample, min_disparity_feature=None, max_disparity_feature=None):
        if train_fn.wants_grad(self, left, right, disparity_sample, min_disparity_feature, max_disparity_feature):
            raise NotImplementedError(_NO_BACKWARD % type(self).__name__)
        if stage == 'pre':
            raw_cost = ops_deeppruner.deeppruner_volume(left, right, disparity_sample)                  # DeepPruner.py:192-195
            return self.confidence_range_predictor(raw_cost, disparity_sample)
        raw_cost = ops_deeppruner.deeppruner_volume(left, right, disparity_sample, min_disparity_feature,
                                                    max_disparity_feature)                               # :192-195, 204-208
        cost = self.cost_aggregator(raw_cost)[0]
        disparity = ops.soft_argmin_sampled(cost, disparity_sample, 1.0, True)                          # :216-218
        H, W = cost.shape[2:]
        # :221: interpolate(disparity * 2) -- doubling is exact in FP32, so interpolate(disparity) * 2 has the same bits
        disparity = ops.bilinear_scale(disparity, (2 * H, 2 * W), 2.0)
        disparity_feature = ops.bilinear_scale(cost, (2 * H, 2 * W))                                    # :224
        return [self.disparity_conv(disparity), self.disparity_feature_conv(disparity_feature)]
