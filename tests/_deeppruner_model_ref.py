"""Yardstick of the DeepPruner model tests: the eval forward of the reference's ``DeepPruner`` (models/DeepPruner.py:36-122)
restated in plain ``torch.nn`` / functional torch from the restatements of its four parts -- the backbones and the refinement of
tests/_deeppruner_features_ref.py, the sampler of tests/_deeppruner_ref.py, the cost processor of
tests/_deeppruner_processor_ref.py -- with the reference's ``state_dict`` keys.  FP32 and, after ``.double()``, FP64, on any device.

Weights are seeded per submodule with the rule of the restatement it comes from (``seeded_model``); images and PatchMatch's noise
are regenerated from seeds (``inputs``), never stored.  The real reference's outputs (every output map sub-sampled, the two range
maps whole) are in tests/golden/deeppruner_model.npz (scripts/gen_golden_deeppruner_model.py, which also asserts that this
restatement equals the reference bit for bit in FP32).

The FP64 yardstick takes the REFERENCE's decisions for the two ``target > 0`` masks of the raw volumes: where a warped value T is
~0 its sign is a decision, not a rounding -- an FP64 run, or an FP32 run on another CPU, decides it the other way at a few voxels and
moves the outputs near them by their own size (measured here: 0.4 - 0.7 pixels against 0.08 of rounding; the finding of
tests/_deeppruner_processor_ref.py, whose FP64 yardstick starts after the volume for that reason).  The recording holds, per
volume, the flat indices of the voxels with 0 < |T| < ``NEAR_ZERO`` in the FP64 run and the reference's decision at each (a few
hundred); everywhere else the FP64 run's own ``T > 0`` is the reference's (asserted when the recording is written).  Everything
else -- PatchMatch, the soft arg-mins, every convolution, the ReLUs and clamps -- is evaluated in FP64 end to end."""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests import _deeppruner_features_ref as FT
from tests import _deeppruner_processor_ref as PR
from tests import _deeppruner_ref as SM

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_model.npz")
CHANNELS, PATCH_MATCH_SAMPLES, UNIFORM_SAMPLES = 32, 14, 9
# name -> (the reference's config file, backbone class, the sampler's max_disp, refinement in_planes_list, image shape, input seed,
# the (y, x) stride of the recorded sub-samples).  Image sizes: multiples of 32 (4x) / 64 (8x) -- features whose sides are multiples
# of 8, as the three stride-2 levels of the hourglasses need -- at which the backbones' average pools (64 pixels at 1/4, 32 at 1/8)
# still have one window: 256 rows.  288 columns are 4.5 tiles of the tail kernel; the 8x case has batch 2.
CASES = {"4x": ("configs/DeepPruner/scene_flow_4x.py", "DeepPrunerBestBackbone", 48, [42], (1, 3, 256, 288), 61, (3, 5)),
         "8x": ("configs/DeepPruner/scene_flow_8x.py", "DeepPrunerFastBackbone", 24, [74, 33], (2, 3, 256, 320), 62, (5, 7))}
SEEDS = dict(backbone=1801, cost_processor=1802, disp_refinement=1803)
# what ``seeded_model`` changes after the parts' own rules, key suffix -> the sum its 1 -> 1 5x5 filter is normalised to: those rules
# give the three positive filters a sum of about 6 each, which here would stack to disparities of a thousand pixels and leave the
# range unordered.  0.6 / 1.2 / 1.0 keep a disparity a disparity and put min below max on most pixels, as a trained predictor does.
FILTER_SUMS = {"confidence_range_predictor.min_disparity_conv.0.weight": 0.6,
               "confidence_range_predictor.max_disparity_conv.0.weight": 1.2, "disparity_conv.0.weight": 1.0}
# ... and the gain on every ``classify.weight``: the residual of a refinement stage must reach the size of the disparity it is
# added to (tens of pixels), or the ReLU after the add never clamps (measured: 1 % and 78 - 90 % of clamped zeros in the two cases)
CLASSIFY_GAIN = 5.0
NEAR_ZERO = 1e-3          # |T| below which the sign of a warped value is taken from the recording (FP32 rounding moves T by ~1e-5)


class DeepPrunerModel(nn.Module):
    def __init__(self, name):
        super().__init__()
        _, backbone, self.sampler_max_disp, planes, _, _, _ = CASES[name]
        self.backbone = getattr(FT, backbone)(3, True)
        self.cost_processor = PR.DeepPrunerProcessor(CHANNELS, PATCH_MATCH_SAMPLES, UNIFORM_SAMPLES)
        self.disp_refinement = FT.DeepPrunerRefinement(planes, True, len(planes))

    def parts(self, left, right, noise, masks=None):
        """The reference's sequence, :43-79 -> (the refinement's list, better first; min_disparity, max_disparity at feature size;
        the two ``target > 0`` masks; the two warped volumes' targets).  ``masks``: per volume a whole mask, or (flat indices,
        decisions) that overrule ``target > 0`` at those voxels (the FP64 yardstick), instead of deciding everything here."""
        (ref_fms, low), (tgt_fms, _) = self.backbone(left, right)
        pre = SM.sampler('pre', ref_fms, tgt_fms, noise=noise, max_disp=self.sampler_max_disp)
        volume, mask_pre, t_pre = raw_volume(ref_fms, tgt_fms, pre, mask=None if masks is None else masks[0])
        lo, hi, lo_feature, hi_feature = self.cost_processor.from_volume('pre', volume, pre)
        post = SM.sampler('post', ref_fms, tgt_fms, lo, hi, max_disp=self.sampler_max_disp, uniform_sample_number=UNIFORM_SAMPLES)
        volume, mask_post, t_post = raw_volume(ref_fms, tgt_fms, post, lo_feature, hi_feature,
                                               mask=None if masks is None else masks[1])
        disparity, disparity_feature = self.cost_processor.from_volume('post', volume, post)
        low = list(low)
        low[0] = torch.cat((low[0], disparity_feature), dim=1)
        return self.disp_refinement([disparity], low), lo, hi, (mask_pre, mask_post), (t_pre, t_post)

    def forward(self, left, right, noise, masks=None):
        disps, lo, hi, masks, targets = self.parts(left, right, noise, masks)
        return dict(disps=final_maps(disps, lo, hi, left.shape[-2:]), min_disparity=lo, max_disparity=hi, masks=masks,
                    targets=targets)


def raw_volume(left, right, disparity_sample, min_feature=None, max_feature=None, mask=None):
    """``_deeppruner_processor_ref.raw_volume`` (cost_processors/DeepPruner.py:192-195,204-208) that also returns its mask and its
    warped target, and takes a whole mask or (flat indices, decisions) that overrule ``target > 0``."""
    B, C, H, W = left.shape
    D = disparity_sample.shape[1]
    target = SM.inverse_warp_3d(right, -disparity_sample)
    if mask is None:
        mask = target > 0
    elif isinstance(mask, tuple):
        index, decision = mask
        mask = (target > 0).contiguous()
        mask.view(-1)[index.to(mask.device)] = decision.to(mask.device)
    reference = left.unsqueeze(2).expand(B, C, D, H, W) * mask.to(device=left.device).to(left.dtype)
    parts = [reference, target, disparity_sample.unsqueeze(1)]
    if min_feature is not None:
        parts += [min_feature.unsqueeze(2).expand(-1, -1, D, -1, -1), max_feature.unsqueeze(2).expand(-1, -1, D, -1, -1)]
    return torch.cat(parts, dim=1), mask, target


def up(d, size):
    """models/DeepPruner.py:83-94: (d * W) / w, then the half-pixel bilinear interpolation."""
    H, W = size
    return F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=False)


def final_maps(disps, min_disparity, max_disparity, size):
    """models/DeepPruner.py:82-94,115: K + 4 maps.  The full-size range maps go through ``up`` a second time (:94)."""
    D, Mn, Mx = up(disps[-1], size), up(min_disparity, size), up(max_disparity, size)
    return [up(d, size) for d in list(disps) + [Mn, Mx]] + [abs(D - Mn), abs(Mx - D)]


def final_maps_unfused(ops, disps, min_disparity, max_disparity, size):
    """The same K + 4 maps as launches of the library and of torch on the device: what ``deeppruner_final_maps`` replaces.
    The divisor is a device tensor: ``tensor / python_number`` on the GPU is ATen's multiplication by the reciprocal, which is the
    IEEE division of the reference's recording (and of ATen's CPU path) only for a power of two."""
    H, W = size

    def ieee_div(t, n):
        return torch.div(t, torch.full((), float(n), dtype=t.dtype, device=t.device))

    def up_(d):
        return ops.bilinear_scale(ieee_div(d * W, d.shape[-1]), (H, W), 1.0)

    D, Mn, Mx = up_(disps[-1]), up_(min_disparity), up_(max_disparity)
    return [up_(d) for d in disps] + [ieee_div(Mn * W, W), ieee_div(Mx * W, W), torch.abs(D - Mn), torch.abs(Mx - D)]


def seeded_model(module):
    """Fills anything with the model's three submodules -- this restatement, the reference's model, the HIP model -- in place."""
    FT.seeded_state(module.backbone, SEEDS["backbone"])
    PR.seeded_state(module.cost_processor, SEEDS["cost_processor"])
    FT.seeded_state(module.disp_refinement, SEEDS["disp_refinement"])
    with torch.no_grad():
        for key, t in module.state_dict().items():
            for suffix, total in FILTER_SUMS.items():
                if key == "cost_processor." + suffix:
                    t.mul_(total / t.sum())
            if key.endswith("classify.weight") and key.startswith("disp_refinement."):
                t.mul_(CLASSIFY_GAIN)
    return module


def model(name, dtype=torch.float32):
    return seeded_model(DeepPrunerModel(name)).to(dtype).eval()


def inputs(name, dtype=torch.float32):
    """left ~ N(0, 1) (a normalised image), right = left moved 6 pixels to the left plus a tenth of fresh noise, and PatchMatch's
    noise [B, 12, h, w] in [0, 1)."""
    _, _, _, planes, (B, _, H, W), seed, _ = CASES[name]
    g = torch.Generator().manual_seed(seed)
    s = 2 << len(planes)
    left = torch.randn((B, 3, H, W), generator=g)
    right = torch.roll(left, -6, dims=3) + 0.1 * torch.randn((B, 3, H, W), generator=g)
    noise = torch.rand((B, PATCH_MATCH_SAMPLES - 2, H // s, W // s), generator=g)
    return tuple(t.to(dtype) for t in (left, right, noise))


def subsample(name, maps):
    sy, sx = CASES[name][6]
    return [m[:, :, ::sy, ::sx] for m in maps]


def recording():
    return np.load(GOLDEN)


_cache = {}


def fp32_outputs(name):
    """The FP32 restatement on the CPU (bit for bit the reference): computed once, shared, never modified."""
    if ("fp32", name) not in _cache:
        with torch.no_grad():
            _cache[("fp32", name)] = model(name)(*inputs(name))
    return _cache[("fp32", name)]


def decisions(z, name):
    """The recorded (flat indices, decisions) of the two volumes."""
    return tuple((torch.from_numpy(z["%s/%s_index" % (name, v)]), torch.from_numpy(z["%s/%s_decision" % (name, v)])) for v in ("pre", "post"))


def fp64_outputs(name, device="cpu", masks=None, tag="reference"):
    """The FP64 yardstick, evaluated on ``device`` and kept on the CPU: computed once per ``tag``, shared, never modified.
    ``masks`` None: the recorded decisions of the reference (what its own FP32 error is measured against); otherwise the whole
    masks of another FP32 evaluation, ``tag`` naming it (what THAT evaluation's error is measured against)."""
    if ("fp64", name, tag) not in _cache:
        with torch.no_grad():
            out = model(name, torch.float64).to(device)(*(t.to(device) for t in inputs(name, torch.float64)),
                                                        masks=decisions(recording(), name) if masks is None else masks)
        _cache[("fp64", name, tag)] = dict(disps=[t.cpu() for t in out["disps"]], min_disparity=out["min_disparity"].cpu(),
                                           max_disparity=out["max_disparity"].cpu(), masks=[m.cpu() for m in out["masks"]],
                                           targets=[t.cpu() for t in out["targets"]])
    return _cache[("fp64", name, tag)]
