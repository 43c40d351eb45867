"""AnyNet (models/AnyNet.py:12-147 of the reference): anytime stereo, three coarse-to-fine stages on the AnyNet backbone's three
feature scales and an SPN refinement, eval-mode contract only.

The module tree and ``state_dict`` keys are the reference's (backbone, cost_processor.aggregator.<stage>, disp_predictor.<stage>,
disp_refinement); the parts are constructed here directly, not through the registries: AnyNet's stages interleave with its
backbone's feature scales and its refinement reads the image, so it has no "cost path alone" form (``backbone=None`` refuses).
One eval forward at batch 1 is 51 launches and no host synchronisation: 14 for the backbone (both views at once), 8 + 10 + 10
for the stages (the up-sampled coarse disparity is computed ONCE per warp stage and serves both the samples and the combined
map), 8 for the refinement and 1 for the 7 output maps.  Training is not built: train() mode or anything that can receive a
gradient raises NotImplementedError."""
import torch
import torch.nn as nn

from .... import ops
from ..backbones.AnyNet import AnyNetBackbone
from ..cost_processors.AnyNet import AnyNetProcessor
from ..disp_predictors.faster_soft_argmin import FasterSoftArgmin
from ..disp_refinement.AnyNet import AnyNetRefinement


class AnyNet(nn.Module):
    def __init__(self, cfg, backbone="auto"):
        super().__init__()
        if backbone is None or not (isinstance(backbone, str) and backbone in ("auto", "hip")):
            raise NotImplementedError("AnyNet has no cost-path-alone form: its stages interleave with its backbone's three "
                                      "feature scales and its refinement reads the image; build it with backbone='auto'")
        self.cfg = cfg.copy()
        self.max_disp = cfg.model.max_disp
        self.stage = cfg.model.stage
        bb = cfg.model.backbone
        if bb.type != "AnyNet" or cfg.model.cost_processor.type != "AnyNet" or cfg.model.disp_refinement.type != "AnyNet":
            raise NotImplementedError("AnyNet: backbone, cost_processor and disp_refinement must all be of type 'AnyNet'")
        self.backbone = AnyNetBackbone(in_planes=bb.in_planes, C=bb.C, block_num=bb.block_num, batch_norm=cfg.model.batch_norm)
        self.cost_processor = AnyNetProcessor(cfg)
        dp = cfg.model.disp_predictor
        self.disp_predictor = nn.ModuleDict()
        for st in self.stage:
            self.disp_predictor[st] = FasterSoftArgmin(max_disp=dp.max_disp[st], start_disp=dp.start_disp[st],
                                                       dilation=dp.dilation[st], alpha=dp.alpha, normalize=dp.normalize)
        rf = cfg.model.disp_refinement
        self.disp_refinement = AnyNetRefinement(in_planes=rf.in_planes, spn_planes=rf.spn_planes,
                                                batch_norm=cfg.model.batch_norm)
        if list(self.stage) != ['init_guess', 'warp_level_8', 'warp_level_4']:
            raise NotImplementedError("AnyNet: stages init_guess, warp_level_8, warp_level_4 (models/AnyNet.py:53-106)")

    def forward(self, batch):
        ref_img, tgt_img = batch['leftImage'], batch['rightImage']
        if self.training:
            raise NotImplementedError("AnyNet on the HIP path is inference only (its backward is not built); call eval()")
        if torch.is_grad_enabled() and (ref_img.requires_grad or tgt_img.requires_grad
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("AnyNet on the HIP path has no backward; run it under torch.no_grad() (as init_model / "
                                      "inference_stereo do)")
        B = ref_img.shape[0]
        f16, f8, f4 = self.backbone.features(ref_img, tgt_img)
        proc, pred = self.cost_processor, self.disp_predictor
        # initial guess at 1/16 (:53-61): 1-D samples
        costs_init = proc.cost('init_guess', f16[:B], f16[B:], proc.samples('init_guess', ref_img.device))
        d_init = pred['init_guess'](costs_init[0])
        # warp stages (:64-104): up = interpolate(low * W / w) once, for the samples and for up + residual
        low, lows = d_init, []
        costs = []
        for st, fms in (('warp_level_8', f8), ('warp_level_4', f4)):
            H, W = fms.shape[-2:]
            up, samples = ops.anynet_stage_samples(low, (H, W), W / low.shape[-1], proc.samples(st, ref_img.device))
            cost = proc.cost(st, fms[:B], fms[B:], samples)
            low = ops.add(up, pred[st](cost[0]))
            lows.append(low)
            costs.append(cost)
        d8, d4 = lows
        # refinement (:108-111), then all maps at full resolution and the residual maps (:114-147), one launch
        refined, _ = self.disp_refinement([d4], f4[:B], f4[B:], ref_img, tgt_img)
        disps = ops.anynet_final_maps([refined, d4, d8, d_init], ref_img.shape[-2:])
        return dict(disps=disps, costs=costs[1] + costs[0] + costs_init), {}
