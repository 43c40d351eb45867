"""DeepPruner (models/DeepPruner.py:13-122 of the reference): differentiable PatchMatch prunes the disparity range per pixel, a
small 3-D network aggregates the pruned volume, one or two refinement stages bring the map to full resolution.  Eval-mode
contract only: the training branch and the quantile loss are not built.

The module tree and ``state_dict`` keys are the reference's (backbone, cost_processor, disp_refinement; the sampler has no
parameters).  The class is reached by import -- ``build_model`` and the registries keep refusing the DeepPruner configs, the
cost processor is constructed directly (its builder stays refused) -- and ``apis.init_model`` dispatches to it for serving.
The forward is the reference's sequence on the four merged slices (docs/design/14 - 17) and adds no arithmetic of its own but
its output tail, ONE launch of csrc/deeppruner_final_maps.hip for the K + 4 output maps (docs/design/18).

``batch['patchMatchNoise']`` [B, P, h, w] (P = patch_match_disparity_sample_number - 2, feature size), optional: PatchMatch's
initial noise, passed to the sampler as it is.  Absent, the sampler draws it from torch's device generator."""
import torch
import torch.nn as nn

from .... import ops_deeppruner
from ..backbones import build_backbone
from ..cost_processors.DeepPruner import DeepPrunerProcessor
from ..disp_refinement import build_disp_refinement
from ..disp_samplers import build_disp_sampler

_NO_BACKWARD = ("DeepPruner on the HIP path is inference-only (no backward: PatchMatch, the stride-(1, 2, 2) 3-D kernels and the "
                "fused heads have none); call eval() and run under torch.no_grad() (as init_model / inference_stereo do)")


class DeepPruner(nn.Module):
    def __init__(self, cfg, backbone="auto"):
        super().__init__()
        if backbone is None or not (isinstance(backbone, str) and backbone in ("auto", "hip")):
            raise NotImplementedError("DeepPruner has no cost-path-alone form: its refinement is guided by the backbone's "
                                      "low-level feature maps; build it with backbone='auto'")
        if cfg.model.meta_architecture != "DeepPruner":
            raise NotImplementedError("DeepPruner: cfg.model.meta_architecture is %r" % (cfg.model.meta_architecture,))
        self.cfg = cfg.copy()
        self.max_disp = cfg.model.max_disp
        self.backbone = build_backbone(cfg)
        self.disp_sampler = build_disp_sampler(cfg)
        self.cost_processor = DeepPrunerProcessor(cfg)
        self.disp_refinement = build_disp_refinement(cfg)
        if self.disp_refinement.num not in (1, 2):
            raise NotImplementedError("DeepPruner: one refinement stage (features at 1/4) or two (1/8), got %r"
                                      % (self.disp_refinement.num,))
        # the features' down-sampling: every refinement stage doubles the processor's map, which is twice the features' size
        self.down_sample = 2 << self.disp_refinement.num

    def _check(self, ref_img, tgt_img, noise):
        """Everything that can be refused is refused here, before any launch."""
        if self.training:
            raise NotImplementedError(_NO_BACKWARD)
        if torch.is_grad_enabled() and (any(isinstance(t, torch.Tensor) and t.requires_grad for t in (ref_img, tgt_img, noise))
                                        or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError(_NO_BACKWARD)
        if ref_img.dim() != 4 or ref_img.shape != tgt_img.shape:
            raise ValueError("DeepPruner: leftImage and rightImage must be [B, 3, H, W] of one shape, got %s and %s"
                             % (tuple(ref_img.shape), tuple(tgt_img.shape)))
        B, _, H, W = ref_img.shape
        s = self.down_sample
        # a multiple of s for the backbone's maps to meet the refined ones (the reference fails in torch.cat otherwise), of 8 * s
        # for the three stride-(1, 2, 2) levels of the hourglasses (the reference fails in their skip adds)
        if H % (8 * s) or W % (8 * s):
            raise ValueError("DeepPruner: H and W must be multiples of %d (features at 1/%d, hourglasses of three stride-2 "
                             "levels on them), got %dx%d" % (8 * s, s, H, W))
        if noise is not None:
            shape = (B, self.disp_sampler.patch_match_disparity_sample_number - 2, H // s, W // s)
            if not isinstance(noise, torch.Tensor) or tuple(noise.shape) != shape or noise.dtype != torch.float32 \
                    or noise.device != ref_img.device:
                raise ValueError("DeepPruner: patchMatchNoise must be a float32 tensor %s on %s, got %s" % (
                    shape, ref_img.device, "%s %s on %s" % (noise.dtype, tuple(noise.shape), noise.device)
                    if isinstance(noise, torch.Tensor) else type(noise).__name__))

    def forward(self, batch):
        ref_img, tgt_img = batch['leftImage'], batch['rightImage']
        noise = batch.get('patchMatchNoise')
        self._check(ref_img, tgt_img, noise)
        # :43-48: (feature, [low-level maps, coarse first]) per view
        (ref_fms, low_ref_group_fms), (tgt_fms, _) = self.backbone(ref_img, tgt_img)
        # :54-60: PatchMatch over the full range, then the confidence range predictor
        disparity_sample = self.disp_sampler('pre', ref_fms, tgt_fms, noise=noise)
        min_disparity, max_disparity, min_disparity_feature, max_disparity_feature = self.cost_processor(
            'pre', ref_fms, tgt_fms, disparity_sample)
        # :64-72: uniform samples inside the predicted range, then the aggregator
        disparity_sample = self.disp_sampler('post', ref_fms, tgt_fms, min_disparity=min_disparity, max_disparity=max_disparity)
        disparity, disparity_feature = self.cost_processor('post', ref_fms, tgt_fms, disparity_sample,
                                                           min_disparity_feature, max_disparity_feature)
        # :78-79: the first stage's guide also carries the disparity feature
        guides = [torch.cat((low_ref_group_fms[0], disparity_feature), dim=1)] + list(low_ref_group_fms[1:])
        disps = self.disp_refinement([disparity], guides)
        # :82-94, 115: every map at full resolution, the rescaled range maps and the two range residuals, one launch
        disps = ops_deeppruner.deeppruner_final_maps(disps, min_disparity, max_disparity, ref_img.shape[-2:])
        return dict(disps=disps, costs=[None]), {}
