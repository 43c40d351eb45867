"""cost_processors/AnyNet.py:8-86: per stage, the difference volume of fast_dif_fms on disparity samples (linspace, shifted by
the up-sampled disparity of the previous stage) and the stage's AnyNetAggregator.  The 1-D samples of each stage are kept on the
device (made once per device, never copied from the host per call); the per-pixel samples of the warp stages come from ONE
launch (dmb_anynet_stage_samples_f32) that also yields the up-sampled disparity the model adds back (models/AnyNet.py:84)."""
import torch
import torch.nn as nn

from .... import ops
from ..layers.preact import refuse_grad
from .aggregators.AnyNet import AnyNetAggregator


class AnyNetProcessor(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg.copy()
        self.batch_norm = cfg.model.batch_norm
        self.stage = self.cfg.model.stage
        cc = self.cfg.model.cost_processor.cost_computation
        self.max_disp, self.start_disp, self.dilation = cc.max_disp, cc.start_disp, cc.dilation
        agg = self.cfg.model.cost_processor.cost_aggregator
        self.aggregator_type = agg.type
        self.aggregator = nn.ModuleDict()
        for st in self.stage:
            self.aggregator[st] = AnyNetAggregator(in_planes=agg.in_planes[st], agg_planes=agg.agg_planes[st], num=agg.num,
                                                   batch_norm=self.batch_norm)
        self._lin = {}

    def samples(self, stage, device):
        """torch.linspace(start, end, D) of the stage (cost_processors/AnyNet.py:55-62), on ``device``."""
        key = (stage, str(device))
        t = self._lin.get(key)
        if t is None:
            D = (self.max_disp[stage] + self.dilation[stage] - 1) // self.dilation[stage]
            end = self.start_disp[stage] + self.max_disp[stage] - 1
            t = self._lin[key] = torch.linspace(self.start_disp[stage], end, D).float().to(device)
        return t

    def cost(self, stage, left, right, disp_sample):
        """fast_dif_fms + the stage's aggregator: [[B, D, H, W]]."""
        raw_cost = ops.fast_dif_fms(left, right, disp_sample)
        return self.aggregator[stage](raw_cost)

    def forward(self, stage, left, right, disp=None):
        refuse_grad(self, left, right, disp)
        lin = self.samples(stage, left.device)
        if disp is None:
            return self.cost(stage, left, right, lin)
        H, W = left.shape[-2:]
        _, samples = ops.anynet_stage_samples(disp, (H, W), W / disp.shape[-1], lin)
        return self.cost(stage, left, right, samples)
