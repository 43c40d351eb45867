"""DeepPrunerLoss: the training losses of the DeepPruner model (dmb/modeling/stereo/models/DeepPruner.py:82-108) on
csrc/deeppruner_loss.hip.  The reference up-samples the K + 2 maps to the image size, rescales the two range maps a second time,
runs DispSmoothL1Loss over the K + 2 full-size maps and quantile_loss over the un-rescaled range maps; here the maps stay as the
model holds them before line 82 and one fused forward (and, on ``.backward()``, one fused backward) does all of it."""
import torch

from .... import ops_deeppruner


class DeepPrunerLossTerms(torch.autograd.Function):
    """[K + 4] means: the K + 2 smooth-L1 levels, then the two quantile terms (ops_deeppruner.deeppruner_loss_fwd)."""

    @staticmethod
    def forward(ctx, gt, bounds, min_disp, max_disp, *disps):
        out, stats = ops_deeppruner.deeppruner_loss_fwd(list(disps), min_disp, max_disp, gt, *bounds)
        ctx.save_for_backward(gt, min_disp, max_disp, stats, *disps)
        ctx.bounds = bounds
        return out

    @staticmethod
    def backward(ctx, grad_out):
        gt, min_disp, max_disp, stats = ctx.saved_tensors[:4]
        disps = list(ctx.saved_tensors[4:])
        g_disps, g_min, g_max = ops_deeppruner.deeppruner_loss_bwd(disps, min_disp, max_disp, gt, stats,
                                                                  grad_out.float().contiguous(), *ctx.bounds)
        return (None, None, g_min, g_max) + tuple(g_disps)


class DeepPrunerLoss(object):
    """``loss(disps, min_disparity, max_disparity, target)`` -> the reference's ``loss_dict``: ``quantile_loss``, then
    ``l1_loss_lvl0 .. l1_loss_lvl{K+1}``, weighted as CombinedLossEvaluators and DispSmoothL1Loss weight them.  ``disps`` is the
    refinement's list (better first, the last one the cost processor's own disparity), the range maps are the confidence range
    predictor's, all at their own resolution; ``target`` is the full-size ground truth [B, 1, H, W]."""

    def __init__(self, cfg):
        losses = cfg.model.losses
        l1, quantile = losses.get("l1_loss", None), losses.get("quantile_loss", None)
        if l1 is None or quantile is None:
            raise ValueError("DeepPrunerLoss: cfg.model.losses needs the l1_loss and the quantile_loss node")
        if l1.get("max_disp", None) is None or quantile.get("max_disp", None) is None:
            raise ValueError("DeepPrunerLoss: both loss nodes need max_disp")
        if cfg.data.sparse:
            # DispSmoothL1Loss pools the ground truth (max for sparse) only below full size; the maps here are compared at full size
            raise NotImplementedError("DeepPrunerLoss: data.sparse=True is not built: the full-size path never pools the ground "
                                      "truth, so the flag would be ignored")
        self.l1_lower, self.l1_upper = 0.0, float(l1.max_disp)        # make_sll_loss_evaluator: start_disp stays 0, scale is 1
        self.weights, self.l1_weight = [float(v) for v in l1.weights], l1.weight
        self.q_lower = float(quantile.get("start_disp", 0))
        self.q_upper = self.q_lower + float(quantile.max_disp)
        self.q_weight, self.theta = quantile.get("weight", 1.0), float(quantile.get("theta", 0.05))
        if not 0.0 < self.theta < 1.0:
            raise ValueError("DeepPrunerLoss: theta must lie inside (0, 1), got %r" % (self.theta,))

    def __call__(self, disps, min_disparity, max_disparity, target):
        disps = list(disps)
        K = len(disps)
        if len(self.weights) != K + 2:
            raise ValueError("DeepPrunerLoss: %d l1 weights for %d maps in the list and the two range maps" % (len(self.weights), K))
        bounds = (self.l1_lower, self.l1_upper, self.q_lower, self.q_upper, self.theta)
        terms = DeepPrunerLossTerms.apply(target.detach(), bounds, min_disparity, max_disparity, *disps)
        loss_dict = dict(quantile_loss=(terms[K + 2] + terms[K + 3]) * self.q_weight)
        for i in range(K + 2):
            loss_dict["l1_loss_lvl{}".format(i)] = (self.weights[i] * terms[i]) * self.l1_weight
        return loss_dict
