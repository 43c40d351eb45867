"""quantile_loss: drop-in for dmb/modeling/stereo/losses/utils/quantile_loss.py:5-41 on csrc/deeppruner_loss.hip's elementwise pair.
The reference indexes four times with a boolean mask (a ``nonzero`` and a synchronisation each); here the masked means are one
launch plus the finalising block, and the backward one launch, so a step that holds it can be captured in a graph."""
import torch

from ..... import ops_deeppruner


class QuantileTerms(torch.autograd.Function):
    """(mean (gt - min) * (theta - [gt - min < 0]), mean (gt - max) * ((1 - theta) - [gt - max < 0])) under lower < gt < upper."""

    @staticmethod
    def forward(ctx, min_disp, max_disp, gt, lower, upper, theta):
        out, stats = ops_deeppruner.quantile_loss_fwd(min_disp, max_disp, gt, lower, upper, theta)
        ctx.save_for_backward(min_disp, max_disp, gt, stats)
        ctx.args = (lower, upper, theta)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        min_disp, max_disp, gt, stats = ctx.saved_tensors
        g_min, g_max = ops_deeppruner.quantile_loss_bwd(min_disp, max_disp, gt, stats, grad_out.float().contiguous(), *ctx.args)
        return g_min, g_max, None, None, None, None


def quantile_loss(minEstDisp, maxEstDisp, gtDisp, max_disp, start_disp=0, weight=1.0, theta=0.05):
    """Both maps and ``gtDisp`` are [B, 1, H, W] of one size; returns the 0-dim (min term + max term) * weight.  Gradients go to
    the two maps, none to ``gtDisp``.  An empty mask gives NaN, as the mean of an empty tensor does, with zero gradients."""
    if not 0.0 < float(theta) < 1.0:
        raise ValueError("quantile_loss: theta must lie inside (0, 1), got %r" % (theta,))
    if not (tuple(minEstDisp.shape) == tuple(maxEstDisp.shape) == tuple(gtDisp.shape)):
        raise ValueError("quantile_loss: the two maps and the ground truth must have one shape, got %s, %s and %s"
                         % (tuple(minEstDisp.shape), tuple(maxEstDisp.shape), tuple(gtDisp.shape)))
    terms = QuantileTerms.apply(minEstDisp, maxEstDisp, gtDisp.detach(), float(start_disp), float(start_disp + max_disp), float(theta))
    return (terms[0] + terms[1]) * weight
