"""Plain torch restatements of the reference's three loss classes, ``loss_per_level`` by ``loss_per_level``: the level scaling of
the ground truth, the pooling, the two masks of the focal loss and LaplaceDisp2Prob's target distribution.  Used as the yardstick
of tests/test_head_grads_gpu.py and pinned on the CPU against tests/golden/losses.npz (values and autograd gradients of the real
reference) by tests/test_oracle_golden.py.

Everything that decides WHICH pixels and samples take part -- the pooled and rescaled ground truth, the masks and the
``torch.linspace`` sample values -- is computed from the FP32 ground truth in FP32, exactly as the reference computes it, by the
``*_prep`` functions; the ``*_level`` functions then run the arithmetic after it in the dtype of their differentiable input.  An
FP64 and an FP32 evaluation of one case therefore share every mask pixel: a comparison between them measures arithmetic, never a
flipped mask."""
import torch
import torch.nn.functional as F


def level_gt(gt, hw, sparse, pooled=None):
    """(ground truth at a level's resolution, scale): stereo_focal_loss.py:66-73, conf_nll_loss.py:37-43, smooth_l1_loss.py:37-43.
    ``pooled``: the pooled map as another torch evaluation of the same pooling computed it (average pooling sums in an order of
    its own: a caller that compares with that evaluation passes its map, so that both see the same FP32 values)."""
    H, W = hw
    gt = gt.float()
    if gt.shape[-2] == H and gt.shape[-1] == W:
        return gt.clone(), 1.0
    scale = gt.shape[-1] / (W * 1.0)
    if pooled is not None:
        return pooled.float().clone(), scale
    pool = F.adaptive_max_pool2d if sparse else F.adaptive_avg_pool2d
    return pool(gt.clone() / scale, (H, W)), scale


def focal_prep(gt, cost_shape, max_disp, start_disp=0, dilation=1, sparse=False, pooled=None):
    """The FP32 inputs of one focal-loss level: masked ground truth, the loss mask m1, LaplaceDisp2Prob's mask m2, the samples."""
    B, C, H, W = cost_shape
    sg, scale = level_gt(gt, (H, W), sparse, pooled)
    md = int(max_disp / scale)                                             # stereo_focal_loss.py:79,89
    lower, upper = start_disp, start_disp + md
    m1 = ((sg > lower) & (sg < upper)).float()
    end = start_disp + md - 1
    n = (md + dilation - 1) // dilation
    samples = torch.linspace(start_disp, end, n)                           # disp2prob.py:118-126
    g = sg * m1
    m2 = ((g > start_disp) & (g < end)).float()                            # disp2prob.py:127-129
    return dict(g=g * m2, m1=m1, m2=m2, samples=samples, any=bool(m1.sum() >= 1.0))


def focal_level(cost, variance, prep, coefficient=0.0):
    """StereoFocalLoss.loss_per_level on prepared inputs; ``variance`` a float or a map broadcastable to [B, 1, H, W]."""
    dt = cost.dtype
    g, m1, m2 = prep["g"].to(dt), prep["m1"].to(dt), prep["m2"].to(dt)
    if not prep["any"]:
        prob = torch.zeros_like(cost)                                      # stereo_focal_loss.py:84-86
    else:
        s = prep["samples"].to(dt).view(1, -1, 1, 1)
        prob = F.softmax(-torch.abs(s - g) / variance, dim=1) * m2 + 1e-40
    log_q = F.log_softmax(cost, dim=1)
    weight = (1.0 - prob).pow(-coefficient)
    return -((prob * log_q) * weight * m1).sum() / m1.sum().clamp(min=1.0)


def map_prep(gt, hw, max_disp, start_disp=0, sparse=False, pooled=None):
    """(scaled ground truth, mask) of ConfidenceNllLoss / DispSmoothL1Loss: the upper bound is max_disp / scale, not truncated."""
    sg, scale = level_gt(gt, hw, sparse, pooled)
    return sg, (sg > start_disp) & (sg < (max_disp / scale))


def nll_level(logit, sg, mask):
    m = mask.to(logit.dtype)
    return (-1.0 * F.logsigmoid(logit) * m).sum() / m.sum().clamp(min=1.0)


def smooth_l1_level(est, sg, mask):
    sg = sg.to(est.dtype)
    if mask.sum() < 1.0:
        return (torch.abs(est - sg) * mask.to(est.dtype)).mean()
    return F.smooth_l1_loss(est[mask], sg[mask], reduction="mean")
