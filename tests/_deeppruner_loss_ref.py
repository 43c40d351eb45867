"""The training tail of the reference's DeepPruner model in plain torch, any dtype, with autograd: models/DeepPruner.py:82-108 (the
K + 2 maps brought to the image size with (d * W) / w and F.interpolate, the two range maps rescaled and interpolated a second
time), losses/smooth_l1_loss.py:35-58 at full size (scale 1) and losses/utils/quantile_loss.py:25-37 on the un-rescaled range maps.
It is what the GPU tests differentiate on the CPU (FP32 and FP64), and scripts/gen_golden_deeppruner_loss.py asserts that its FP32
run equals the real reference bit for bit, losses and gradients, before it records tests/golden/deeppruner_loss.npz.

The seeded cases: the ground truth is a smooth field spanning about (-40, 255), so several per cent fall outside (0, 192) on each
side, with a sprinkling of exact zeros (KITTI-style invalid pixels); every map is the pooled ground truth in its own units plus
noise scaled so that |v - gt| < 1 and > 1 both occur and gt - Mn, gt - Mx take both signs."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deeppruner_loss.npz")
MAX_DISP = 192

# name -> (image size, list sizes (better first), range map size, batch, l1 weights, theta, seed).  The first two are recorded from
# the reference with the two shipped configs' own weights and theta; the others are the awkward shapes of the GPU tests.
CASES = {
    "4x": ((64, 96), [(32, 48), (16, 24)], (16, 24), 1, (1.3, 1.0, 0.7, 0.7), 0.05, 401),
    "8x": ((64, 96), [(32, 48), (16, 24), (8, 12)], (8, 12), 2, (1.6, 1.3, 1.0, 0.7, 0.7), 0.05, 402),
    "one_pixel_maps": ((4, 4), [(1, 1), (1, 1), (1, 1)], (1, 1), 1, (1.6, 1.3, 1.0, 0.7, 0.7), 0.05, 403),
    "odd_ratios": ((12, 20), [(12, 20), (5, 9)], (3, 5), 1, (1.3, 1.0, 0.7, 0.7), 0.05, 404),
    "partial_tiles": ((24, 72), [(12, 36), (6, 18)], (6, 18), 2, (1.3, 1.0, 0.7, 0.7), 0.05, 405),
    "k1": ((16, 40), [(8, 20)], (4, 10), 1, (1.0, 0.7, 0.7), 0.2, 406),
}
RECORDED = ("4x", "8x")


def settings(name):
    """The two loss nodes and the data node ``DeepPrunerLoss`` reads, as a plain dict."""
    _, _, _, _, weights, theta, _ = CASES[name]
    return dict(model=dict(losses=dict(l1_loss=dict(max_disp=MAX_DISP, weights=tuple(weights), weight=1.0),
                                       quantile_loss=dict(max_disp=MAX_DISP, theta=theta, weight=1.0))),
                data=dict(sparse=False))


def inputs(name, dtype=torch.float32, empty=False):
    """(disps, min_disparity, max_disparity, gt) on the CPU, generated in FP32 from the case's seed.  ``empty``: a ground truth with
    no pixel inside (0, 192)."""
    (H, W), sizes, (h, w), B, _, _, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    coarse = torch.rand((B, 1, max(2, H // 16), max(2, W // 16)), generator=g) * 300 - 45
    smooth = F.interpolate(coarse, size=(H, W), mode='bilinear', align_corners=True)
    gt = torch.where(torch.rand((B, 1, H, W), generator=g) < 0.03, torch.zeros(()), smooth)
    if empty:
        gt = -1.0 - gt.abs()

    def pooled(size, shift, spread):
        # in the map's own units: the model's maps hold disparities at their resolution, (d * W) / w brings them to the image's
        noise = shift + spread * torch.randn((B, 1) + tuple(size), generator=g)
        return (F.adaptive_avg_pool2d(smooth, size) + noise) * (size[1] / W)   # (pooled before the zeros went in)

    disps = [pooled(s, 0.0, 1.0) for s in sizes]
    lo, hi = pooled((h, w), -1.0, 2.5), pooled((h, w), 1.0, 2.5)
    return [d.to(dtype) for d in disps], lo.to(dtype), hi.to(dtype), gt.to(dtype)


def up(d, size):
    """models/DeepPruner.py:83-94: (d * W) / w, then the half-pixel bilinear interpolation."""
    H, W = size
    return F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=False)


def smooth_l1_level(est, gt, lower, upper):
    """smooth_l1_loss.py:35-58 for a map at the ground truth's size (scale = 1)."""
    mask = (gt > lower) & (gt < upper)
    if mask.sum() < 1.0:
        return (torch.abs(est - gt) * mask.to(est.dtype)).mean()
    return F.smooth_l1_loss(est[mask], gt[mask], reduction='mean')


def quantile_terms(mn, mx, gt, lower, upper, theta):
    """quantile_loss.py:25-37, the two means before they are added."""
    mask = (gt > lower) & (gt < upper)
    min_mask = ((gt[mask] - mn[mask]) < 0).to(mn.dtype)
    min_loss = ((gt[mask] - mn[mask]) * (theta - min_mask)).mean()
    max_mask = ((gt[mask] - mx[mask]) < 0).to(mx.dtype)
    max_loss = ((gt[mask] - mx[mask]) * ((1 - theta) - max_mask)).mean()
    return min_loss, max_loss


def full_maps(disps, lo, hi, size):
    """The K + 2 maps handed to DispSmoothL1Loss (:93-94) and the un-rescaled range maps handed to quantile_loss (:87-92)."""
    Mn, Mx = up(lo, size), up(hi, size)
    return [up(d, size) for d in list(disps) + [Mn, Mx]], Mn, Mx


def terms(disps, lo, hi, gt, theta, l1=(0, MAX_DISP), q=(0, MAX_DISP)):
    """The K + 4 unweighted terms: K + 2 smooth-L1 levels, then the two quantile means."""
    full, Mn, Mx = full_maps(disps, lo, hi, gt.shape[-2:])
    return [smooth_l1_level(m, gt, *l1) for m in full] + list(quantile_terms(Mn, Mx, gt, q[0], q[1], theta))


def loss_dict(name, disps, lo, hi, gt):
    """The reference's ``loss_dict`` (:99-109): quantile_loss, then l1_loss_lvl0 .. l1_loss_lvl{K+1}, with the case's weights."""
    _, _, _, _, weights, theta, _ = CASES[name]
    t = terms(disps, lo, hi, gt, theta)
    K = len(disps)
    out = dict(quantile_loss=(t[K + 2] + t[K + 3]) * 1.0)
    for i in range(K + 2):
        out["l1_loss_lvl{}".format(i)] = weights[i] * t[i] * 1.0
    return out


def coefficients(n):
    """Distinct, non-trivial weights for the scalar that is differentiated: a swapped or dropped term shows."""
    return [0.6 + 0.35 * i - 0.05 * i * i for i in range(n)]


def total(losses):
    """sum_i c_i * loss_i over a loss dict (in its order) or a list of terms."""
    values = list(losses.values()) if isinstance(losses, dict) else list(losses)
    out = 0
    for c, v in zip(coefficients(len(values)), values):
        out = out + c * v
    return out


def run(name, dtype, empty=False):
    """(loss dict values, gradients of ``total`` with respect to the K list maps, min and max) of the restatement on the CPU."""
    disps, lo, hi, gt = inputs(name, dtype, empty)
    leaves = [t.requires_grad_() for t in disps + [lo, hi]]
    d = loss_dict(name, leaves[:-2], leaves[-2], leaves[-1], gt)
    total(d).backward()
    return [v.detach() for v in d.values()], [t.grad for t in leaves]


def branch_fractions(name):
    """Of the valid pixels, the share on each side of every branch: |v - gt| < 1 per smooth-L1 level, gt - M < 0 per range map;
    and the share of pixels each mask excludes."""
    disps, lo, hi, gt = inputs(name)
    full, Mn, Mx = full_maps(disps, lo, hi, gt.shape[-2:])
    mask = (gt > 0) & (gt < MAX_DISP)
    out = [((m - gt).abs() < 1)[mask].float().mean().item() for m in full]
    out += [((gt - m) < 0)[mask].float().mean().item() for m in (Mn, Mx)]
    return out, 1.0 - mask.float().mean().item(), (gt <= 0).float().mean().item(), (gt >= MAX_DISP).float().mean().item()


def recording():
    return np.load(GOLDEN)
