"""The hand-placed inputs of tests/test_value_edges_gpu.py and their CPU references: values that sit exactly on a decision of a
kernel.  Every construction is exact in FP32; tests/test_value_edges_host.py checks that on the CPU."""
import functools
import math

import numpy as np
import torch

from oracle import dmb_oracle as O
from tests import _deeppruner_loss_ref as R

MAP = (2, 1, 8, 64)


def nxt(v, up=True):
    """The FP32 neighbour of v."""
    return float(np.nextafter(np.float32(v), np.float32(math.inf if up else -math.inf)))


def around(v):
    return (nxt(v, False), float(v), nxt(v, True))


# ---------------------------------------------------------------------------------------------- 1. end-point error
EPE_BOUNDS = (0.0, 192.0)
EPE_ORIGINAL = (6, 60)        # of 8 x 64 maps: the two top rows and the four right columns are padding


def epe_pairs():
    """(gt, est) pairs with |gt - est| exactly 1, 2, 3, 5 or an FP32 neighbour of those, the estimate on either side.  gt lies in the
    binade of the error, so gt -/+ err is representable and the FP32 difference is exact (10 - 1.0000001 would not be)."""
    out = []
    for T in (1.0, 2.0, 3.0, 5.0):
        for err in around(T):
            top = 2.0 ** math.floor(math.log2(err) + 1)          # the end of err's binade
            cands = [(top * 0.75, top * 0.75 - err), (top * 0.5 + err, top * 0.5)]             # estimate below ...
            cands += [(E - err, E) for E in (top * 0.75, top * 1.5)]                           # ... and above (FP64: exact)
            for gt, est in cands:
                if gt > 0 and float(np.float32(gt)) == gt and float(np.float32(est)) == est:
                    out.append((gt, est, err))
    return out


@functools.lru_cache(maxsize=None)
def epe_case():
    """(ests, gt): two 8 x 64 images and three estimates.  Image 0: threshold pairs, gt on lb and ub and their inner neighbours,
    in-range pixels with ordinary errors; image 1: its ONLY in-range pixels sit on thresholds.  The padding holds in-range pixels
    with large errors: counting them shows.  Estimates 1 and 2 are estimate 0 with the pixels off the threshold pairs moved by exactly +/- 0.5."""
    lb, ub = EPE_BOUNDS
    pairs = epe_pairs()
    H, W = MAP[-2:]
    H0, W0 = EPE_ORIGINAL
    gt = torch.full(MAP, -1.0)
    est = torch.zeros(MAP)
    inside = [(r, c) for r in range(H - H0, H) for c in range(W0)]
    for b in range(2):
        for k, (g, e, _) in enumerate(pairs):
            r, c = inside[(k * 7 + 3 * b) % len(inside)] if b == 0 else inside[k]
            gt[b, 0, r, c], est[b, 0, r, c] = g, e
    taken = gt[0, 0] != -1.0
    edge = [lb, ub, 2.0 ** -126, nxt(ub, False), 100.0, 17.25, 191.0, 0.5]
    free = [(r, c) for (r, c) in inside if not taken[r, c]]
    for k, g in enumerate(edge * 4):
        r, c = free[k * 5]
        gt[0, 0, r, c], est[0, 0, r, c] = g, g + (k % 5) * 0.75 - 1.5
    gt[:, :, :H - H0, :] = 50.0          # the padding: in range, error 50
    gt[:, :, :, W0:] = 50.0
    # the other estimates: the threshold pairs kept, every other pixel (multiples of 0.25) moved by exactly +/- 0.5
    on_pair = torch.zeros(MAP, dtype=torch.bool)
    for b in range(2):
        for k in range(len(pairs)):
            r, c = inside[(k * 7 + 3 * b) % len(inside)] if b == 0 else inside[k]
            on_pair[b, 0, r, c] = True
    ests = [est, torch.where(on_pair, est, est + 0.5), torch.where(on_pair, est, est - 0.5)]
    return ests, gt


def epe_expected(est, gt):
    """The six accumulator entries after one update of a zero accumulator, in FP64 and in the kernel's order of operations:
    images, then sums over the images of mean error and 100 * count / valid."""
    lb, ub = EPE_BOUNDS
    H0, W0 = EPE_ORIGINAL
    tot = [0.0] * 6
    for b in range(gt.shape[0]):
        g = O.remove_padding(gt[b:b + 1], EPE_ORIGINAL)
        e = O.remove_padding(est[b:b + 1], EPE_ORIGINAL)
        m = (g > lb) & (g < ub)
        a = (g[m] - e[m]).abs()                  # FP32, as the kernel and the reference take it
        cnt = float(m.sum())
        tot[0] += 1.0
        if cnt >= 1.0:
            tot[1] += float(a.double().sum()) / cnt
            for i, k in enumerate((1, 2, 3, 5)):
                tot[2 + i] += 100.0 * float((a > k).sum()) / cnt
    return tot


# ---------------------------------------------------------------------------------------------- 2., 3. the map losses
MAP_BOUNDS = (0.0, 192.0)


@functools.lru_cache(maxsize=None)
def smooth_l1_case():
    """(x, gt): |x - gt| at 0, at 1 and its neighbours (either sign), ordinary values elsewhere; gt on lower and on upper."""
    vals, gts = [], []
    for d in (0.0,) + around(1.0):
        vals.append(1.5 - d), gts.append(1.5)        # the map below the ground truth: 1.5 - d is exact (the binade of 1)
        vals.append(1.5), gts.append(1.5 - d)        # ... and above it
    for g in (MAP_BOUNDS[0], MAP_BOUNDS[1], 2.0 ** -126, nxt(MAP_BOUNDS[1], False)):
        vals.append(g + 0.75), gts.append(g)
    gen = torch.Generator().manual_seed(41)
    gt = torch.rand(MAP, generator=gen) * 220 - 10
    x = gt + torch.randn(MAP, generator=gen) * 1.5
    n = len(vals)
    x.view(-1)[3:3 + n] = torch.tensor(vals)
    gt.view(-1)[3:3 + n] = torch.tensor(gts)
    return x, gt


LOGITS = (0.0, 20.0, -20.0, 88.0, -88.0, 89.0, -89.0, 100.0, -100.0)


@functools.lru_cache(maxsize=None)
def nll_case():
    """(logits, gt): 0, +/-20 and either side of where exp leaves FP32 (+/-88, +/-89, +/-100), each under a valid and a masked gt."""
    gen = torch.Generator().manual_seed(42)
    gt = torch.rand(MAP, generator=gen) * 220 - 10
    x = torch.randn(MAP, generator=gen) * 3
    for k, v in enumerate(LOGITS * 3):
        x.view(-1)[5 + k] = v
        gt.view(-1)[5 + k] = (7.0, MAP_BOUNDS[0], MAP_BOUNDS[1])[k // len(LOGITS)]
    return x, gt


def map_loss_reference(x, gt, mode, dtype):
    """(loss, d loss / d x) of the reference's ConfidenceNllLoss (mode 0) / DispSmoothL1Loss (mode 1) in ``dtype``."""
    xl = x.to(dtype).requires_grad_(True)
    fn = O.conf_nll_loss if mode == 0 else O.disp_smooth_l1_loss
    loss = fn(xl, gt.to(dtype), MAP_BOUNDS[1], MAP_BOUNDS[0])
    g, = torch.autograd.grad(loss, xl)
    return loss.detach(), g


# ---------------------------------------------------------------------------------------------- 4. the focal loss
FOCAL_D = 8


def focal_geometry(start):
    """(lower, upper, start_disp, end_disp, samples) of a StereoFocalLoss level with max_disp = 8."""
    return float(start), float(start + FOCAL_D), float(start), float(start + FOCAL_D - 1), [float(start + k) for k in range(FOCAL_D)]


@functools.lru_cache(maxsize=None)
def focal_case(start, variances):
    """(cost, gt, variance map): gt on lower (= start_disp), upper, end_disp and their inner neighbours, on samples, halfway between
    samples, on 0; the variance map cycles through ``variances`` at another period than the ground truth."""
    lower, upper, s0, s1, samples = focal_geometry(start)
    special = [lower, upper, s1, nxt(lower), nxt(s1, False), nxt(upper, False), 0.0, lower - 2.0, upper + 3.0]
    special += samples[1:-1] + [s + 0.5 for s in samples[:-1]] + [samples[2] + 0.25]
    gen = torch.Generator().manual_seed(43 + int(start))
    cost = torch.randn((2, FOCAL_D, 8, 64), generator=gen) * 2
    gt = torch.rand(MAP, generator=gen) * (FOCAL_D + 4) + start - 2
    n = len(special)
    for rep in range(len(variances) + 1):
        gt.view(-1)[rep * n:(rep + 1) * n] = torch.tensor(special)
    var = torch.tensor([variances[i % len(variances)] for i in range(gt.numel())], dtype=torch.float32).view(MAP)
    return cost, gt, var


def focal_reference(cost, gt, variance, start, fc, dtype):
    """(loss, d / d cost, d / d variance or None) of O.stereo_focal_loss in ``dtype``; ``variance`` a float or a map."""
    c = cost.to(dtype).requires_grad_(True)
    is_map = torch.is_tensor(variance)
    v = variance.to(dtype).requires_grad_(True) if is_map else variance
    loss = O.stereo_focal_loss(c, gt.to(dtype), v, FOCAL_D, int(start), 1, fc)
    grads = torch.autograd.grad(loss, (c, v) if is_map else (c,))
    return loss.detach(), grads[0], grads[1] if is_map else None


# (coefficient, variances) of focal_case.  A coefficient of 5 meets variance 0.05 in focal_off_sample_case only: with the target ON a
# sample (gt on a sample or its FP32 neighbour; with start_disp < 0 every masked pixel too, gt * m1 = 0 being a sample) the target
# probability is 1 - 4e-9, which is 1 in FP32, and (1 - P)^-5 is infinite in the reference's own FP32 run: its loss is inf or NaN.
# The kernel's is too (focal_pow: expf(-fc * logf(1 - P)) with P == 1; NaN observed with start_disp = -3 and no valid pixel).
FOCAL_SETTINGS = ((0.0, (0.05, 1.0, 50.0)), (5.0, (1.0, 50.0)))
FOCAL_OFF_SAMPLE = (0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5, 2.25, 4.75, 7.0, 7.5, 8.0, 0.0, -2.0, 11.0)


@functools.lru_cache(maxsize=None)
def focal_off_sample_case():
    """(cost, gt, variance map) for start_disp 0, coefficient 5 and variance 0.05, the steepest regime of the weight
    (1 - P)^-fc: the ground truth takes the values of FOCAL_OFF_SAMPLE only -- halfway between samples (P = 0.5), a quarter off
    (1 - P = 4.5e-5, the weight 5e21), on end_disp and beyond it (m2 = 0), on and outside the bounds (m1 = 0) -- so the target never
    sits on a sample and the reference's FP32 run is finite.  The quarter-off pixels under variance 0.05 are "steep": their gradients
    are 20 orders above the others', and the FP32 reference itself is 2e-3 off there (1 - P carries 2^-24 / 4.5e-5, to the fifth)."""
    gen = torch.Generator().manual_seed(48)
    cost = torch.randn((2, FOCAL_D, 8, 64), generator=gen) * 2
    n = MAP[0] * MAP[2] * MAP[3]
    gi = torch.arange(n) % len(FOCAL_OFF_SAMPLE)
    vi = (torch.arange(n) // len(FOCAL_OFF_SAMPLE)) % 3
    gt = torch.tensor(FOCAL_OFF_SAMPLE, dtype=torch.float32)[gi].view(MAP)
    var = torch.tensor((0.05, 1.0, 50.0), dtype=torch.float32)[vi].view(MAP)
    return cost, gt, var


FOCAL_STEEP = (2.25, 4.75)


# ---------------------------------------------------------------------------------------------- 5. the quantile loss
QUANTILE_BOUNDS = (0.0, 192.0)
THETA = 0.05


@functools.lru_cache(maxsize=None)
def quantile_case():
    """(min, max, gt): gt - min and gt - max exactly 0 and on either FP32 side of it; gt on q_lo and q_hi."""
    gen = torch.Generator().manual_seed(44)
    gt = torch.rand(MAP, generator=gen) * 220 - 10
    mn = gt - 1.0 + torch.randn(MAP, generator=gen) * 2.5
    mx = gt + 1.0 + torch.randn(MAP, generator=gen) * 2.5
    g, lo, hi = gt.view(-1), mn.view(-1), mx.view(-1)
    for k, v in enumerate((3.0, 100.0, 17.25, 191.5)):
        base = 8 * k
        g[base:base + 8] = v
        lo[base:base + 3] = torch.tensor(around(v))
        hi[base + 3:base + 6] = torch.tensor(around(v))
        lo[base + 6], hi[base + 6] = v, v
    for k, v in enumerate((QUANTILE_BOUNDS[0], QUANTILE_BOUNDS[1], 2.0 ** -126, nxt(QUANTILE_BOUNDS[1], False))):
        g[40 + k], lo[40 + k], hi[40 + k] = v, v, v
    return mn, mx, gt


def quantile_reference(mn, mx, gt, dtype):
    """(the two terms, their gradients w.r.t. min and max) of the reference's quantile loss in ``dtype``."""
    a, b = mn.to(dtype).requires_grad_(True), mx.to(dtype).requires_grad_(True)
    t0, t1 = R.quantile_terms(a, b, gt.to(dtype), QUANTILE_BOUNDS[0], QUANTILE_BOUNDS[1], THETA)
    ga, gb = torch.autograd.grad(t0 + t1, (a, b))
    return torch.stack([t0.detach(), t1.detach()]), ga, gb


# ---------------------------------------------------------------------------------------------- 6. ReLU ties of the BN unit
TIE_SHAPES = ((2, 4, 3, 5, 8), (2, 3, 9, 7))


@functools.lru_cache(maxsize=None)
def tie_case(shape, relu):
    """(c, res, dy), small integers: the value the unit's ReLU sees -- c + res after the skip add (relu 1, and relu 0 for symmetry),
    c alone before it (relu 2, every res non-zero) -- is exactly 0 on a third of the elements, positive on a third, negative on the
    rest, in a shuffled order."""
    n = 1
    for d in shape:
        n *= d
    gen = torch.Generator().manual_seed(45 + relu)
    cls = torch.randperm(n, generator=gen) % 3                                   # 0: tie, 1: positive, 2: negative
    mag = torch.randint(1, 4, (n,), generator=gen).float()
    seen = torch.where(cls == 0, torch.zeros(n), torch.where(cls == 1, mag, -mag))
    other = torch.randint(1, 4, (n,), generator=gen).float() * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    if relu == 2:
        c, res = seen, other
    else:
        c, res = other, seen - other
    dy = torch.randint(1, 8, (n,), generator=gen).float() * 0.25 * (torch.randint(0, 2, (n,), generator=gen).float() * 2 - 1)
    return c.view(shape), res.view(shape), dy.view(shape)


def tie_reference(c, res, dy, relu, dtype=torch.float32):
    """O.bn_act_train in eval mode with scale 1, shift 0, mean 0, invstd 1 (eps = 1e-30: 1 + eps is 1 in FP32 and FP64, invstd exactly 1)."""
    C = c.shape[1]
    return O.bn_act_train(c, torch.ones(C), torch.zeros(C), res, relu, eps=1e-30, dy=dy, dtype=dtype, training=False,
                          running_mean=torch.zeros(C), running_var=torch.ones(C))


# ---------------------------------------------------------------------------------------------- 7. the soft-argmin family
GAINS = (1e2, 1e3, 1e4)
SOFT_SHAPE = (2, 3, 8)       # B, H, W


@functools.lru_cache(maxsize=None)
def soft_argmin_case(D):
    """(logits [2, D, 3, 8], kinds [2, 3, 8]): per pixel a column of O(1) logits in which one entry exceeds the rest by 1e2, 1e3 or
    1e4 (kinds 0 - 2: one-hot), two entries equal 1e4 (kind 3), or every entry equals 1e4 or -1e4 (kinds 4, 5).  The peak's plane
    moves with the pixel and reaches the first and the last plane."""
    B, H, W = SOFT_SHAPE
    gen = torch.Generator().manual_seed(46 + D)
    x = torch.rand((B, D, H, W), generator=gen) * 2 - 1
    kinds = (torch.arange(B * H * W) % 6).view(B, H, W)
    peaks = torch.zeros((B, H, W, 2), dtype=torch.long)
    for i in range(B * H * W):
        b, h, w = i // (H * W), (i // W) % H, i % W
        kind = int(kinds[b, h, w])
        p = (0, D - 1, (i * 5) % D, (i * 3 + 1) % D)[(i // 6) % 4]
        q = (p + 1 + i % max(D - 1, 1)) % D if D > 1 else p
        peaks[b, h, w] = torch.tensor([p, q])
        if kind < 3:
            x[b, p, h, w] = 1.0 + GAINS[kind]
        elif kind == 3:
            x[b, p, h, w] = 1e4
            x[b, q, h, w] = 1e4
        else:
            x[b, :, h, w] = 1e4 if kind == 4 else -1e4
    return x, kinds, peaks
