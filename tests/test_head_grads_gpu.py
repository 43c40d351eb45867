"""Randomised forward AND backward sweep of the training path's heads, volume ends and losses against torch on the CPU in FP64.

tests/test_unit_grads_gpu.py sweeps the convolution units.  Everything on either side of them -- the cost-volume builders, the
volume-free first unit, the up-sampling and regression ends, AcfNet's learned up-sampling and confidence head, the 2-D resamplers
and the three losses -- had its backward kernels checked at a few fixed shapes with default settings.  This module draws ~250
seeded cases over them, each through the PUBLIC modules or the layers/train_fn.py Functions (never the raw ops wrappers):

  focal loss (levels, truncating level widths, start_disp, dilation, focal coefficient, every variance form, sparse pooling,
  > 65 536 pixels), NLL / smooth-L1 (logits to +-40, |est - gt| at and around 1), SoftArgmin / FasterSoftArgmin (D 1 .. 256,
  alpha), UpsampleRegressFn (extents of 1, non-integer ratios, both forms of the (y, x) contraction, gradient on either output or
  both), DeconvK8S4Fn (dx only, dw only, both), the CMN confidence head with every BatchNorm option, cat_fms / dif_fms,
  FastFmsFn (per-pixel samples with a gradient, normalize p 1 / 2, W to 1024), CatConvUnitFn, the three 2-D resamplers;
  and the CHAINS PSMNet head (the RegressionHint accepted or rejected), AcfNet adaptive and AcfNet uniform.

The reference is torch on the CPU, run in FP64 and again in FP32; the losses use tests/_head_ref.py, whose masks, pooled ground
truth and sample values are computed once in FP32 as the reference computes them and shared by both evaluations (CPU-pinned
against the real reference by tests/test_oracle_golden.py).  One seeded upstream gradient per output.  Every output and gradient:
|hip - fp64| <= 4 |fp32 - fp64| + 2e-6 range (test_backward_gpu.py's rule; a scalar loss: range = |loss_64|).  Also per case: the
intended train_fn Function / _FocalLevel / MapLoss is in the output's graph (no silent fall-back), and a second identical pass is
bit-identical -- except FastFmsFn's target-feature gradient, which is scattered with LDS atomics in the hardware's order (held to
the tolerance only).  Shapes the library documents as unsupported are drawn on purpose and must raise DmbLibraryError /
NotImplementedError in the forward pass; any other refusal is a failure.  ``DMB_HEAD_GRADS_SEED_BASE`` moves the seeds."""
import copy
import os
import random
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import dmb_oracle as O
from tests import _head_ref as HR
from tests.test_unit_grads_gpu import _compare, _init

pytestmark = pytest.mark.gpu

CASES_PER_CHUNK = 21
CHUNKS = 12
ELEM_BUDGET = 1.5e6    # elements of the largest tensor of a case (the CPU reference runs it forward + backward twice)
FLOP_BUDGET = 3e8      # multiply-adds x 2 of a case's convolutions
SEED_BASE = int(os.environ.get("DMB_HEAD_GRADS_SEED_BASE", "90000"))
MAX_DISPS = [2, 5, 12, 48, 64, 65, 128, 192, 256]
STARTS = [0, -4, 3]
BN_OPTS = ["none", "train", "eval", "momentum_none", "affine_false", "no_track"]


def _lib_errors():
    from densematchingbenchmark_amd._lib import DmbLibraryError
    return (DmbLibraryError, NotImplementedError)


# ------------------------------------------------------------------------------------------------------------- references
def _trilinear(x, size):
    return F.interpolate(x.unsqueeze(1), size=tuple(size), mode="trilinear", align_corners=True).squeeze(1)


def _soft_argmin(cost, values, alpha):
    v = torch.tensor(values, dtype=torch.float32).to(cost.dtype).view(1, -1, 1, 1)
    return (F.softmax(cost * alpha, dim=1) * v).sum(1, keepdim=True)


def _deconv8(x, w):
    return F.conv_transpose3d(x.unsqueeze(1), w, None, stride=4, padding=2).squeeze(1)


def _volume(L, R, idx, kind):
    """cat_fms.py:7-48 / dif_fms.py:7-46 with the integer disparities ``idx`` (differentiable slices)."""
    B, C, H, W = L.shape
    vol = L.new_zeros((B, 2 * C if kind == "cat" else C, len(idx), H, W)) + 0.0 * (L.sum() + R.sum())   # (a graph when all is zero)
    for k, d in enumerate(idx):
        lo, hi = max(d, 0), min(W, W + d)
        if lo >= hi:
            continue
        if kind == "cat":
            vol[:, :C, k, :, lo:hi] = L[:, :, :, lo:hi]
            vol[:, C:, k, :, lo:hi] = R[:, :, :, lo - d:hi - d]
        else:
            vol[:, :, k, :, lo:hi] = L[:, :, :, lo:hi] - R[:, :, :, lo - d:hi - d]
    return vol


def _fast_volume(L, R, ds, kind, normalize=False, p=1.0):
    """cat_fms.py:51-82 / dif_fms.py:49-86 through the sampler of inverse_warp_3d.py (grid_sample, align_corners=False on a
    (size - 1)-normalised grid), as oracle.fast_volume_grads runs it; ``ds`` [B, D, H, W]."""
    dt = L.dtype
    B, D, H, W = ds.shape
    C = R.shape[1]
    img = R.unsqueeze(2).expand(B, C, D, H, W)
    gd = torch.linspace(0, D - 1, D, dtype=dt).view(1, D, 1, 1).expand(B, D, H, W)
    gh = torch.linspace(0, H - 1, H, dtype=dt).view(1, 1, H, 1).expand(B, D, H, W)
    gw = torch.linspace(0, W - 1, W, dtype=dt).view(1, 1, 1, W).expand(B, D, H, W) + (-ds)
    grid = torch.stack(((gw / (W - 1) * 2) - 1, (gh / (H - 1) * 2) - 1, (gd / (D - 1) * 2) - 1), dim=4)
    tgt = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    ref = L.unsqueeze(2) * (tgt > 0).to(dt).detach()
    vol = torch.cat((ref, tgt), dim=1) if kind == "cat" else ref - tgt
    return torch.norm(vol, p=p, dim=1, keepdim=False) if normalize else vol


# ------------------------------------------------------------------------------------------------------------- ground truth
def _gt(rng, g, B, H, W, lo, hi, specials):
    """Ground truth [B, 1, H, W] from a mixture: uniform past both bounds, exact bound / sample values, KITTI-like sparse maps,
    batch items without a valid pixel."""
    form = rng.choice(["uniform", "uniform", "special", "sparse", "empty_item"])
    span = hi - lo
    gt = lo - 0.1 * span - 2 + (1.2 * span + 4) * torch.rand((B, 1, H, W), generator=g)
    if form == "special" and specials:
        pick = torch.rand((B, 1, H, W), generator=g) < 0.4
        vals = torch.tensor(specials, dtype=torch.float32)[torch.randint(0, len(specials), (B, 1, H, W), generator=g)]
        gt = torch.where(pick, vals, gt)
    elif form == "sparse":
        gt = torch.where(torch.rand((B, 1, H, W), generator=g) < 0.8, torch.zeros_like(gt), gt.abs())
    elif form == "empty_item":
        gt[rng.randrange(B)] = float(lo) - 1.0 if rng.random() < 0.5 else 0.0
        if rng.random() < 0.2:
            gt.fill_(float(min(lo, 0)) - 1.0)                       # no valid pixel anywhere
    return gt.float(), form


def _shrink(dims, cost, budget):
    """Halve the largest of ``dims`` (a dict name -> extent, in preference order) until cost(dims) <= budget."""
    while cost(dims) > budget:
        k = max(dims, key=lambda n: dims[n])
        if dims[k] <= 1:
            break
        dims[k] = max(1, dims[k] // 2)
    return dims


# ------------------------------------------------------------------------------------------------------------- the draws
def _case(desc, leaves, dev, ref, fns, consts=None, mods=None, nograd=(), ograd=None, refuse=False, nondet=(), pool=None):
    return dict(desc=desc, leaves=leaves, consts=consts or {}, dev=dev, ref=ref, fns=fns, mods=mods, nograd=set(nograd),
                ograd=ograd, refuse=refuse, nondet=set(nondet), pool=pool)


def _pooled(c, hw):
    return c.get("pooled", {}).get(tuple(hw))


def _draw(seed):
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    kind = rng.choice(["focal"] * 5 + ["map"] * 3 + ["regress"] * 3 + ["upreg"] * 3 + ["deconv"] * 2 + ["confhead"] * 2
                      + ["catdif"] * 2 + ["fastfms"] * 3 + ["firstunit"] * 2 + ["pool", "bilac", "bilac", "bilscale"]
                      + ["chain_psm"] * 2 + ["chain_acf"] * 2 + ["chain_uni", "refuse"])
    return globals()["_draw_" + kind](rng, g)


def _levels(rng, Wg, Hg, n):
    """Level sizes for gt [Hg, Wg]: 1x .. 4x the level width, some non-integer ratios (int(max_disp / scale) truncates)."""
    out = []
    for _ in range(n):
        f = rng.choice([1, 1, 2, 3, 4, 1.5, 2.5, 3.3])
        out.append((max(1, int(round(Hg / f))), max(1, int(round(Wg / f)))))
    return out


def _draw_focal(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.losses import StereoFocalLoss
    B = rng.randint(1, 4)
    md, sd, dil = rng.choice(MAX_DISPS), rng.choice(STARTS), rng.randint(1, 3)
    fc = rng.choice([0.0, 2.0, 5.0]) if (md + dil - 1) // dil > 1 else 0.0    # (one sample: P = 1, (1 - P)^-fc is not finite)
    sparse = rng.random() < 0.3
    nlev = rng.choice([1, 1, 2, 3])
    big = rng.random() < 0.12
    Hg, Wg = (rng.randint(150, 260), rng.randint(300, 420)) if big else (rng.randint(2, 40), rng.randint(2, 80))
    levels = _levels(rng, Wg, Hg, nlev)
    if big:
        md, dil, levels = rng.choice([2, 5, 12]), 1, [(Hg, Wg)] + levels[1:]
    nsamp = lambda hw: (int(md / (Wg / hw[1])) + dil - 1) // dil    # noqa: E731
    levels = [hw for hw in levels if nsamp(hw) >= 1] or [(Hg, Wg)]
    while sum(B * nsamp(hw) * hw[0] * hw[1] for hw in levels) > (4 * ELEM_BUDGET if big else ELEM_BUDGET) and B > 1:
        B -= 1
    while sum(B * nsamp(hw) * hw[0] * hw[1] for hw in levels) > (4 * ELEM_BUDGET if big else ELEM_BUDGET) and len(levels) > 1:
        levels.pop()
    cscale = rng.choice([1.0, 3.0, 30.0])
    vform = rng.choice(["float", "map", "map1", "detached"])
    gt, gform = _gt(rng, g, B, Hg, Wg, sd, sd + md, [sd, sd + md, sd + md - 1, sd + 1.0, sd + 2.5, float(sd + md // 2)])
    leaves, consts = {}, {"gt": gt}
    for i, (h, w) in enumerate(levels):
        leaves["cost%d" % i] = torch.randn((B, nsamp((h, w)), h, w), generator=g, dtype=torch.float64) * cscale
        if vform in ("map", "map1", "detached"):
            v = 0.3 + 3.7 * torch.rand((B if vform != "map1" else 1, 1, h, w), generator=g, dtype=torch.float64)
            (consts if vform == "detached" else leaves)["var%d" % i] = v.float() if vform == "detached" else v
    vfloat = rng.uniform(0.3, 4.0)
    weights = tuple(round(rng.uniform(0.3, 1.5), 3) for _ in levels)
    n = len(levels)

    def variance(t, c):
        if vform == "float":
            return vfloat
        src = c if vform == "detached" else t
        return [src["var%d" % i] for i in range(n)]

    def dev(m, t, c):
        out = StereoFocalLoss(md, sd, dil, weights, fc, sparse)([t["cost%d" % i] for i in range(n)], c["gt"], variance(t, c))
        return [out["stereo_focal_loss_lvl%d" % i] for i in range(n)]

    def ref(m, t, c):
        var = variance(t, c)
        outs = []
        for i in range(n):
            cost = t["cost%d" % i]
            v = var if vform == "float" else var[i].to(cost.dtype)
            prep = HR.focal_prep(c["gt"], cost.shape, md, sd, dil, sparse, _pooled(c, cost.shape[-2:]))
            outs.append(weights[i] * HR.focal_level(cost, v, prep, fc))
        return outs
    return _case(("focal", B, md, sd, dil, fc, sparse, levels, (Hg, Wg), cscale, vform, gform, weights), leaves, dev, ref,
                 [["_FocalLevel"]] * n, consts=consts, pool=(levels, sparse))


def _draw_map(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.losses import ConfidenceNllLoss, DispSmoothL1Loss
    which = rng.choice(["nll", "l1"])
    B = rng.randint(1, 4)
    md, sd = rng.choice(MAX_DISPS), rng.choice(STARTS)
    sparse = rng.random() < 0.3
    big = rng.random() < 0.1
    Hg, Wg = (rng.randint(200, 300), rng.randint(300, 500)) if big else (rng.randint(1, 48), rng.randint(1, 96))
    levels = _levels(rng, Wg, Hg, rng.choice([1, 1, 2, 3]))
    gt, gform = _gt(rng, g, B, Hg, Wg, sd, sd + md, [sd, sd + md, sd + 0.5, float(sd + md) - 0.5])
    leaves = {}
    for i, (h, w) in enumerate(levels):
        if which == "nll":
            x = torch.randn((B, 1, h, w), generator=g, dtype=torch.float64) * rng.choice([1.0, 5.0, 15.0])
            x = x.clamp(-40, 40)
            x.view(-1)[torch.randint(0, x.numel(), (max(1, x.numel() // 10),), generator=g)] = rng.choice([40.0, -40.0])
        else:
            sg = HR.level_gt(gt, (h, w), sparse)[0].double()
            delta = torch.randn(sg.shape, generator=g, dtype=torch.float64) * 2.0
            form = torch.randint(0, 4, sg.shape, generator=g)
            sign = torch.where(torch.rand(sg.shape, generator=g) < 0.5, -1.0, 1.0).double()
            delta = torch.where(form == 1, sign, torch.where(form == 2, sign * (1.0 + 1e-3 * torch.randn(sg.shape, generator=g,
                                                                                                         dtype=torch.float64)), delta))
            x = sg + delta
        leaves["x%d" % i] = x
    weights = tuple(round(rng.uniform(0.3, 1.5), 3) for _ in levels)
    n = len(levels)
    cls = ConfidenceNllLoss if which == "nll" else DispSmoothL1Loss
    key = "conf_loss_lvl%d" if which == "nll" else "l1_loss_lvl%d"
    lvl = HR.nll_level if which == "nll" else HR.smooth_l1_level

    def dev(m, t, c):
        out = cls(md, sd, weights, sparse)([t["x%d" % i] for i in range(n)], c["gt"])
        return [out[key % i] for i in range(n)]

    def ref(m, t, c):
        return [weights[i] * lvl(t["x%d" % i], *HR.map_prep(c["gt"], t["x%d" % i].shape[-2:], md, sd, sparse,
                                                             _pooled(c, t["x%d" % i].shape[-2:]))) for i in range(n)]
    return _case((which, B, md, sd, sparse, levels, (Hg, Wg), gform, weights), leaves, dev, ref, [["MapLoss"]] * n,
                 consts={"gt": gt}, pool=(levels, sparse))


def _draw_regress(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import FasterSoftArgmin, SoftArgmin
    cls = rng.choice([SoftArgmin, FasterSoftArgmin])
    md = rng.choice([1, 2, 3, 5, 12, 47, 48, 64, 65, 128, 192, 255, 256])
    sd, dil = rng.choice(STARTS), rng.choice([1, 1, 2, 3])
    D = (md + dil - 1) // dil
    alpha = rng.choice([1.0, 0.5, -1.0, 4.0])
    dims = _shrink({"H": rng.randint(1, 40), "W": rng.randint(1, 130), "B": rng.randint(1, 4)},
                   lambda d: d["B"] * D * d["H"] * d["W"], ELEM_BUDGET)
    B, H, W = dims["B"], dims["H"], dims["W"]
    values = torch.linspace(sd, sd + md - 1, D).tolist()
    leaves = {"cost": torch.randn((B, D, H, W), generator=g, dtype=torch.float64) * rng.choice([1.0, 3.0, 10.0])}
    return _case(("regress", cls.__name__, B, md, sd, dil, D, H, W, alpha), leaves,
                 lambda m, t, c: [cls(md, sd, dil, alpha)(t["cost"])],
                 lambda m, t, c: [_soft_argmin(t["cost"], values, alpha)], [["SoftArgminFn"]])


def _upreg_shape(rng):
    form = rng.choice(["psm", "psm", "odd", "ones", "wide"])
    if form == "psm":            # 48 -> 192 and (Hi, Wi) -> (4 Hi, 4 Wi), scaled down
        Di = rng.choice([1, 3, 6, 12])
        Hi, Wi = rng.randint(1, 10), rng.randint(1, 40)
        return (Di, Hi, Wi), (4 * Di, 4 * Hi, 4 * Wi), form
    if form == "odd":            # non-integer ratios
        Di, Hi, Wi = rng.randint(1, 13), rng.randint(1, 12), rng.randint(1, 60)
        return (Di, Hi, Wi), (rng.randint(Di, 4 * Di + 3), rng.randint(Hi, 4 * Hi + 3), rng.randint(Wi, 4 * Wi + 3)), form
    if form == "ones":           # extents of 1 in the input and / or the output
        ex = [rng.choice([1, 1, rng.randint(2, 9)]) for _ in range(3)]
        return tuple(ex), tuple(rng.choice([1, e, 4 * e, 4 * e + 1]) if e > 1 else rng.choice([1, 4, 7]) for e in ex), form
    Wi = rng.randint(300, 410)   # past the 64 KB LDS of the row-group form at ratio 4: one thread per voxel
    return (rng.randint(1, 3), rng.randint(1, 3), Wi), None, form


def _draw_upreg(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    (Di, Hi, Wi), out, form = _upreg_shape(rng)
    if out is None:
        out = (4 * Di, 4 * Hi, 4 * Wi)
    Do, Ho, Wo = out
    B = rng.randint(1, 3)
    while B * Do * Ho * Wo > ELEM_BUDGET and B > 1:
        B -= 1
    if B * Do * Ho * Wo > ELEM_BUDGET:
        Do = max(1, int(ELEM_BUDGET // (Ho * Wo)))
    sd = rng.choice(STARTS)
    values = torch.linspace(sd, sd + Do - 1, Do).tolist()
    alpha = rng.choice([1.0, 0.5, -1.0, 4.0])
    want = rng.choice(["disp", "vol", "both"])
    ograd = {"disp": [False, True], "vol": [True, False], "both": [True, True]}[want]
    leaves = {"x": torch.randn((B, Di, Hi, Wi), generator=g, dtype=torch.float64) * rng.choice([1.0, 4.0])}

    def ref(m, t, c):
        up = _trilinear(t["x"], (Do, Ho, Wo))
        return [up, _soft_argmin(up, values, alpha)]
    return _case(("upreg", form, B, (Di, Hi, Wi), (Do, Ho, Wo), sd, alpha, want), leaves,
                 lambda m, t, c: list(train_fn.UpsampleRegressFn.apply(t["x"], (Do, Ho, Wo), tuple(values), alpha)), ref,
                 [["UpsampleRegressFn"]] * 2, ograd=ograd)


def _draw_deconv(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    dims = _shrink({"W": rng.choice([1, 2, 3, 5, 7, 9, 16, 33, 65, rng.randint(1, 80)]), "H": rng.choice([1, 2, 3, 5, 9, 13]),
                    "D": rng.choice([1, 2, 3, 5, 12]), "B": rng.randint(1, 3)},
                   lambda d: 64 * d["B"] * d["D"] * d["H"] * d["W"], ELEM_BUDGET)
    B, D, H, W = dims["B"], dims["D"], dims["H"], dims["W"]
    want = rng.choice(["dx", "dw", "both"])
    leaves = {"x": torch.randn((B, D, H, W), generator=g, dtype=torch.float64),
              "w": torch.randn((1, 1, 8, 8, 8), generator=g, dtype=torch.float64) / 8.0}
    nograd = {"dx": ["w"], "dw": ["x"], "both": []}[want]
    return _case(("deconv", B, D, H, W, want), leaves, lambda m, t, c: [train_fn.DeconvK8S4Fn.apply(t["x"], t["w"])],
                 lambda m, t, c: [_deconv8(t["x"], t["w"])], [["DeconvK8S4Fn"]], nograd=nograd)


def _conf_head(rng, D, opt, mode):
    from densematchingbenchmark_amd.modeling.stereo.cmn.cmn import ConfHead
    h = ConfHead(D, batch_norm=opt != "none")
    if opt != "none":
        bn_cls, Cm = type(h.conf_net[0][1]), h.sec_in_planes
        if opt == "affine_false":
            h.conf_net[0][1] = bn_cls(Cm, affine=False)
        elif opt == "no_track":
            h.conf_net[0][1] = bn_cls(Cm, track_running_stats=False)
        elif opt == "momentum_none":
            h.conf_net[0][1].momentum = None
        h.conf_net[0][1].train(opt in ("train", "momentum_none", "affine_false") or (opt == "no_track" and rng.random() < 0.5))
    h.train(mode == "train")
    return h


def _draw_confhead(rng, g):
    D = rng.choice([4, 12, 48, 96, 192])
    opt, mode = rng.choice(BN_OPTS), rng.choice(["train", "eval"])
    Cm = max(1, D // 3)
    dims = _shrink({"W": rng.randint(1, 70), "H": rng.randint(1, 30), "B": rng.randint(1, 3)},
                   lambda d: d["B"] * d["H"] * d["W"] * D * Cm * 18, FLOP_BUDGET)
    B, H, W = dims["B"], dims["H"], dims["W"]
    if opt != "none" and B * H * W < 8:
        H, W = max(H, 3), max(W, 3)
    leaves = {"cost": torch.randn((B, D, H, W), generator=g, dtype=torch.float64) * 2.0}
    return _case(("confhead", B, D, H, W, opt, mode), leaves, lambda m, t, c: [m[0].logits(t["cost"])],
                 lambda m, t, c: [m[0].conf_net(t["cost"])], [["ConfHeadFn"]], mods=lambda: [_conf_head(rng, D, opt, mode)])


def _draw_catdif(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import cat_fms
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.dif_fms import dif_fms
    kind = rng.choice(["cat", "dif"])
    W = rng.randint(1, 90)
    md = rng.choice([1, 3, 12, 48, W + rng.randint(1, 20)])
    sd, dil = rng.choice([0, 0, -4, 3, -W - 2]), rng.randint(1, 3)
    idx = O.disp_index_list(md, sd, dil)
    C = rng.choice([1, 3, 8, 16, 32])
    dims = _shrink({"H": rng.randint(1, 20), "B": rng.randint(1, 3)},
                   lambda d: d["B"] * 2 * C * len(idx) * d["H"] * W, ELEM_BUDGET)
    B, H = dims["B"], dims["H"]
    leaves = {"L": torch.randn((B, C, H, W), generator=g, dtype=torch.float64),
              "R": torch.randn((B, C, H, W), generator=g, dtype=torch.float64)}
    fn = cat_fms if kind == "cat" else dif_fms
    return _case((kind, B, C, H, W, md, sd, dil), leaves, lambda m, t, c: [fn(t["L"], t["R"], md, sd, dil)],
                 lambda m, t, c: [_volume(t["L"], t["R"], idx, kind)], [["CatFmsFn" if kind == "cat" else "DifFmsFn"]])


def _draw_fastfms(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import fast_cat_fms
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.dif_fms import fast_dif_fms
    kind = rng.choice(["cat", "dif", "dif"])
    normalize = kind == "dif" and rng.random() < 0.5
    p = rng.choice([1.0, 2.0])
    W = rng.choice([2, 3, 17, 64, 100, rng.randint(2, 200), rng.randint(900, 1024), 1024])
    C = rng.choice([1, 3, 8, 9, 13, 16, 20])
    md, sd, dil = rng.choice([2, 5, 12, 24]), rng.choice([0, -4, 3]), rng.randint(1, 2)
    D = (md + dil - 1) // dil
    if D < 2:
        md, D = 2 * dil, 2
    samples = rng.choice(["builder", "pixel_grad", "pixel_grad", "pixel"])
    dims = _shrink({"H": rng.randint(2, 16), "B": rng.randint(1, 3)},
                   lambda d: d["B"] * 2 * C * D * d["H"] * W, ELEM_BUDGET / 2)
    B, H = dims["B"], max(2, dims["H"])
    leaves = {"L": torch.randn((B, C, H, W), generator=g, dtype=torch.float64),
              "R": torch.randn((B, C, H, W), generator=g, dtype=torch.float64)}
    consts = {}
    if samples == "builder":
        consts["ds"] = O.fast_disp_samples(md, sd, dil).view(1, -1, 1, 1).expand(B, D, H, W).contiguous()
    else:       # fractional, some outside [0, W)
        s = sd + (md + 4) * torch.rand((B, D, H, W), generator=g, dtype=torch.float64) - 2
        s.view(-1)[torch.randint(0, s.numel(), (max(1, s.numel() // 20),), generator=g)] = float(W) + 1.5
        if samples == "pixel_grad":
            leaves["ds"] = s
        else:
            consts["ds"] = s.float()

    def dev(m, t, c):
        ds = None if samples == "builder" else (t["ds"] if samples == "pixel_grad" else c["ds"])
        if kind == "cat":
            return [fast_cat_fms(t["L"], t["R"], md, sd, dil, ds)]
        return [fast_dif_fms(t["L"], t["R"], md, sd, dil, ds, normalize, p)]

    def ref(m, t, c):
        ds = t["ds"] if samples == "pixel_grad" else c["ds"].to(t["L"].dtype)
        return [_fast_volume(t["L"], t["R"], ds, kind, normalize, p)]
    return _case(("fast", kind, normalize, p, B, C, D, H, W, md, sd, dil, samples), leaves, dev, ref, [["FastFmsFn"]],
                 consts=consts, nondet=[("in", "R")])


def _draw_firstunit(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import LazyCatVolume
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d
    kind = rng.choice(["cat", "dif"])
    C, Co = rng.choice([1, 3, 8, 16, 32]), rng.choice([1, 4, 8, 16, 32])
    D = rng.choice([4, 8, 12, 16, 24])
    W = 4 * rng.randint((D + 8 + 3) // 4, 30)
    opt, mode, bias = rng.choice(BN_OPTS), rng.choice(["train", "train", "eval"]), rng.random() < 0.5
    Ci = 2 * C if kind == "cat" else C
    dims = _shrink({"H": rng.randint(1, 12), "B": rng.randint(1, 3)},
                   lambda d: d["B"] * D * d["H"] * W * Ci * Co * 54, FLOP_BUDGET)
    B, H = dims["B"], dims["H"]
    leaves = {"L": torch.randn((B, C, H, W), generator=g, dtype=torch.float64),
              "R": torch.randn((B, C, H, W), generator=g, dtype=torch.float64)}

    def make():
        u = FusedConv3d(opt != "none", Ci, Co, 3, 1, 1, 1, bias)
        u.train(mode == "train")
        if opt != "none":
            bn_cls = type(u[1])
            if opt == "affine_false":
                u[1] = bn_cls(Co, affine=False)
            elif opt == "no_track":
                u[1] = bn_cls(Co, track_running_stats=False)
            elif opt == "momentum_none":
                u[1].momentum = None
            u[1].train(opt in ("train", "momentum_none", "affine_false") or (opt == "no_track" and rng.random() < 0.5))
        return [u]

    def dev(m, t, c):
        lazy = LazyCatVolume(t["L"], t["R"], max_disp=D, kind=kind, differentiable=True)
        return [train_fn.cat_conv_unit(m[0], lazy)]

    def ref(m, t, c):
        body = nn.Sequential(*list(m[0].children())[:2 if m[0].has_bn else 1])
        return [body(_volume(t["L"], t["R"], list(range(D)), kind))]
    return _case(("firstunit", kind, B, C, Co, D, H, W, opt, mode, bias), leaves, dev, ref, [["CatConvUnitFn"]], mods=make)


def _draw_pool(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    k = rng.choice([8, 16, 32, 64])
    H, W = k * rng.randint(1, 4) + rng.randint(0, k - 1), k * rng.randint(1, 6) + rng.randint(0, k - 1)
    B, C = rng.randint(1, 2), rng.choice([1, 3, 8, 32])
    leaves = {"x": torch.randn((B, C, H, W), generator=g, dtype=torch.float64)}
    return _case(("avgpool", B, C, H, W, k), leaves, lambda m, t, c: [train_fn.AvgPool2dFn.apply(t["x"], k)],
                 lambda m, t, c: [F.avg_pool2d(t["x"], k)], [["AvgPool2dFn"]])


def _draw_bilac(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    if rng.random() < 0.5:        # footprints of >= 64 output pixels: the one-wave-per-input-element form
        Hi, Wi = rng.randint(1, 6), rng.randint(1, 8)
        Ho, Wo = rng.randint(8 * Hi, 16 * Hi + 5), rng.randint(8 * Wi, 16 * Wi + 5)
    else:
        Hi, Wi = rng.randint(1, 20), rng.choice([rng.randint(1, 60), rng.randint(300, 420)])
        Ho, Wo = rng.choice([Hi, 2 * Hi, 4 * Hi, rng.randint(1, 4 * Hi + 3)]), rng.choice([Wi, 2 * Wi, 4 * Wi, rng.randint(1, 4 * Wi + 3)])
    B, C = rng.randint(1, 2), rng.choice([1, 2, 8, 32])
    while B * C * Ho * Wo > ELEM_BUDGET and C > 1:
        C //= 2
    leaves = {"x": torch.randn((B, C, Hi, Wi), generator=g, dtype=torch.float64)}
    return _case(("bilinear_ac", B, C, Hi, Wi, Ho, Wo), leaves, lambda m, t, c: [train_fn.BilinearAcFn.apply(t["x"], (Ho, Wo))],
                 lambda m, t, c: [F.interpolate(t["x"], (Ho, Wo), mode="bilinear", align_corners=True)], [["BilinearAcFn"]])


def _draw_bilscale(rng, g):
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    Hi, Wi = rng.randint(1, 24), rng.randint(1, 80)
    Ho, Wo = rng.randint(1, 3 * Hi + 5), rng.randint(1, 3 * Wi + 5)
    mult = rng.choice([1.0, 0.5, 2.0, 3.7, -1.25])
    B, C = rng.randint(1, 2), rng.choice([1, 3, 8, 32])
    leaves = {"x": torch.randn((B, C, Hi, Wi), generator=g, dtype=torch.float64)}
    return _case(("bilinear_scale", B, C, Hi, Wi, Ho, Wo, mult), leaves,
                 lambda m, t, c: [train_fn.BilinearScaleFn.apply(t["x"], (Ho, Wo), mult)],
                 lambda m, t, c: [F.interpolate(t["x"], (Ho, Wo), mode="bilinear", align_corners=False) * mult], [["BilinearScaleFn"]])


def _draw_chain_psm(rng, g):
    """Low-resolution cost -> UpsampleRegressFn -> FasterSoftArgmin -> DispSmoothL1Loss on two 'levels': the predictor's disparity
    and the up-sampling's own.  alpha != 1 rejects the RegressionHint: SoftArgminFn runs on the volume and the gradient reaches
    UpsampleRegressFn through both outputs."""
    from densematchingbenchmark_amd import ops
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import FasterSoftArgmin
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from densematchingbenchmark_amd.modeling.stereo.losses import DispSmoothL1Loss
    Di = rng.choice([1, 2, 3, 6, 12])
    Hi, Wi, B = rng.randint(1, 8), rng.randint(1, 30), rng.randint(1, 2)
    Do, Ho, Wo = 4 * Di, 4 * Hi, 4 * Wi
    alpha = rng.choice([1.0, 1.0, 0.5, 2.0])
    vals = ops.disp_sample_values(Do, 0, 1)
    gt, gform = _gt(rng, g, B, Ho, Wo, 0, Do, [0.0, float(Do), 1.0, float(Do) - 0.5])
    leaves = {"x": torch.randn((B, Di, Hi, Wi), generator=g, dtype=torch.float64) * 3.0}

    def dev(m, t, c):
        cost, disp = train_fn.UpsampleRegressFn.apply(t["x"], (Do, Ho, Wo), tuple(vals), 1.0)
        ops.RegressionHint.attach(cost, vals, 1.0, disp)
        pred = FasterSoftArgmin(Do, alpha=alpha)(cost)
        out = DispSmoothL1Loss(Do, weights=(1.0, 0.7))([pred, disp], c["gt"])
        return [out["l1_loss_lvl0"], out["l1_loss_lvl1"]]

    def ref(m, t, c):
        up = _trilinear(t["x"], (Do, Ho, Wo))
        sg, mask = HR.map_prep(c["gt"], (Ho, Wo), Do)
        return [HR.smooth_l1_level(_soft_argmin(up, vals, alpha), sg, mask),
                0.7 * HR.smooth_l1_level(_soft_argmin(up, vals, 1.0), sg, mask)]
    fns = [["MapLoss", "UpsampleRegressFn"] + (["SoftArgminFn"] if alpha != 1.0 else []), ["MapLoss", "UpsampleRegressFn"]]
    return _case(("chain_psm", B, Di, Hi, Wi, alpha, gform), leaves, dev, ref, fns, consts={"gt": gt})


def _draw_chain_acf(rng, g):
    """AcfNet adaptive: DeconvK8S4Fn -> confidence head -> sigmoid -> alpha (1 - conf) + beta -> focal loss (variance gradient),
    NLL on the logits."""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from densematchingbenchmark_amd.modeling.stereo.losses import ConfidenceNllLoss, StereoFocalLoss
    Dq = rng.choice([1, 3, 12])
    D = 4 * Dq
    Hq, Wq, B = rng.randint(1, 5), rng.randint(1, 12), rng.randint(1, 2)
    opt, mode = rng.choice(BN_OPTS), rng.choice(["train", "eval"])
    if opt != "none" and B * Hq * Wq * 16 < 8:
        Hq = 2
    a, b, fc = rng.choice([1.0, 0.5]), rng.choice([1.0, 0.3]), rng.choice([0.0, 5.0])
    gt, gform = _gt(rng, g, B, 4 * Hq, 4 * Wq, 0, D, [0.0, float(D), float(D - 1), 1.0])
    leaves = {"x": torch.randn((B, Dq, Hq, Wq), generator=g, dtype=torch.float64),
              "w": torch.randn((1, 1, 8, 8, 8), generator=g, dtype=torch.float64) / 4.0}

    def dev(m, t, c):
        cost = train_fn.DeconvK8S4Fn.apply(t["x"], t["w"])
        logit = m[0].logits(cost)
        var = a * (1 - torch.sigmoid(logit)) + b
        return [StereoFocalLoss(D, focal_coefficient=fc)(cost, c["gt"], var)["stereo_focal_loss_lvl0"],
                ConfidenceNllLoss(D)(logit, c["gt"])["conf_loss_lvl0"]]

    def ref(m, t, c):
        cost = _deconv8(t["x"], t["w"])
        logit = m[0].conf_net(cost)
        var = a * (1 - torch.sigmoid(logit)) + b
        return [HR.focal_level(cost, var, HR.focal_prep(c["gt"], cost.shape, D), fc),
                HR.nll_level(logit, *HR.map_prep(c["gt"], logit.shape[-2:], D))]
    return _case(("chain_acf", B, Dq, Hq, Wq, opt, mode, a, b, fc, gform), leaves, dev, ref,
                 [["_FocalLevel", "DeconvK8S4Fn", "ConfHeadFn"], ["MapLoss", "ConfHeadFn", "DeconvK8S4Fn"]], consts={"gt": gt},
                 mods=lambda: [_conf_head(rng, D, opt, mode)])


def _draw_chain_uni(rng, g):
    """AcfNet uniform: DeconvK8S4Fn -> focal loss (float variance) + SoftArgmin -> smooth-L1."""
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import SoftArgmin
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    from densematchingbenchmark_amd.modeling.stereo.losses import DispSmoothL1Loss, StereoFocalLoss
    Dq = rng.choice([1, 3, 12])
    D = 4 * Dq
    Hq, Wq, B = rng.randint(1, 6), rng.randint(1, 16), rng.randint(1, 2)
    var, fc = rng.uniform(0.3, 4.0), rng.choice([0.0, 2.0, 5.0])
    gt, gform = _gt(rng, g, B, 4 * Hq, 4 * Wq, 0, D, [0.0, float(D), float(D - 1), 1.0])
    leaves = {"x": torch.randn((B, Dq, Hq, Wq), generator=g, dtype=torch.float64),
              "w": torch.randn((1, 1, 8, 8, 8), generator=g, dtype=torch.float64) / 4.0}
    values = torch.linspace(0, D - 1, D).tolist()

    def dev(m, t, c):
        cost = train_fn.DeconvK8S4Fn.apply(t["x"], t["w"])
        return [StereoFocalLoss(D, focal_coefficient=fc)(cost, c["gt"], var)["stereo_focal_loss_lvl0"],
                DispSmoothL1Loss(D)(SoftArgmin(D)(cost), c["gt"])["l1_loss_lvl0"]]

    def ref(m, t, c):
        cost = _deconv8(t["x"], t["w"])
        sg, mask = HR.map_prep(c["gt"], cost.shape[-2:], D)
        return [HR.focal_level(cost, var, HR.focal_prep(c["gt"], cost.shape, D), fc),
                HR.smooth_l1_level(_soft_argmin(cost, values, 1.0), sg, mask)]
    return _case(("chain_uni", B, Dq, Hq, Wq, var, fc, gform), leaves, dev, ref,
                 [["_FocalLevel", "DeconvK8S4Fn"], ["MapLoss", "SoftArgminFn", "DeconvK8S4Fn"]], consts={"gt": gt})


def _draw_refuse(rng, g):
    """A shape the library documents as unsupported: it must raise DmbLibraryError / NotImplementedError in the forward pass."""
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import fast_cat_fms
    from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.dif_fms import fast_dif_fms
    from densematchingbenchmark_amd.modeling.stereo.disp_predictors import FasterSoftArgmin, SoftArgmin
    from densematchingbenchmark_amd.modeling.stereo.losses import StereoFocalLoss
    what = rng.choice(["softargmin_d", "focal_d", "fast_wide", "fast_small", "scalar_var", "no_normalize"])
    B, H, W = 1, rng.randint(2, 4), rng.randint(2, 9)
    leaves, consts = {}, {}
    if what == "softargmin_d":
        D = rng.choice([257, 300])
        leaves["x"] = torch.randn((B, D, H, W), generator=g, dtype=torch.float64)
        dev = lambda m, t, c: [rng.choice([SoftArgmin, FasterSoftArgmin])(D)(t["x"])]   # noqa: E731
    elif what == "focal_d":
        D = rng.choice([257, 320])
        leaves["x"] = torch.randn((B, D, H, W), generator=g, dtype=torch.float64)
        consts["gt"] = torch.full((B, 1, H, W), 3.0)
        dev = lambda m, t, c: [StereoFocalLoss(D)(t["x"], c["gt"], 1.0)["stereo_focal_loss_lvl0"]]   # noqa: E731
    elif what in ("fast_wide", "fast_small"):
        if what == "fast_wide":
            W, md = rng.choice([1025, 1100]), 4
        else:        # a plane, row or column count of 1: the sampler divides by (size - 1)
            H, W, md = rng.choice([(1, 5, 4), (4, 1, 4), (3, 6, 1)])
        leaves["L"] = torch.randn((B, 3, H, W), generator=g, dtype=torch.float64)
        leaves["R"] = torch.randn((B, 3, H, W), generator=g, dtype=torch.float64)
        f = rng.choice([fast_cat_fms, fast_dif_fms])
        dev = lambda m, t, c: [f(t["L"], t["R"], md)]   # noqa: E731
    elif what == "scalar_var":
        leaves["x"] = torch.randn((B, 4, H, W), generator=g, dtype=torch.float64)
        leaves["v"] = torch.full(rng.choice([(), (1,), (1, 1, 1, 1)]), 1.5, dtype=torch.float64)
        consts["gt"] = torch.full((B, 1, H, W), 1.5)
        dev = lambda m, t, c: [StereoFocalLoss(4)(t["x"], c["gt"], t["v"])["stereo_focal_loss_lvl0"]]   # noqa: E731
    else:
        leaves["x"] = torch.randn((B, 4, H, W), generator=g, dtype=torch.float64)
        dev = lambda m, t, c: [rng.choice([SoftArgmin, FasterSoftArgmin])(4, normalize=False)(t["x"])]   # noqa: E731
    return _case(("refuse", what, B, H, W), leaves, dev, None, [], consts=consts, refuse=True)


# ------------------------------------------------------------------------------------------------------------- running a case
def _made_by(out, names):
    """The names of ``names`` missing from the autograd graph of ``out``."""
    seen, stack, found = set(), [out.grad_fn], set()
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        found.add(type(fn).__name__)
        stack.extend(n for n, _ in fn.next_functions)
    return [n for n in names if n + "Backward" not in found]


def _params(mods):
    return {(i, n): p for i, m in enumerate(mods or []) for n, p in m.named_parameters()}


def _buffers(mods):
    return [{k: v.detach().cpu().clone() for k, v in m.named_buffers()} for m in (mods or [])]


def _leaves(case, dtype, device):
    return {k: v.detach().to(device=device, dtype=dtype, copy=True).requires_grad_(k not in case["nograd"])
            for k, v in case["leaves"].items()}


def _pass(case, mods, t, c, gs):
    for p in _params(mods).values():
        p.grad = None
    outs = case_call(case, mods, t, c)
    sel = [i for i in range(len(outs)) if case["ograd"] is None or case["ograd"][i]]
    torch.autograd.backward([outs[i] for i in sel], [gs[i].to(outs[i].device, outs[i].dtype) for i in sel])
    grads = {("in", k): v.grad for k, v in t.items() if v.requires_grad}
    grads.update({k: p.grad for k, p in _params(mods).items()})
    return outs, grads


def case_call(case, mods, t, c):
    on_dev = any(v.is_cuda for v in t.values())
    return (case["dev"] if on_dev else case["ref"])(mods, t, c)


def _check_case(case, mods, g, dev):
    fails = []
    consts_cpu = dict(case["consts"])
    consts_dev = {k: v.to(dev) for k, v in case["consts"].items()}
    if case["pool"]:
        # the ground truth pooled by the loss classes on the device (torch's pooling there sums in its own order) is the level
        # map both CPU evaluations get: within 8 ulps of the largest pooled summand of the CPU pooling, or the case fails on the
        # pooling itself
        from densematchingbenchmark_amd.modeling.stereo.losses._common import scaled_gt
        levels, sparse = case["pool"]
        consts_cpu["pooled"] = {}
        for hw in levels:
            got = scaled_gt(consts_dev["gt"], tuple(hw), sparse)[0].cpu()
            want = HR.level_gt(consts_cpu["gt"], tuple(hw), sparse)[0]
            top = consts_cpu["gt"].abs().max().item() * hw[1] / consts_cpu["gt"].shape[-1]
            if not (got.double() - want.double()).abs().max().item() <= 9.6e-7 * top:
                fails.append("level %s: the device's pooled ground truth differs from the CPU's by more than 8 ulps" % (hw,))
            consts_cpu["pooled"][tuple(hw)] = got
    refs = {dt: [copy.deepcopy(m).cpu().to(dt) for m in mods] for dt in (torch.float64, torch.float32)}
    with torch.no_grad():     # (on a throwaway copy: a forward in training mode moves the running buffers)
        shapes = [o.shape for o in case_call(case, [copy.deepcopy(m).cpu().double() for m in mods],
                                             _leaves(case, torch.float64, "cpu"), consts_cpu)]
    gs = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    saved = _buffers(mods)
    outs64, grads64 = _pass(case, refs[torch.float64], _leaves(case, torch.float64, "cpu"), consts_cpu, gs)
    outs32, grads32 = _pass(case, refs[torch.float32], _leaves(case, torch.float32, "cpu"), consts_cpu, gs)

    runs = []
    for rep in range(2):
        if rep:
            with torch.no_grad():
                for m, s in zip(mods or [], saved):
                    for k, v in m.named_buffers():
                        if not torch.equal(v.cpu(), s[k]):
                            v.copy_(s[k])
        outs, grads = _pass(case, mods, _leaves(case, torch.float32, dev), consts_dev, gs)
        torch.cuda.synchronize()
        runs.append(([o.detach().cpu() for o in outs], {k: (v.detach().cpu() if v is not None else None) for k, v in grads.items()},
                     _buffers(mods)))
        if rep == 0:
            for i, (o, names) in enumerate(zip(outs, case["fns"])):
                missing = _made_by(o, names)
                if missing:
                    fails.append("output %d: %s not in its graph (made by %s)" % (i, missing, type(o.grad_fn).__name__))
    (outs, grads, bufs), (outs2, grads2, _) = runs
    for i, (o, o64, o32) in enumerate(zip(outs, outs64, outs32)):
        _compare("output %d" % i, o, o64, o32, 0.0, fails)
    for k in grads64:
        if grads64[k] is None and grads.get(k) is not None and not grads[k].any():
            continue      # (the reference's graph left the leaf out -- a level without a valid pixel -- the Function returned zeros)
        _compare("d%s" % (k,), grads.get(k), grads64[k], grads32[k], 0.0, fails)
    for k in grads:
        if k not in grads64:
            fails.append("d%s: no such gradient in the reference" % (k,))
    for i, (m64, b) in enumerate(zip(refs[torch.float64], bufs)):
        for k, v64 in m64.named_buffers():
            got = b[k]
            if v64.dtype == torch.int64:
                if not torch.equal(got, v64):
                    fails.append("module %d %s: %s != %s" % (i, k, got.tolist(), v64.tolist()))
            elif not (got.double() - v64).abs().max().item() <= 1e-5 * max(v64.abs().max().item(), 1e-2):
                fails.append("module %d %s: error %.3e" % (i, k, (got.double() - v64).abs().max().item()))
    for a, b in zip(outs, outs2):
        if not torch.equal(a, b):
            fails.append("second pass: output differs")
    for k, v in grads.items():
        if k in case["nondet"]:
            continue
        if (v is None) != (grads2[k] is None) or (v is not None and not torch.equal(v, grads2[k])):
            fails.append("second pass: d%s not bit-identical" % (k,))
    return fails


def _make_case(seed, dev):
    case = _draw(seed)
    g = torch.Generator().manual_seed(seed)
    mods = case["mods"]() if case["mods"] else []
    _init(mods, g)
    mods = [m.to(dev) for m in mods]
    return case, mods, g


def _check_refusal(case, dev):
    t = _leaves(case, torch.float32, dev)
    c = {k: v.to(dev) for k, v in case["consts"].items()}
    try:
        outs = case["dev"]([], t, c)
    except _lib_errors():
        return []
    torch.autograd.backward(outs, [torch.ones_like(o) for o in outs])      # (it ran: say so, do not leave the graph behind)
    return ["not refused: %s" % ([tuple(o.shape) for o in outs],)]


def _run_chunk(chunk, dev):
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    failures, ran = [], 0
    try:
        for i in range(CASES_PER_CHUNK):
            seed = SEED_BASE + chunk * 1000 + i
            desc = None
            try:
                case, mods, g = _make_case(seed, dev)
                desc = case["desc"]
                fails = _check_refusal(case, dev) if case["refuse"] else _check_case(case, mods, g, dev)
            except Exception as e:  # noqa: BLE001  (a refusal of a supported shape is a failure)
                failures.append((seed, desc, "EXC", repr(e)[:400]))
                continue
            ran += 1
            if fails:
                failures.append((seed, desc, fails[:6]))
    finally:
        torch.set_num_threads(threads)
    return failures, ran


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_head_forward_and_backward_against_fp64(dev, chunk):
    failures, ran = _run_chunk(chunk, dev)
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), ran, "\n".join(map(str, failures)))


# ------------------------------------------------------------------------------------------------------------- fixed draws
FIXED = [97011,     # focal loss, variance-map gradient: the fast exp of the target distribution (fc = 0)
         96003,     # focal loss, cost gradient at fc = 5: the fast exp / log of (1 - P)^-fc
         ]


@pytest.mark.parametrize("seed", FIXED)
def test_head_fixed_draws(dev, seed):
    """Seeds of the regressions the sweep found (smallest failing draw of each), kept whatever SEED_BASE says."""
    case, mods, g = _make_case(seed, dev)
    fails = _check_refusal(case, dev) if case["refuse"] else _check_case(case, mods, g, dev)
    assert not fails, (case["desc"], fails)


# ------------------------------------------------------------------------------------------------------------- coverage
KERNELS = ["volume_bwd_kernel", "cat_wgrad_maps_kernel", "soft_argmin_bwd_kernel", "upsample_regress_bwd_z_kernel",
           "upsample_bwd_z_kernel", "upsample_regress_bwd_hw_kernel", "upsample_bwd_hw_rows_kernel", "deconv_k8s4_dx_kernel",
           "deconv_k8s4_dw_kernel", "deconv_k8s4_dw_reduce_kernel", "avgpool2d_bwd_kernel", "bilinear_ac_bwd_small_kernel",
           "bilinear_hp_bwd_kernel", "warp_volume_bwd_kernel<0>", "warp_volume_bwd_kernel<1>", "warp_volume_bwd_kernel<2>",
           "warp_volume_bwd_samples_kernel", "warp_volume_bwd_rows_kernel", "focal_fwd_kernel", "focal_bwd_kernel",
           "map_loss_fwd_kernel", "map_loss_bwd_kernel", "loss_finalize_kernel"]


def _kernel_pattern(name):
    base, _, arg = name.partition("<")
    if arg:     # the MODE template argument, spelled as a number or as the enumerator
        mode = arg.rstrip(">")
        enum = {"0": "WARP_CAT", "1": "WARP_DIF", "2": "WARP_DIF_NORM"}[mode]
        return r"\b%s<(\(\w+\))?(%s|(\w+::)*%s)>" % (re.escape(base), mode, enum)
    return r"\b%s\b" % re.escape(base)


def test_sweep_reaches_every_backward_kernel(dev):
    """The device side of every draw (no CPU reference) under torch.profiler: every backward / loss kernel of the list must
    launch.  A kernel the draws stop reaching is a sweep that stopped testing it: widen the draw tables."""
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for chunk in range(CHUNKS):
            for i in range(CASES_PER_CHUNK):
                case, mods, g = _make_case(SEED_BASE + chunk * 1000 + i, dev)
                t = _leaves(case, torch.float32, dev)
                c = {k: v.to(dev) for k, v in case["consts"].items()}
                try:
                    outs = case["dev"](mods, t, c)
                except _lib_errors():
                    if case["refuse"]:
                        continue
                    raise
                sel = [o for j, o in enumerate(outs) if case["ograd"] is None or case["ograd"][j]]
                torch.autograd.backward(sel, [torch.randn_like(o) for o in sel])
        torch.cuda.synchronize()
    names = {re.sub(r"\s+", "", e.key) for e in prof.key_averages()}
    missing = [k for k in KERNELS if not any(re.search(_kernel_pattern(k), n) for n in names)]
    assert not missing, "kernels the sweep never launches: %s\nlaunched: %s" % (
        missing, sorted(n[:120] for n in names if "kernel" in n))
