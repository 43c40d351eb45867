"""Randomised forward AND backward sweep of the training-path units against torch's CPU autograd in FP64.

tests/test_backward_gpu.py checks every backward entry point at a dozen hand-picked shapes and the assembled gradients only through
whole models, with bounds loose enough for ReLU flips.  The places where a gradient can be wrong unnoticed are the autograd Functions
of layers/train_fn.py and the launch choices behind them: BatchNorm backward with skip and both ReLU orders, ``dbias`` under batch
versus running statistics, the gradient carry (``dx_acc`` / ``dres_acc``), the stride-2 2-D layers as depth-1 3-D launches, the 5x5
stride-2 layers as space-to-depth 3x3 layers, the odd-extent crop of the stride-2 adjoint, and the weight-gradient tile / staging /
z-segment / slot choices of csrc/wgrad.hip.  This module draws ~250 seeded cases over them:

  one UNIT (FusedConv3d of the three forms, the two 3-D heads, FusedConv2d, the bare 2-D layers of StereoNet / edge-aware
  refinement / PSMNet) or a two-unit CHAIN inside ``train_fn.carry_scope()``, in train() or eval() with trainable weights, with
  BatchNorm none / batch statistics / running statistics / momentum=None / affine=False / track_running_stats=False, bias, skip and
  ReLU options, and the library toggles (split-K, gradient carry, pack group, epilogue statistics) drawn per case.

The reference is the unit's own torch children (deep copies on the CPU, FP64 and again FP32) composed as the module documents.
Every case runs forward and backward with one random upstream gradient ``g`` on all three; ``g`` is zero wherever the FP64
pre-activation of a ReLU lies within MARGIN of zero, so that no ReLU can flip between the runs and EVERY tensor is held to the tight
rule of test_backward_gpu.py: |hip - fp64| <= 4 |fp32 - fp64| + 2e-6 range (floor: 1e-6 of the case's largest gradient).  Also per
case: running buffers within 1e-5 relative, ``num_batches_tracked`` exact, the output made by the intended train_fn Function (no
silent inference-kernel fall-back), and a second identical pass bit-identical (the weight gradients promise a fixed order).  A shape
the library refuses is a failure.  ``DMB_UNIT_GRADS_SEED_BASE`` moves the seeds for open-ended hunts."""
import copy
import math
import os
import random
import re

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CASES_PER_CHUNK = 21
CHUNKS = 12
FLOP_BUDGET = 4e8     # forward multiply-adds x 2 per case: the CPU reference runs forward + backward in FP64 and FP32
MARGIN = 1e-5         # |pre-activation| below MARGIN x max |pre-activation|: the upstream gradient is zero there
SEED_BASE = int(os.environ.get("DMB_UNIT_GRADS_SEED_BASE", "70000"))

W3 = [1, 2, 3, None, 24, 32, 48, 60, 64, 78, 96, 120, 128, 156]     # None: a random width 4 .. 70
CI3 = [1, 3, 8, 16, 32, 33, 48, 64, 96, 128]
CI2 = [1, 3, 4, 8, 20, 32, 64, 128, 192, 320]
BN_OPTS = ["none", "train", "eval", "momentum_none", "affine_false", "no_track"]


# ------------------------------------------------------------------------------------------------------------- the reference
class _RefUnit:
    """torch composition of a FusedConv3d / FusedConv2d: act(BN(conv(x)) + residual) (relu=True), act before the add (relu='pre',
    or skip=: GC-Net's order).  Records the FP64 pre-activation of its ReLU for the margin."""

    def __init__(self, unit, dtype):
        kids = list(unit.children())[:2 if unit.has_bn else 1]
        self.body = nn.Sequential(*[copy.deepcopy(c) for c in kids]).cpu().to(dtype)
        self.pre = None
        for p in self.body.parameters():
            p.grad = None

    def __call__(self, x, residual=None, relu=False, skip=None):
        if skip is not None:
            residual, relu = skip, ("pre" if relu else False)
        y = self.body(x)
        self.pre = None
        if relu == "pre":
            self.pre, y = y, F.relu(y)
        if residual is not None:
            y = y + residual
        if relu is True:
            self.pre, y = y, F.relu(y)
        return y


class _RefPlain:
    """A head / bare layer: the module's own deep copy run by its torch base class (+ the fused residual / skip + ReLU)."""

    def __init__(self, mod, dtype, relu=False):
        self.body = copy.deepcopy(mod).cpu().to(dtype)
        self.base = next(c for c in (nn.ConvTranspose3d, nn.Conv3d, nn.Conv2d) if isinstance(mod, c))
        self.relu, self.pre = relu, None
        for p in self.body.parameters():
            p.grad = None

    def __call__(self, x, residual=None):
        y = self.base.forward(self.body, x)
        if residual is not None:
            y = y + residual
        self.pre = y if self.relu else None
        return F.relu(y) if self.relu else y


def _params(m):
    return dict((m.body if isinstance(m, (_RefUnit, _RefPlain)) else m).named_parameters())


def _buffers(m):
    return dict((m.body if isinstance(m, (_RefUnit, _RefPlain)) else m).named_buffers())


# ------------------------------------------------------------------------------------------------------------- the draws
def _flops(shape_out, ci, taps):
    n = 1
    for e in shape_out:
        n *= e
    return 2.0 * n * ci * taps


def _s2(e):
    return (e - 1) // 2 + 1


def _bn_setup(rng, units, opt):
    """Apply a BatchNorm option to every unit with a BatchNorm (after the unit's own .train(mode))."""
    for u in units:
        if not u.has_bn:
            continue
        C = u.out_planes
        bn_cls = type(u[1])
        if opt == "affine_false":
            u[1] = bn_cls(C, affine=False)
        elif opt == "no_track":
            u[1] = bn_cls(C, track_running_stats=False)
        elif opt == "momentum_none":
            u[1].momentum = None
        u[1].train(opt in ("train", "momentum_none", "affine_false") or (opt == "no_track" and rng.random() < 0.5))


def _init(mods, g):
    """Seeded parameters and buffers: fan-in-normalised weights, non-trivial BatchNorm affine and running statistics."""
    with torch.no_grad():
        for m in mods:
            for mod in m.modules():
                if isinstance(mod, (nn.Conv2d, nn.Conv3d, nn.ConvTranspose3d)):
                    w = mod.weight
                    fan = w[0].numel() if not isinstance(mod, nn.ConvTranspose3d) else w.shape[0] * 27 / 8.0
                    w.copy_(torch.randn(w.shape, generator=g) / math.sqrt(fan))
                    if mod.bias is not None:
                        mod.bias.copy_(0.1 * torch.randn(mod.bias.shape, generator=g))
                elif isinstance(mod, nn.modules.batchnorm._BatchNorm):
                    C = mod.num_features
                    if mod.affine:
                        mod.weight.copy_(1.0 + 0.3 * torch.randn(C, generator=g))
                        mod.bias.copy_(0.2 * torch.randn(C, generator=g))
                    if mod.track_running_stats:
                        mod.running_mean.copy_(0.3 * torch.randn(C, generator=g))
                        mod.running_var.copy_(0.5 + torch.rand(C, generator=g))
                        mod.num_batches_tracked.fill_(int(torch.randint(0, 6, (1,), generator=g)))


def _toggles(rng):
    return dict(split_k=rng.random() < 0.7, carry=rng.random() < 0.7, pack_group=rng.random() < 0.7, epilogue=rng.random() < 0.5)


def _w3(rng):
    w = rng.choice(W3)
    return rng.randint(4, 70) if w is None else w


def _draw(seed):
    """-> the case: desc, make(dev) -> device modules, inputs {name: shape}, call(mods, t) -> outputs, fns (expected Functions),
    toggles, batch-stat sizes (for the >= 8 values per channel rule)."""
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d, HeadConv3d, HeadDeconv3d
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers_2d import FusedConv2d
    rng = random.Random(seed)
    kind = rng.choice(["s1", "s1", "s1", "s2", "s2", "s2", "deconv", "deconv", "head", "hdeconv", "c2d", "c2d", "c2d", "c2d",
                       "hip5", "reshead", "bare1x1", "chain3", "chain3", "chain2", "chain2"])
    tg = _toggles(rng)
    mode = rng.choice(["train", "train", "eval"])
    bn_opt = rng.choice(BN_OPTS)
    bias = rng.random() < 0.5
    relu = rng.choice([False, True, "pre"])
    extra = rng.choice(["none", "residual", "skip"])
    B = rng.randint(1, 4)

    if kind in ("s1", "s2", "deconv"):
        D, H, W = rng.randint(1, 12), rng.randint(1, 17), _w3(rng)
        Ci = rng.choice(CI3)
        if rng.random() < 0.3:
            # a deep, narrow volume: enough work items per weight-gradient slot for the tile / z-segment choices of the larger
            # launches (the 4 x 8 stride-2 tile needs two z segments of >= 4 planes in a round)
            D, H, Ci = rng.randint(8, 12), rng.randint(8, 17), rng.choice(CI3[:5])
        if kind == "s2":      # each big extent 2n or 2n - 1
            D, H, W = [e - 1 if e > 1 and e % 2 == 0 and rng.random() < 0.5 else e for e in (D, H, W)]
        Co = rng.choice([32, 64, 128]) if kind != "deconv" else rng.choice([rng.randint(1, 32), 16, 32, 64])
        out_sp = lambda D, H, W: ((D, H, W) if kind == "s1" else (_s2(D), _s2(H), _s2(W)) if kind == "s2" else (2 * D, 2 * H, 2 * W))
        # (a transposed layer: 27 taps per INPUT voxel)
        while B * _flops(out_sp(D, H, W) if kind != "deconv" else (D, H, W), Ci * Co, 27) > FLOP_BUDGET and (B > 1 or D > 1 or H > 1):
            if B > 1:
                B -= 1
            elif D > 1:
                D -= 1
            else:
                H -= 1
        osz = out_sp(D, H, W)

        def make(dev):
            u = FusedConv3d(bn_opt != "none", Ci, Co, 3, 1 if kind == "s1" else 2, 1, 1, bias, transposed=kind == "deconv",
                            output_padding=1 if kind == "deconv" else 0)
            u.train(mode == "train")
            _bn_setup(rng, [u], bn_opt)
            return [u]
        inputs = {"x": (B, Ci, D, H, W)}
        if extra != "none":
            inputs["r"] = (B, Co) + osz
        kw = "residual" if extra == "residual" else "skip"
        call = lambda m, t: [m[0](t["x"], relu=relu, **({kw: t["r"]} if "r" in t else {}))]   # noqa: E731
        return dict(desc=(kind, B, Ci, Co, D, H, W, bn_opt, mode, bias, relu, extra), make=make, inputs=inputs, call=call,
                    fns=["ConvUnitFn"], toggles=tg, stat_n=[B * osz[0] * osz[1] * osz[2]] if bn_opt != "none" else [])

    if kind in ("head", "hdeconv"):
        D, H, W = rng.randint(1, 12), rng.randint(1, 17), _w3(rng)
        Ci = rng.choice(CI3)
        Co = 1 if kind == "head" else rng.choice([1, rng.randint(1, 32), 32])
        while B * _flops((D, H, W), Ci * Co, 27) > FLOP_BUDGET and (B > 1 or D > 1 or H > 1):
            if B > 1:
                B -= 1
            elif D > 1:
                D -= 1
            else:
                H -= 1
        hbias = kind == "hdeconv" or rng.random() < 0.7
        with_res = kind == "head" and rng.random() < 0.7

        def make(dev):
            u = HeadConv3d(Ci, bias=hbias) if kind == "head" else HeadDeconv3d(Ci, Co)
            u.train(mode == "train")
            return [u]
        inputs = {"x": (B, Ci, D, H, W)}
        if with_res:
            inputs["r"] = (B, 1, D, H, W)
        call = lambda m, t: [m[0](t["x"], t["r"]) if "r" in t else m[0](t["x"])]   # noqa: E731
        return dict(desc=(kind, B, Ci, Co, D, H, W, mode, hbias, with_res), make=make, inputs=inputs, call=call,
                    fns=["HeadConvFn" if kind == "head" else "HeadDeconvFn"], toggles=tg, stat_n=[])

    if kind in ("c2d", "hip5", "reshead", "bare1x1"):
        H, W = rng.randint(1, 40), rng.choice([rng.randint(1, 100), rng.randint(1, 100), 16, 48, 52, 96, 100, 64])
        if kind == "c2d":
            k, s, dil = rng.choice([(1, 1, 1), (3, 1, 1), (3, 1, 1), (3, 1, 2), (3, 1, 4), (3, 1, 8), (3, 2, 1), (3, 2, 1), (1, 2, 1),
                                    (5, 2, 1)])
            Co = rng.choice([1, 8, 32] if (dil > 2 or k == 5) else ([16, 32, 64] if s == 2 else [1, 32, 64, 128]))
        elif kind == "hip5":
            k, s, dil, Co = 5, 2, 1, 32
            H, W = 2 * rng.randint(1, 20), 2 * rng.randint(1, 50)      # StereoNet's down-sampling: even sizes
        elif kind == "reshead":
            k, s, dil, Co = 3, 1, 1, 1
        else:
            k, s, dil, Co = 1, 1, 1, rng.choice([32, 64])
        Ci = rng.choice(CI2) if kind not in ("hip5", "reshead") else (rng.choice([3, 32]) if kind == "hip5" else 32)
        if kind == "c2d" and (k, s) == (3, 2) and rng.random() < 0.5:
            Ci = rng.choice(CI2[-3:])    # wide inputs: few weight-gradient slots per channel block, the 4 x 8 stride-2 tile's regime
        if kind == "bare1x1":
            Ci = rng.choice([128, 64, 32])
        Ho, Wo = (H, W) if s == 1 else (_s2(H), _s2(W))
        while B * _flops((Ho, Wo), Ci * Co, k * k) > FLOP_BUDGET and (B > 1 or H > 2):
            if B > 1:
                B -= 1
            else:
                H -= 2 if kind == "hip5" else 1
                Ho = H if s == 1 else _s2(H)

        def make(dev):
            if kind == "c2d":
                u = FusedConv2d(bn_opt != "none", Ci, Co, k, s, dil * (k // 2), dil, bias)
                u.train(mode == "train")
                _bn_setup(rng, [u], bn_opt)
                return [u]
            from densematchingbenchmark_amd.modeling.stereo.backbones.StereoNet import _HipConv2d
            from densematchingbenchmark_amd.modeling.stereo.backbones.PSMNet import _BareConv1x1
            from densematchingbenchmark_amd.modeling.stereo.disp_refinement.utils.edge_aware import _ResidualHead
            u = _HipConv2d(Ci, Co, 5, 2, 2) if kind == "hip5" else _ResidualHead(Ci) if kind == "reshead" else _BareConv1x1(Ci, Co)
            u.train(mode == "train")
            return [u]
        inputs = {"x": (B, Ci, H, W)}
        if kind == "c2d":
            if extra != "none":
                inputs["r"] = (B, Co, Ho, Wo)
            act = relu if extra != "skip" else ("pre" if relu else False)
            call = lambda m, t: [m[0](t["x"], t.get("r"), act)]   # noqa: E731
            fns, desc = ["Conv2dUnitFn"], (kind, B, Ci, Co, H, W, k, s, dil, bn_opt, mode, bias, act, extra)
        elif kind == "reshead":
            inputs["r"] = (B, 1, H, W)
            call = lambda m, t: [m[0](t["x"], t["r"])]   # noqa: E731
            fns, desc = ["BareConv2dFn"], (kind, B, Ci, H, W, mode)
        else:
            call = lambda m, t: [m[0](t["x"])]   # noqa: E731
            fns, desc = ["BareConv2dFn" if kind == "hip5" else "BareConv1x1Fn"], (kind, B, Ci, Co, H, W, mode)
        return dict(desc=desc, make=make, inputs=inputs, call=call, fns=fns, toggles=tg,
                    stat_n=[B * Ho * Wo] if kind == "c2d" and bn_opt != "none" else [])

    if kind == "chain3":
        # seq: a = u1(x), b = u2(a, residual=x) (stride-1 pair, or the hourglass's stride-2 + transposed pair on even extents);
        # fan: a = u1(x), b = u2(x) -- x has two consumers either way, so the gradient carry hands u2's share to u1 as dx_acc
        form = rng.choice(["s1s1", "s2de", "fan"])
        D, H, W = rng.randint(1, 8), rng.randint(1, 12), _w3(rng)
        if form == "s2de":
            D, H, W = 2 * max(1, D // 2), 2 * max(1, H // 2), 2 * max(1, W // 2)
        Ci = rng.choice([32, 64]) if form != "fan" else rng.choice(CI3)
        C = rng.choice([32, 64])
        s1, s2 = (1, 1) if form == "s1s1" else (2, 1) if form == "s2de" else (rng.choice([1, 2]), rng.choice([1, 2]))
        C2 = Ci if form != "fan" else rng.choice([32, 64])
        osz1 = (D, H, W) if s1 == 1 else (_s2(D), _s2(H), _s2(W))
        while B * (_flops(osz1, Ci * C, 27) + _flops(osz1 if form == "s2de" else (D, H, W), C * C2, 27)) > FLOP_BUDGET \
                and (B > 1 or D > 2 or H > 2):
            if B > 1:
                B -= 1
            elif D > 2:
                D -= 2 if form == "s2de" else 1
            else:
                H -= 2 if form == "s2de" else 1
            osz1 = (D, H, W) if s1 == 1 else (_s2(D), _s2(H), _s2(W))
        osz2 = (D, H, W) if (form != "fan" or s2 == 1) else (_s2(D), _s2(H), _s2(W))
        relu1 = False if form != "fan" else relu
        relu2 = rng.choice([False, True, "pre"])

        def make(dev):
            if form == "fan":
                u1, u2 = FusedConv3d(bn_opt != "none", Ci, C, 3, s1, 1, 1, bias), FusedConv3d(bn_opt != "none", Ci, C2, 3, s2, 1, 1, bias)
            else:
                u1 = FusedConv3d(bn_opt != "none", Ci, C, 3, s1, 1, 1, bias)
                u2 = FusedConv3d(bn_opt != "none", C, Ci, 3, 2 if form == "s2de" else 1, 1, 1, bias, transposed=form == "s2de",
                                 output_padding=1 if form == "s2de" else 0)
            for u in (u1, u2):
                u.train(mode == "train")
            _bn_setup(rng, [u1, u2], bn_opt)
            return [u1, u2]
        inputs = {"x": (B, Ci, D, H, W)}
        if form == "fan":
            call = lambda m, t: [m[0](t["x"], relu=relu1), m[1](t["x"], relu=relu2)]   # noqa: E731
        else:
            def call(m, t):
                a = m[0](t["x"], relu=relu1)
                return [a, m[1](a, residual=t["x"], relu=relu2)]
        n1 = B * osz1[0] * osz1[1] * osz1[2]
        n2 = B * osz2[0] * osz2[1] * osz2[2]
        return dict(desc=(kind, form, B, Ci, C, C2, D, H, W, s1, s2, bn_opt, mode, bias, relu1, relu2), make=make, inputs=inputs,
                    call=call, fns=["ConvUnitFn", "ConvUnitFn"], toggles=tg, stat_n=[n1, n2] if bn_opt != "none" else [])

    # chain2: the BasicBlock (seq: conv2(conv1(x), residual=x)) and the down-sampling block's fan-out (conv1 and downsample both
    # read x: the stride-2 data gradients take the other consumer's share as dx_acc)
    form = rng.choice(["seq", "fan"])
    H, W = rng.randint(2, 40), rng.choice([rng.randint(2, 100), 16, 48, 64])
    Ci = rng.choice([32, 64]) if form == "seq" else rng.choice(CI2[:8])
    if form == "seq":
        k1, s1, d1 = rng.choice([(3, 1, 1), (3, 1, 2), (1, 1, 1), (3, 1, 4)])
        k2, s2, d2 = 3, 1, (d1 if k1 == 3 else 1)
        C = 32
        C2 = Ci
    else:
        k1, s1, d1 = rng.choice([(3, 2, 1), (3, 2, 1), (5, 2, 1), (1, 2, 1)])
        k2, s2, d2 = rng.choice([(1, 2, 1), (3, 2, 1), (3, 1, 1)])
        C, C2 = 32, rng.choice([32, 64])
    if d2 > 2 and C2 > 32:
        d2 = 1
    Ho1, Wo1 = (H, W) if s1 == 1 else (_s2(H), _s2(W))
    Ho2, Wo2 = (H, W) if s2 == 1 else (_s2(H), _s2(W))
    while B * (_flops((Ho1, Wo1), Ci * C, k1 * k1) + _flops((Ho2, Wo2), (C if form == "seq" else Ci) * C2, k2 * k2)) > FLOP_BUDGET and B > 1:
        B -= 1
    relu1 = False if form == "seq" else relu
    relu2 = rng.choice([False, True, "pre"])

    def make(dev):
        u1 = FusedConv2d(bn_opt != "none", Ci, C, k1, s1, d1 * (k1 // 2), d1, bias)
        u2 = FusedConv2d(bn_opt != "none", C if form == "seq" else Ci, C2, k2, s2, d2 * (k2 // 2), d2, bias)
        for u in (u1, u2):
            u.train(mode == "train")
        _bn_setup(rng, [u1, u2], bn_opt)
        return [u1, u2]
    inputs = {"x": (B, Ci, H, W)}
    if form == "fan":
        call = lambda m, t: [m[0](t["x"], None, relu1), m[1](t["x"], None, relu2)]   # noqa: E731
    else:
        def call(m, t):
            a = m[0](t["x"], None, relu1)
            return [a, m[1](a, t["x"], relu2)]
    return dict(desc=("chain2", form, B, Ci, C, C2, H, W, (k1, s1, d1), (k2, s2, d2), bn_opt, mode, bias, relu1, relu2), make=make,
                inputs=inputs, call=call, fns=["Conv2dUnitFn", "Conv2dUnitFn"], toggles=tg,
                stat_n=[B * Ho1 * Wo1, B * Ho2 * Wo2] if bn_opt != "none" else [])


def _batch_stat_units(mods):
    """nn.BatchNorm's rule: batch statistics in training mode and wherever there are no running buffers."""
    return [getattr(m, "has_bn", False) and (m[1].training or m[1].running_mean is None) for m in mods]


# ------------------------------------------------------------------------------------------------------------- running a case
class _Toggles:
    def __init__(self, tg):
        self.tg = tg

    def __enter__(self):
        from densematchingbenchmark_amd import ops
        from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
        self.before = (ops.split_k(), train_fn._carry_enabled, train_fn._pack_group_enabled, train_fn._epilogue_stats)
        ops.set_split_k(self.tg["split_k"])
        train_fn.set_gradient_carry(self.tg["carry"])
        train_fn.set_pack_group(self.tg["pack_group"])
        train_fn.set_epilogue_stats(self.tg["epilogue"])
        return self

    def __exit__(self, *exc):
        from densematchingbenchmark_amd import ops
        from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
        sk, carry, pg, ep = self.before
        ops.set_split_k(sk)
        train_fn.set_gradient_carry(carry)
        train_fn.set_pack_group(pg)
        train_fn.set_epilogue_stats(ep)
        return False


def _leaves(t64, dtype, device):
    return {k: v.detach().to(device=device, dtype=dtype, copy=True).requires_grad_() for k, v in t64.items()}


def _pass(mods, call, t, gs, carry_scope=None):
    """Forward + backward of <outputs, gs>; -> (outputs, {key: gradient}).  Keys: ('in', name) and (unit index, parameter name)."""
    for m in mods:
        for p in _params(m).values():
            p.grad = None
    if carry_scope is not None:
        with carry_scope():
            outs = call(mods, t)
    else:
        outs = call(mods, t)
    torch.autograd.backward(outs, [g.to(o.device, o.dtype) for o, g in zip(outs, gs)])
    grads = {("in", k): v.grad for k, v in t.items()}
    for i, m in enumerate(mods):
        for n, p in _params(m).items():
            grads[(i, n)] = p.grad
    return outs, grads


def _upstream(outs64, pres, g):
    gs = []
    for o, pre in zip(outs64, pres):
        gi = torch.randn(o.shape, generator=g, dtype=torch.float64)
        if pre is not None:
            pre = pre.detach()
            gi[pre.abs() < MARGIN * pre.abs().max()] = 0.0
        gs.append(gi)
    return gs


def _compare(tag, got, r64, r32, floor, fails):
    if got is None or r64 is None:
        if (got is None) != (r64 is None):
            fails.append("%s: gradient %s on the device, %s in the reference" % (tag, got is not None, r64 is not None))
        return
    got = got.detach().cpu().double()
    r64, r32 = r64.detach().double(), r32.detach().double()
    if got.shape != r64.shape:
        fails.append("%s: shape %s != %s" % (tag, tuple(got.shape), tuple(r64.shape)))
        return
    if got.numel() == 0:
        return
    scale = r64.abs().max().item()
    err = (got - r64).abs().max().item()
    own = (r32 - r64).abs().max().item()
    bound = max(4 * own + 2e-6 * scale, floor)
    if not err <= bound:       # (NaN fails too)
        fails.append("%s: error %.3e > bound %.3e (fp32 error %.3e, range %.3e)" % (tag, err, bound, own, scale))


def _check_case(case, mods, t64, dev, g):
    """Reference (FP64, FP32) and device runs of one case with the current parameters / buffers of ``mods``; -> failure strings."""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    fails = []
    ref64 = [(_RefUnit if hasattr(m, "has_bn") else _RefPlain)(m, torch.float64, **({} if hasattr(m, "has_bn") else
                                                                                    {"relu": _plain_relu(m)})) for m in mods]
    ref32 = [(_RefUnit if hasattr(m, "has_bn") else _RefPlain)(m, torch.float32, **({} if hasattr(m, "has_bn") else
                                                                                    {"relu": _plain_relu(m)})) for m in mods]
    saved = [{k: v.detach().clone() for k, v in _buffers(m).items()} for m in mods]
    # FP64 forward first: its pre-activations decide where the upstream gradient must be zero
    t_64 = _leaves(t64, torch.float64, "cpu")
    outs64 = case["call"](ref64, t_64)
    gs = _upstream(outs64, [r.pre for r in ref64], g)
    torch.autograd.backward(outs64, gs)
    grads64 = {("in", k): v.grad for k, v in t_64.items()}
    for i, m in enumerate(ref64):
        for n, p in _params(m).items():
            grads64[(i, n)] = p.grad
    outs32, grads32 = _pass(ref32, case["call"], _leaves(t64, torch.float32, "cpu"), gs)

    runs = []
    for rep in range(2):
        if rep:
            with torch.no_grad():     # (only what the first pass changed: a copy moves the buffer's version, a cache key)
                for m, s in zip(mods, saved):
                    for k, v in _buffers(m).items():
                        if not torch.equal(v, s[k].to(v.device)):
                            v.copy_(s[k])
        with _Toggles(case["toggles"]):
            outs, grads = _pass(mods, case["call"], _leaves(t64, torch.float32, dev), gs, train_fn.carry_scope)
        torch.cuda.synchronize()
        bufs = [{k: v.detach().cpu().clone() for k, v in _buffers(m).items()} for m in mods]
        runs.append(([o.detach().cpu() for o in outs], {k: (v.detach().cpu() if v is not None else None) for k, v in grads.items()}, bufs))
        if rep == 0:
            for i, (o, fn) in enumerate(zip(outs, case["fns"])):
                name = type(o.grad_fn).__name__ if o.grad_fn is not None else None
                if name != fn + "Backward":
                    fails.append("output %d made by %s, not %s" % (i, name, fn))
    (outs, grads, bufs), (outs2, grads2, bufs2) = runs

    gmax = max([v.detach().abs().max().item() for v in grads64.values() if v is not None and v.numel()] + [0.0])
    for i, (o, o64, o32) in enumerate(zip(outs, outs64, outs32)):
        _compare("output %d" % i, o, o64, o32, 0.0, fails)
    for k in grads64:
        _compare("d%s" % (k,), grads.get(k), grads64[k], grads32[k], 1e-6 * gmax, fails)
    for k in grads:
        if k not in grads64:
            fails.append("d%s: no such gradient in the reference" % (k,))
    for i, (m64, b) in enumerate(zip(ref64, bufs)):
        for k, v64 in _buffers(m64).items():
            got = b[k]
            if v64.dtype == torch.int64:
                if not torch.equal(got, v64):
                    fails.append("unit %d %s: %s != %s" % (i, k, got.tolist(), v64.tolist()))
            elif not (got.double() - v64).abs().max().item() <= 1e-5 * max(v64.abs().max().item(), 1e-2):
                fails.append("unit %d %s: error %.3e" % (i, k, (got.double() - v64).abs().max().item()))
    for a, b in zip(outs, outs2):
        if not torch.equal(a, b):
            fails.append("second pass: output differs")
    for k, v in grads.items():
        if (v is None) != (grads2[k] is None) or (v is not None and not torch.equal(v, grads2[k])):
            fails.append("second pass: d%s not bit-identical" % (k,))
    return fails


def _plain_relu(m):
    from densematchingbenchmark_amd.modeling.stereo.disp_refinement.utils.edge_aware import _ResidualHead
    return isinstance(m, _ResidualHead)


def _make_case(seed, dev):
    case = _draw(seed)
    g = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    mods = case["make"](dev)
    _init(mods, g)
    mods = [m.to(dev) for m in mods]
    for m in mods:
        for p in m.parameters():
            p.requires_grad_(True)
    for n, bs in zip(case["stat_n"], _batch_stat_units(mods)):
        if bs and n < 8:
            return case, None, None, g          # torch needs > 1 value per channel; fewer than 8 is a degenerate draw
    t64 = {k: torch.randn(s, generator=g, dtype=torch.float64) for k, s in case["inputs"].items()}
    return case, mods, t64, g


def _run_chunk(chunk, dev):
    threads = torch.get_num_threads()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    failures, ran = [], 0
    try:
        for i in range(CASES_PER_CHUNK):
            seed = SEED_BASE + chunk * 1000 + i
            desc = None
            try:
                case, mods, t64, g = _make_case(seed, dev)
                desc = case["desc"]
                if mods is None:
                    continue
                fails = _check_case(case, mods, t64, dev, g)
            except Exception as e:  # noqa: BLE001  (a shape the library refuses is a failure too: every drawn shape is legal)
                failures.append((seed, desc, "EXC", repr(e)[:400]))
                continue
            ran += 1
            if fails:
                failures.append((seed, desc, case["toggles"], fails[:6]))
    finally:
        torch.set_num_threads(threads)
    return failures, ran


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_unit_forward_and_backward_against_fp64(dev, chunk):
    failures, ran = _run_chunk(chunk, dev)
    assert not failures, "%d of %d cases failed:\n%s" % (len(failures), ran, "\n".join(map(str, failures)))
    assert ran >= CASES_PER_CHUNK - 4


# ------------------------------------------------------------------------------------------------------------- coverage
WGRAD_FORMS = {
    "conv3d_wgrad_s1_kernel<true,24>": r"conv3d_wgrad_s1_kernel<true,24>",
    "conv3d_wgrad_s1_kernel<true,32>": r"conv3d_wgrad_s1_kernel<true,32>",
    "conv3d_wgrad_s1_kernel<false,24>": r"conv3d_wgrad_s1_kernel<false,24>",
    "conv3d_wgrad_s2_kernel<Wg2Cfg<2,12>,true>": r"conv3d_wgrad_s2_kernel<(\w+::)*Wg2Cfg<2,12>,true>",
    "conv3d_wgrad_s2_kernel<Wg2Cfg<2,12>,false>": r"conv3d_wgrad_s2_kernel<(\w+::)*Wg2Cfg<2,12>,false>",
    "conv3d_wgrad_s2_kernel<Wg2Cfg<4,8>,true>": r"conv3d_wgrad_s2_kernel<(\w+::)*Wg2Cfg<4,8>,true>",
    "conv3d_wgrad_s2_kernel<Wg2Cfg<4,8>,false>": r"conv3d_wgrad_s2_kernel<(\w+::)*Wg2Cfg<4,8>,false>",
    "conv3d_c1_wgrad_kernel": r"conv3d_c1_wgrad_kernel\b",
    "conv2d_wgrad_kernel<3,1>": r"conv2d_wgrad_kernel<3,1>",
    "conv2d_wgrad_kernel<3,2>": r"conv2d_wgrad_kernel<3,2>",
    "conv2d_wgrad_kernel<3,4>": r"conv2d_wgrad_kernel<3,4>",
    "conv2d_wgrad_kernel<3,8>": r"conv2d_wgrad_kernel<3,8>",
    "conv2d_wgrad_kernel<1,1>": r"conv2d_wgrad_kernel<1,1>",
}


def test_sweep_reaches_every_weight_gradient_form(dev):
    """The device side of every draw of the sweep (no CPU reference) under torch.profiler: the launched kernel names must cover every
    weight-gradient instantiation of csrc/wgrad.hip.  A form the draws stop reaching (a cost model there changed) is a sweep that
    stopped testing it: widen the draw tables."""
    from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
    with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        for chunk in range(CHUNKS):
            for i in range(CASES_PER_CHUNK):
                case, mods, t64, g = _make_case(SEED_BASE + chunk * 1000 + i, dev)
                if mods is None:
                    continue
                with _Toggles(case["toggles"]):
                    t = _leaves(t64, torch.float32, dev)
                    with train_fn.carry_scope():
                        outs = case["call"](mods, t)
                    torch.autograd.backward(outs, [torch.randn_like(o) for o in outs])
        torch.cuda.synchronize()
    names = {re.sub(r"\s+", "", e.key) for e in prof.key_averages()}
    missing = [form for form, pat in WGRAD_FORMS.items() if not any(re.search(pat, n) for n in names)]
    assert not missing, "weight-gradient forms the sweep never launches: %s\nlaunched: %s" % (
        missing, sorted(n[:120] for n in names if "wgrad" in n))


# ------------------------------------------------------------------------------------------------------------- two steps
@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("dim", [3, 2])
def test_two_steps_with_a_fused_optimizer(dev, dim, mode):
    """Forward + backward, Adam(fused=True).step(), forward + backward again in the same mode -- in eval() (frozen BatchNorm,
    trainable weights) also a torch.no_grad() pass before and after the step, which takes the fused inference kernels and the
    unit's packed / folded parameters.  A fused step leaves ``_version`` alone: every comparison loads the reference with the
    device's parameters and buffers of that moment, so packs or folded BatchNorm from before the step fail it."""
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers import FusedConv3d
    from densematchingbenchmark_amd.modeling.stereo.layers.basic_layers_2d import FusedConv2d
    g = torch.Generator().manual_seed(4242 + dim)
    if dim == 3:
        u = FusedConv3d(True, 32, 32, 3, 1, 1, 1, True)
        shape = (2, 32, 4, 6, 24)
        call = lambda m, t: [m[0](t["x"], residual=t["r"], relu=True)]   # noqa: E731
        fn = "ConvUnitFn"
    else:
        u = FusedConv2d(True, 32, 64, 3, 1, 1, 1, True)
        shape = (2, 32, 10, 28)
        call = lambda m, t: [m[0](t["x"], t["r"], True)]   # noqa: E731
        fn = "Conv2dUnitFn"
    _init([u], g)
    u = u.to(dev)
    u.train(mode == "train")
    t64 = {"x": torch.randn(shape, generator=g, dtype=torch.float64),
           "r": torch.randn((shape[0], u.out_planes) + shape[2:], generator=g, dtype=torch.float64)}
    case = dict(call=call, fns=[fn], toggles=dict(split_k=True, carry=True, pack_group=True, epilogue=False))
    opt = torch.optim.Adam(list(u.parameters()), lr=0.05, fused=True)

    def no_grad_pass(what):
        ref, ref32 = _RefUnit(u, torch.float64), _RefUnit(u, torch.float32)
        with torch.no_grad():
            got = call([u], {k: v.float().to(dev) for k, v in t64.items()})[0].cpu()
            r64 = call([ref], t64)[0]
            r32 = call([ref32], {k: v.float() for k, v in t64.items()})[0]
        fails = []
        _compare("%s: no_grad output" % what, got, r64, r32, 0.0, fails)
        return fails

    fails = []
    if mode == "eval":
        fails += no_grad_pass("before the step")          # fills the inference path's packs with the initial weights
    fails += ["step 0: " + f for f in _check_case(case, [u], t64, dev, g)]
    v = u[0].weight._version
    opt.step()
    assert u[0].weight._version == v                      # the premise: a fused step leaves the version alone
    fails += ["step 1: " + f for f in _check_case(case, [u], t64, dev, g)]
    if mode == "eval":
        fails += no_grad_pass("after the step")
    assert not fails, "\n".join(fails)
