"""The hand-placed inputs of tests/test_value_edges_gpu.py (tests/_value_edges.py) and the distributions of
tests/test_conditioning_gpu.py (tests/_values.py), checked on the CPU: the constructions are exact in FP32 (a difference meant to be
1 IS 1, a tie is a tie), the FP32 references stay close to their FP64 evaluation (so 4x their error is a yardstick, neither vacuous
nor enormous), the centre-tap convolution carries the mean it is meant to carry, and everything is deterministic."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dmb_oracle as O
from tests import _values as V
from tests._value_edges import (EPE_BOUNDS, EPE_ORIGINAL, FOCAL_D, FOCAL_OFF_SAMPLE, FOCAL_SETTINGS, FOCAL_STEEP, GAINS, LOGITS, MAP, MAP_BOUNDS, QUANTILE_BOUNDS, SOFT_SHAPE, THETA, TIE_SHAPES, around, epe_case, epe_expected, epe_pairs, focal_case, focal_geometry, focal_off_sample_case, focal_reference, map_loss_reference, nll_case, nxt, quantile_case, quantile_reference, smooth_l1_case, soft_argmin_case, tie_case, tie_reference)


def test_epe_pairs_are_exact():
    pairs = epe_pairs()
    errs = sorted(set(err for _, _, err in pairs))
    assert errs == sorted(e for T in (1.0, 2.0, 3.0, 5.0) for e in around(T))          # every threshold, both neighbours
    assert {(err, est > gt) for gt, est, err in pairs} >= {(e, s) for e in errs for s in (False, True)}   # either side
    for gt, est, err in pairs:
        assert abs(np.float32(gt) - np.float32(est)) == np.float32(err) and EPE_BOUNDS[0] < gt < EPE_BOUNDS[1]
    ests, gt = epe_case()
    for e in ests:                                                     # the +/- 0.5 copies keep exact differences too
        assert torch.equal((gt.double() - e.double()).float().double(), gt.double() - e.double())
    inner = O.remove_padding(gt[1:2], EPE_ORIGINAL)
    m = (inner > 0) & (inner < 192)
    d = (inner - O.remove_padding(ests[0][1:2], EPE_ORIGINAL)).abs()[m]
    assert int(m.sum()) == len(pairs) and set(d.tolist()) == set(np.float32(errs).tolist())
    g0 = O.remove_padding(gt[0:1], EPE_ORIGINAL)
    assert (g0 == 0.0).any() and (g0 == 192.0).any()
    # the reference's own FP32 percentages agree with the FP64 expectation to FP32 rounding
    ref, n = O.dataset_metrics([ests[0]], [gt], EPE_ORIGINAL, *EPE_BOUNDS)
    exp = epe_expected(ests[0], gt)
    assert n == exp[0] == 2
    for i, k in enumerate(("epe", "1px", "2px", "3px", "5px")):
        assert abs(ref[k] * n - exp[1 + i]) <= 4 * 2.0 ** -24 * n * max(abs(exp[1 + i]), 1.0), k


@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("shape", TIE_SHAPES)
def test_relu_ties_are_ties(shape, relu):
    c, res, dy = tie_case(shape, relu)
    seen = c if relu == 2 else c + res
    n = seen.numel()
    for count in ((seen == 0).sum(), (seen > 0).sum(), (seen < 0).sum()):
        assert abs(int(count) - n / 3) <= 2
    assert (res != 0).all() if relu == 2 else True
    assert (dy != 0).all() and torch.equal(c, c.round()) and torch.equal(res, res.round())
    ref, ref64 = tie_reference(c, res, dy, relu), tie_reference(c, res, dy, relu, torch.float64)
    # torch's ReLU passes nothing at a tie; FP32 and FP64 agree bit for bit on these integers
    assert torch.equal(ref["y"].double(), ref64["y"]) and torch.equal(ref["dc"].double(), ref64["dc"])
    if relu:
        assert torch.equal(ref["dc"] != 0, seen > 0)
    assert torch.equal(ref["dres"] != 0, seen > 0 if relu == 1 else torch.ones_like(seen, dtype=torch.bool))


@pytest.mark.parametrize("D", [1, 5, 192])
def test_soft_argmin_columns(D):
    x, kinds, peaks = soft_argmin_case(D)
    vals = O.disp_sample_values(D).double()
    ref64 = O.soft_argmin_f64(x, D)[:, 0]
    ref32 = O.soft_argmin(x, D)[:, 0]
    one_hot = kinds < 3
    assert (ref64[one_hot] - vals[peaks[..., 0][one_hot]]).abs().max() <= 1e-30                # exp(-99) and below next to 1
    two = kinds == 3
    assert (ref64[two] - (vals[peaks[..., 0][two]] + vals[peaks[..., 1][two]]) / 2).abs().max() <= 1e-12 * max(D, 1)
    flat = kinds >= 4
    assert (ref64[flat] - (D - 1) / 2).abs().max() <= 1e-12 * D
    assert (ref32.double() - ref64).abs().max() <= 2e-6 * max(1.0, float(ref64.abs().max()))
    assert torch.isfinite(x).all()


# ---------------------------------------------------------------------------------------------- references against FP64
def _within(ref32, ref64, factor=1.0):
    rng = float(ref64.abs().max())
    return float((ref32.double() - ref64).abs().max()) <= factor * V.FLOOR * rng


def test_loss_references_stay_close_to_fp64():
    """The FP32 CPU evaluation of every section-A loss case meets its own FP64 evaluation within the floor of the rule (2e-6 of the
    output's range): 4x its error is a yardstick of FP32 size.  The focal references get 4x the floor: exp(-|s - g| / v) with
    arguments down to -140 (variance 0.05), then (1 - P)^-5, amplify the 2^-24 of P by more than a map loss's one rounding.  The
    steep pixels of focal_off_sample_case are 2e-3 off by construction (bounded here by 1e-2): 1 - P = 4.5e-5 in FP32."""
    for mode, (x, gt) in ((0, nll_case()), (1, smooth_l1_case())):
        l32, g32 = map_loss_reference(x, gt, mode, torch.float32)
        l64, g64 = map_loss_reference(x, gt, mode, torch.float64)
        assert _within(l32, l64) and _within(g32, g64), mode
        assert torch.isfinite(g32).all() and (mode == 0 or torch.equal(g64 != 0, g32 != 0))    # (sigmoid(-100) is 0 in FP32)
    mn, mx, gt = quantile_case()
    q32, q64 = quantile_reference(mn, mx, gt, torch.float32), quantile_reference(mn, mx, gt, torch.float64)
    for a, b in zip(q32, q64):
        assert _within(a, b)
    for start in (0, -3):
        for fc, variances in FOCAL_SETTINGS:
            cost, gt, var = focal_case(start, variances)
            for v in variances + (var,):
                r32 = focal_reference(cost, gt, v, start, fc, torch.float32)
                r64 = focal_reference(cost, gt, v, start, fc, torch.float64)
                for a, b in zip(r32, r64):
                    if a is not None:
                        assert torch.isfinite(a).all() and _within(a, b, 4.0), (start, fc, v if not torch.is_tensor(v) else "map")


def test_focal_off_sample_reference_is_finite():
    cost, gt, vmap = focal_off_sample_case()
    samples = torch.tensor(focal_geometry(0)[4])
    valid = (gt > 0) & (gt < FOCAL_D - 1)                                  # m1 and m2: the pixels that have a target
    assert ((gt[valid].view(-1, 1) - samples).abs().min(dim=1).values >= 0.25).all()      # ... and none of them on a sample
    assert set(gt.view(-1).tolist()) == set(FOCAL_OFF_SAMPLE)
    for v in (0.05, vmap):
        steep = ((gt == FOCAL_STEEP[0]) | (gt == FOCAL_STEEP[1])) & ((vmap == 0.05) if torch.is_tensor(v) else torch.ones_like(gt, dtype=torch.bool))
        assert int(steep.sum()) >= 40
        r32, r64 = focal_reference(cost, gt, v, 0, 5.0, torch.float32), focal_reference(cost, gt, v, 0, 5.0, torch.float64)
        assert abs(float(r32[0]) - float(r64[0])) <= 1e-2 * float(r64[0])
        for a, b in zip(r32[1:], r64[1:]):
            if a is None:
                continue
            assert torch.isfinite(a).all()
            m = steep.expand_as(b)
            assert (a[m].double() - b[m]).abs().max() <= 1e-2 * b[m].abs().max()
            # (64x the floor: under variance 0.05 the halfway pixels' grad_variance cancels to nothing in FP64, dt - E[dt] = 200 - 200,
            # and is 1e-5 of FP32 noise next to the 0.17 of the variance-1 pixels)
            assert (a[~m].double() - b[~m]).abs().max() <= 64 * V.FLOOR * b[~m].abs().max()


def test_smooth_l1_differences_are_exact():
    x, gt = smooth_l1_case()
    d = (x - gt).abs().view(-1)[3:11]
    assert d.tolist() == [float(np.float32(v)) for v in (0.0,) + around(1.0) for _ in range(2)]
    assert torch.equal((x.double() - gt.double())[..., :1, :16].float().double(), (x.double() - gt.double())[..., :1, :16])


def test_quantile_ties():
    mn, mx, gt = quantile_case()
    _, ga, gb = quantile_reference(mn, mx, gt, torch.float64)
    n = float(((gt > 0) & (gt < 192)).sum())
    tie = (gt == mn) & (gt > 0) & (gt < 192)
    assert int(tie.sum()) >= 8 and (ga[tie] + THETA / n).abs().max() <= 1e-18      # the indicator is 0 at 0: -theta / n, not -(theta - 1) / n
    tie = (gt == mx) & (gt > 0) & (gt < 192)
    assert int(tie.sum()) >= 8 and (gb[tie] + (1 - THETA) / n).abs().max() <= 1e-18
    assert (ga[(gt == 0) | (gt == 192)] == 0).all()


# ---------------------------------------------------------------------------------------------- section B
def test_distributions_are_deterministic_and_finite():
    for name in V.NAMES:
        a, b = V.channel(name, 2, 512, 5), V.channel(name, 2, 512, 5)
        assert torch.equal(a, b) and torch.isfinite(a).all() and a.dtype == torch.float32, name
        if name != "constant":
            assert not torch.equal(a, V.channel(name, 2, 512, 6)), name
    t, names = V.mixed((2, 4, 4096), 7, first=4)
    assert names == ["constant", "outlier30", "outlier100", "outlier1000"] and torch.equal(t, V.mixed((2, 4, 4096), 7, first=4)[0])
    assert (t[:, 0] == 3.0).all()
    rest = t[:, 3].reshape(-1)[1:]
    assert abs(float(t[0, 3, 0] - rest.mean())) > 900 * V.SIGMA            # the pivot element is the outlier
    for shape in V.SHAPES:                                                  # every shape sees every distribution; 1 MiB at most
        seen = set(n for case in V.CASES if case[0] == shape for n in V.channel_names(shape[1], first=case[1]))
        assert seen == set(V.NAMES), shape
        assert 4 * math.prod(shape) <= 1 << 20


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_batch_norm_references_stay_close_to_fp64(case):
    """ATen's FP32 statistics against FP64, per channel: within the floor, except where FP32 STORAGE of the quantity itself rounds
    coarser than that -- the quantity is then within one rounding of its own size (mean of an offset channel) or of the size of
    the terms that cancel in it (shift, y)."""
    k = V.bn_case(*case)
    r64, r32, std = V.bn_forward_reference(k["c"], k["gamma"], k["beta"], k["rm0"], k["rv0"])
    C = len(k["names"])
    u = 2.0 ** -24
    cancel = r64["mean"].abs() * r64["scale"].abs()                       # |mean * scale|: what shift and y subtract
    peak = V.per_channel_max(k["c"], C) * r64["scale"].abs()
    room = dict(mean=r64["mean"].abs(), invstd=r64["invstd"], scale=r64["scale"].abs(), shift=cancel, running_mean=r64["mean"].abs(),
                running_var=r64["running_var"], y=peak, y_stored=peak)
    for key, ref in r32.items():
        own = V.per_channel_max(ref.double() - r64["y" if key == "y_stored" else key], C)
        rng = V.per_channel_max(r64["y" if key == "y_stored" else key], C)
        bound = V.FLOOR * rng + 4 * u * room[key]
        assert (own <= bound).all(), (key, k["names"], own.tolist(), bound.tolist())


@pytest.mark.parametrize("offset,target", zip(V.EPILOGUE_OFFSETS, (0.0, 100.0, 1000.0)))
@pytest.mark.parametrize("shape", V.EPILOGUE_SHAPES)
def test_centre_tap_convolution_carries_the_mean(shape, offset, target):
    x, w = V.centre_tap_conv_inputs(shape, 32, offset, 131)
    assert torch.equal(x, V.centre_tap_conv_inputs(shape, 32, offset, 131)[0])
    raw = F.conv3d(x.double(), w.double(), padding=1)
    plain = F.conv3d(x.double()[:, :-1], w.double()[:, :-1], padding=1)
    assert (raw - plain - offset).abs().max() <= 1e-9 * max(offset, 1.0)      # exactly the offset on top, borders included
    ratio = raw.mean(dim=(0, 2, 3, 4)).abs() / raw.std(dim=(0, 2, 3, 4))
    if target == 0.0:
        assert float(ratio.max()) < 0.5
    else:
        assert float(ratio.min()) >= target / 2 and float(ratio.max()) <= target * 2


@pytest.mark.parametrize("case", V.CASES, ids=V.case_id)
def test_backward_and_dot_references_stay_close_to_fp64(case):
    """The yardsticks of test_bn_backward and test_channel_dot, per channel.  The stored-statistics backward (FP64 arithmetic on
    FP32 mean and invstd) is off by the rounding of the mean alone: xhat moves by at most b = |mean| * 2^-24 * invstd, dgamma by
    b * |dbeta|, dc by scale * (b * |dgamma| + max|xhat| * b * |dbeta|) / n; on top of that one rounding of invstd in each.  dbeta
    does not read the statistics: exact.  ATen's FP32 autograd is listed against the same room: it exceeds it where its own FP32
    sums add to the bias (a factor 8 covers every case), which is why it is not the yardstick there.  The FP32 torch sum behind
    channel_dot is within the floor of every channel's own value."""
    k = V.bn_case(*case)
    c, C = k["c"], len(k["names"])
    r64, r32, stored = V.bn_backward_reference(c, k["gamma"], k["beta"], k["dy"])
    f64, _, std = V.bn_forward_reference(c, k["gamma"], k["beta"], k["rm0"], k["rv0"])
    u, n = 2.0 ** -24, c.numel() // C
    b = f64["mean"].abs() * u * f64["invstd"]
    xmax = V.per_channel_max(c, C) * f64["invstd"] + f64["mean"].abs() * f64["invstd"]
    room = dict(dbeta=torch.zeros(C, dtype=torch.float64),
                dgamma=b * r64["dbeta"].abs() + 2 * u * r64["dgamma"].abs(),
                dc=f64["scale"].abs() * (b * r64["dgamma"].abs() + xmax * b * r64["dbeta"].abs()) / n + 4 * u * V.per_channel_max(r64["dc"], C))
    for key in ("dc", "dgamma", "dbeta"):
        rng = V.per_channel_max(r64[key], C)
        scale = rng if key == "dc" else rng.max().expand(C)
        own = V.per_channel_max(stored[key] - r64[key], C)
        assert (own <= 1e-12 * scale + room[key]).all(), (key, k["names"], own.tolist(), room[key].tolist())
        aten = V.per_channel_max(r32[key].double() - r64[key], C)
        assert (aten <= 8 * (V.FLOOR * scale + room[key])).all(), (key, k["names"], aten.tolist(), room[key].tolist())
    shape = case[0]
    g = V.mixed((shape[0], 1) + tuple(shape[2:]), 13, names=("plain",))[0]
    dims = [0] + list(range(2, c.dim()))
    d64, d32 = (c.double() * g.double()).sum(dim=dims), (c * g).sum(dim=dims)
    assert ((d32.double() - d64).abs() <= V.FLOOR * d64.abs()).all(), (k["names"], (d32.double() - d64).abs().tolist(), d64.tolist())
