"""Values that sit ON a decision of a kernel: errors of exactly 1, 2, 3 and 5 pixels, ground truth on a mask bound, a difference of
exactly 0, a pre-activation of exactly 0, logits whose exponential leaves FP32.  A continuous random draw -- what the rest of the
suite feeds -- lands on none of them, so a ``>`` turned ``>=`` passes everywhere else.

The inputs are hand-placed on tiny maps and exactly representable (tests/_value_edges.py builds them, tests/test_value_edges_host.py checks them); the
reference evaluates the same inputs on the CPU.  Counts, masks and zero patterns are compared exactly, values against FP64 within
4x the FP32 reference's own error plus 2e-6 of the range (tests/_values.py::close).  No element is left out."""
import pytest
import torch

from oracle import dmb_oracle as O
from tests import _value_edges as K
from tests._values import close as _close

pytestmark = pytest.mark.gpu


def _ops():
    from densematchingbenchmark_amd import ops

    return ops


# ---------------------------------------------------------------------------------------------- 1. end-point error
def _check_acc(acc, est, gt, what):
    exp = K.epe_expected(est, gt)
    got = acc.cpu().tolist()
    print(what, got, exp)
    assert got[0] == exp[0] == 2
    assert got[2:] == exp[2:], what                  # integers over counts, the same FP64 operations: exactly
    assert abs(got[1] - exp[1]) <= 1e-12 * exp[1], what
    ref, n = O.dataset_metrics([est], [gt], K.EPE_ORIGINAL, *K.EPE_BOUNDS)
    for i, k in enumerate(("epe", "1px", "2px", "3px", "5px")):      # and the reference's FP32 figures to FP32 rounding
        assert abs(got[1 + i] - ref[k] * n) <= 4 * 2.0 ** -24 * n * max(1.0, abs(got[1 + i])), (what, k)


def test_epe_on_the_thresholds(dev):
    """epe_accumulate and epe_accumulate_multi, cropped (8 x 64 maps, original size 6 x 60): |gt - est| exactly 1, 2, 3, 5 and their
    FP32 neighbours, gt exactly on lb and ub, an image whose only in-range pixels sit on thresholds."""
    ops = _ops()
    ests, gt = K.epe_case()
    gd, ed = gt.to(dev), [e.to(dev) for e in ests]
    multi = torch.zeros((3, 6), dtype=torch.float64, device=dev)
    ops.epe_accumulate_multi(ed, gd, multi, K.EPE_ORIGINAL, *K.EPE_BOUNDS)
    for i, e in enumerate(ests):
        single = torch.zeros(6, dtype=torch.float64, device=dev)
        ops.epe_accumulate(ed[i], gd, single, K.EPE_ORIGINAL, *K.EPE_BOUNDS)
        _check_acc(single, e, gt, "estimate %d" % i)
        assert torch.equal(single, multi[i])


# ---------------------------------------------------------------------------------------------- 2., 3. the map losses
@pytest.mark.parametrize("mode", [1, 0])
def test_map_loss_edges(dev, mode):
    """mode 1 (smooth L1): |x - gt| at 0, at 1 and its neighbours, gt on lower and upper; the gradient's zero pattern is the
    reference's.  mode 0 (-logsigmoid): logits 0, +/-20, +/-88, +/-89, +/-100; the gradient is finite everywhere."""
    ops = _ops()
    x, gt = K.smooth_l1_case() if mode == 1 else K.nll_case()
    lower, upper = K.MAP_BOUNDS
    l32, g32 = K.map_loss_reference(x, gt, mode, torch.float32)
    l64, g64 = K.map_loss_reference(x, gt, mode, torch.float64)
    xd, gd = x.to(dev), gt.to(dev)
    out = ops.map_loss_fwd(xd, gd, lower, upper, mode)
    grad = ops.map_loss_bwd(xd, gd, out, torch.ones((1,), device=dev), lower, upper, mode).cpu()
    mask = (gt > lower) & (gt < upper)
    assert out[1].item() == float(mask.sum())
    _close(out[:1].cpu(), l64.view(1), l32.view(1), "loss")
    assert torch.isfinite(grad).all()
    _close(grad, g64, g32, "gradient")
    assert (grad[~mask] == 0).all()
    if mode == 1:
        assert torch.equal(grad != 0, g64 != 0)       # the mask, less the pixels whose difference is exactly 0
    else:
        n = float(mask.sum())                         # no valid logit below 88 has a zero gradient (1 / (1 + e^88) is an FP32 normal / n)
        assert (grad[mask & (x < 80)] != 0).all() and (grad.abs() <= (1.0 + 2.0 ** -22) / n).all()


# ---------------------------------------------------------------------------------------------- 4. the focal loss
@pytest.mark.parametrize("start", [0, -3])
@pytest.mark.parametrize("fc,variances", K.FOCAL_SETTINGS)
def test_focal_loss_edges(dev, start, fc, variances):
    """stereo_focal_loss_fwd / bwd, D = 8: gt on lower (= start_disp), upper and end_disp -- the m1 / m2 pairs of Target::setup --, on
    a sample, halfway between two; each variance as a scalar, then all of them in one map (with its gradient)."""
    ops = _ops()
    lower, upper, s0, s1, samples = K.focal_geometry(start)
    cost, gt, vmap = K.focal_case(start, variances)
    m1 = (gt > lower) & (gt < upper)
    cd, gd = cost.to(dev), gt.to(dev)
    for v in variances + (vmap,):
        is_map = torch.is_tensor(v)
        what = "start %d, coefficient %g, variance %s" % (start, fc, "map" if is_map else v)
        l32, gc32, gv32 = K.focal_reference(cost, gt, v, start, fc, torch.float32)
        l64, gc64, gv64 = K.focal_reference(cost, gt, v, start, fc, torch.float64)
        vd = v.to(dev) if is_map else v
        out, stats = ops.stereo_focal_loss_fwd(cd, gd, vd, samples, lower, upper, s0, s1, fc)
        gcost, gvar = ops.stereo_focal_loss_bwd(cd, gd, vd, samples, stats, out, torch.ones((1,), device=dev), lower, upper, s0, s1,
                                                fc, is_map)
        assert out[1].item() == float(m1.sum()), what
        _close(out[:1].cpu(), l64.view(1), l32.view(1), what + ": loss")
        gcost = gcost.cpu()
        _close(gcost, gc64, gc32, what + ": grad_cost")
        assert (gcost[(~m1).expand_as(gcost)] == 0).all(), what          # rows outside (lower, upper): exactly nothing
        if is_map:
            gvar = gvar.cpu()
            _close(gvar, gv64, gv32, what + ": grad_variance")
            assert (gvar[~m1] == 0).all(), what


def _close_per_class(got, ref64, ref32, steep, what):
    """The rule over the steep pixels and over the others ([B, 1, H, W] mask; outputs [B, D or 1, H, W]): 20 orders apart in range."""
    for name, m in (("steep", steep), ("others", ~steep)):
        m = m.expand_as(ref64)
        print(what, name, (got[m].double() - ref64[m]).abs().max().item(), (ref32[m].double() - ref64[m]).abs().max().item(),
              ref64[m].abs().max().item())
        _close(got[m], ref64[m], ref32[m], "%s, %s pixels" % (what, name))


def test_focal_loss_steepest_weight(dev):
    """Coefficient 5 with variance 0.05 -- scalar, then in a map next to 1 and 50 -- on ground truth that never sits on a sample
    (_value_edges.focal_off_sample_case): every pixel compared, the steep ones among themselves."""
    ops = _ops()
    lower, upper, s0, s1, samples = K.focal_geometry(0)
    cost, gt, vmap = K.focal_off_sample_case()
    m1 = (gt > lower) & (gt < upper)
    cd, gd = cost.to(dev), gt.to(dev)
    for v in (0.05, vmap):
        is_map = torch.is_tensor(v)
        what = "variance %s" % ("map" if is_map else v)
        steep = ((gt == K.FOCAL_STEEP[0]) | (gt == K.FOCAL_STEEP[1])) & ((vmap == 0.05) if is_map else torch.ones_like(gt, dtype=torch.bool))
        l32, gc32, gv32 = K.focal_reference(cost, gt, v, 0, 5.0, torch.float32)
        l64, gc64, gv64 = K.focal_reference(cost, gt, v, 0, 5.0, torch.float64)
        vd = v.to(dev) if is_map else v
        out, stats = ops.stereo_focal_loss_fwd(cd, gd, vd, samples, lower, upper, s0, s1, 5.0)
        gcost, gvar = ops.stereo_focal_loss_bwd(cd, gd, vd, samples, stats, out, torch.ones((1,), device=dev), lower, upper, s0, s1, 5.0,
                                                is_map)
        assert out[1].item() == float(m1.sum()), what
        print(what, "loss", out[0].item(), l64.item(), l32.item())
        _close(out[:1].cpu(), l64.view(1), l32.view(1), what + ": loss")
        gcost = gcost.cpu()
        assert torch.isfinite(gcost).all(), what
        _close_per_class(gcost, gc64, gc32, steep, what + ": grad_cost")
        assert (gcost[(~m1).expand_as(gcost)] == 0).all(), what
        if is_map:
            gvar = gvar.cpu()
            assert torch.isfinite(gvar).all()
            _close_per_class(gvar, gv64, gv32, steep, what + ": grad_variance")
            assert (gvar[~m1] == 0).all(), what


@pytest.mark.parametrize("start", [0, -3])
@pytest.mark.parametrize("fc,variances", K.FOCAL_SETTINGS)
def test_focal_loss_without_a_valid_pixel(dev, start, fc, variances):
    """Loss 0 over a divisor of 1, every gradient exactly zero.  (A masked pixel still has a target: gt * m1 = 0, which IS a sample
    when start_disp < 0 -- with variance 0.05 and a coefficient of 5 the reference's FP32 weight is infinite there and its loss
    NaN, the combination K.FOCAL_SETTINGS leaves out.)"""
    ops = _ops()
    lower, upper, s0, s1, samples = K.focal_geometry(start)
    cost, gt, vmap = K.focal_case(start, variances)
    gt = torch.where((gt > lower) & (gt < upper), torch.full_like(gt, upper), gt)       # on and beyond the bounds only
    cd, gd, vd = cost.to(dev), gt.to(dev), vmap.to(dev)
    out, stats = ops.stereo_focal_loss_fwd(cd, gd, vd, samples, lower, upper, s0, s1, fc)
    gcost, gvar = ops.stereo_focal_loss_bwd(cd, gd, vd, samples, stats, out, torch.ones((1,), device=dev), lower, upper, s0, s1, fc, True)
    assert out[0].item() == 0.0 and out[1].item() == 1.0
    assert (gcost == 0).all() and (gvar == 0).all()
    assert float(O.stereo_focal_loss(cost, gt, vmap, K.FOCAL_D, start, 1, fc)) == 0.0          # the reference, in FP32


# ---------------------------------------------------------------------------------------------- 5. the quantile loss
def test_quantile_loss_ties(dev):
    """gt - min == 0 and gt - max == 0: the reference's indicator [gt - M < 0] is 0 there, the gradient -theta / n and
    -(1 - theta) / n; gt on q_lo and q_hi is masked."""
    from densematchingbenchmark_amd import ops_deeppruner as opsd
    mn, mx, gt = K.quantile_case()
    lo, hi = K.QUANTILE_BOUNDS
    t32, ga32, gb32 = K.quantile_reference(mn, mx, gt, torch.float32)
    t64, ga64, gb64 = K.quantile_reference(mn, mx, gt, torch.float64)
    md, xd, gd = mn.to(dev), mx.to(dev), gt.to(dev)
    out, stats = opsd.quantile_loss_fwd(md, xd, gd, lo, hi, K.THETA)
    ga, gb = opsd.quantile_loss_bwd(md, xd, gd, stats, torch.ones((2,), device=dev), lo, hi, K.THETA)
    mask = (gt > lo) & (gt < hi)
    assert stats[1].item() == float(mask.sum())
    _close(out.cpu(), t64, t32, "terms")
    ga, gb = ga.cpu(), gb.cpu()
    _close(ga, ga64, ga32, "grad_min")
    _close(gb, gb64, gb32, "grad_max")
    assert torch.equal(ga != 0, mask) and torch.equal(gb != 0, mask)
    # every valid gradient is one of two values a factor 19 apart: the side it took is the reference's, ties included
    assert torch.equal(ga < -0.5 / float(mask.sum()), ga64 < -0.5 / float(mask.sum()))
    assert torch.equal(gb < -0.5 / float(mask.sum()), gb64 < -0.5 / float(mask.sum()))
    tie = mask & (gt == mn)
    assert int(tie.sum()) >= 8 and torch.equal(ga[tie], ga32[tie])


# ---------------------------------------------------------------------------------------------- 6. ReLU ties of the BN unit
@pytest.mark.parametrize("relu", [0, 1, 2])
@pytest.mark.parametrize("shape", K.TIE_SHAPES)
def test_bn_act_relu_ties(dev, shape, relu):
    """bn_act + bn_act_bwd in eval mode with scale 1, shift 0, mean 0, invstd 1 on small integers whose ReLU argument is exactly 0
    on a third of the elements: y, dc and dres equal autograd of O.bn_act_train bit for bit, every element (test_bn_act_train
    compares away from the ties)."""
    ops = _ops()
    c, res, dy = K.tie_case(shape, relu)
    C = shape[1]
    ref = K.tie_reference(c, res, dy, relu)
    ref64 = K.tie_reference(c, res, dy, relu, torch.float64)
    one, zero = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    mode = {0: False, 1: True, 2: "pre"}[relu]
    cd, rd, dyd = c.to(dev), res.to(dev), dy.to(dev)
    y = ops.bn_act(cd, one, zero, rd, relu=mode)
    assert torch.equal(y.cpu(), ref["y"])
    dc, dgamma, dbeta, dres = ops.bn_act_bwd(dyd, cd, y, one, zero, zero, one, relu=mode, training=False, want_dres=True)
    assert torch.equal(dc.cpu(), ref["dc"])
    assert torch.equal(dres.cpu(), ref["dres"])
    _close(dgamma.cpu(), ref64["dgamma"], ref["dgamma"], "dgamma")
    _close(dbeta.cpu(), ref64["dbeta"], ref["dbeta"], "dbeta")


# ---------------------------------------------------------------------------------------------- 7. the soft-argmin family
@pytest.mark.parametrize("alpha", [1.0, -1.0])
@pytest.mark.parametrize("D", [1, 5, 192])
def test_soft_argmin_saturated_columns(dev, D, alpha):
    """soft_argmin, soft_argmin_sampled, trilinear_soft_argmin and soft_argmin_bwd on columns whose largest logit (cost * alpha)
    exceeds the rest by 1e2, 1e3 and 1e4 -- one-hot: that sample within 1e-6 --, with two equal maxima at 1e4 (the midpoint), and
    all-equal at +/-1e4 (the mean of the samples); the rest of the suite stops at a gain of 12."""
    ops = _ops()
    logits, kinds, peaks = K.soft_argmin_case(D)
    cost = logits * alpha                                            # alpha = +/-1: exact, cost * alpha gives the logits back
    B, H, W = K.SOFT_SHAPE
    vals = O.disp_sample_values(D)
    vlist = vals.tolist()
    ref64 = O.soft_argmin_f64(cost, D, alpha=alpha)
    ref32 = O.soft_argmin(cost, D, alpha=alpha)
    cd = cost.to(dev)
    forms = dict(soft_argmin=ops.soft_argmin(cd, vlist, alpha, True),
                 sampled=ops.soft_argmin_sampled(cd, vals.view(1, D, 1, 1).expand(B, D, H, W).contiguous().to(dev), alpha, True),
                 trilinear=ops.trilinear_soft_argmin(cd, (D, H, W), vlist, alpha))
    one_hot = (kinds < 3).unsqueeze(1)
    for name, disp in forms.items():
        got = disp.cpu()
        assert torch.isfinite(got).all(), name
        print(name, (got.double() - ref64).abs().max().item(), (ref32.double() - ref64).abs().max().item())
        assert (got.double() - ref64)[one_hot].abs().max().item() <= 1e-6, name
        _close(got, ref64, ref32, name)
    g = torch.randn((B, 1, H, W), generator=torch.Generator().manual_seed(47))
    grads = {}
    for dtype in (torch.float32, torch.float64):
        c = cost.to(dtype).requires_grad_(True)
        d = (torch.softmax(c * alpha, dim=1) * vals.to(dtype).view(1, D, 1, 1)).sum(1, keepdim=True)
        grads[dtype], = torch.autograd.grad(d, c, g.to(dtype))
    got = ops.soft_argmin_bwd(cd, forms["soft_argmin"], g.to(dev), vlist, alpha).cpu()
    assert torch.isfinite(got).all()
    _close(got, grads[torch.float64], grads[torch.float32], "soft_argmin_bwd")
