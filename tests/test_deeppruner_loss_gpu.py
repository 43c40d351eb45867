"""The DeepPruner training losses (csrc/deeppruner_loss.hip, ``ops_deeppruner.deeppruner_loss_fwd`` / ``_bwd``, ``DeepPrunerLoss``
and the drop-in ``quantile_loss``) on the MI355X.  The cases are tests/_deeppruner_loss_ref.py's: the two recorded ones, 1 x 1 maps
under a 4 x 4 image with K = 3, a 12 x 20 image with maps of 5 x 9 and 3 x 5 (ratios 12 / 5 and 20 / 9) and one already at 12 x 20,
B = 2 on 24 x 72 (partial tiles), and K = 1.

Bounds.  Forward values: the kernel's per-pixel terms are the FP32 statements torch evaluates on the maps of
``deeppruner_final_maps``; only the final FP64-to-FP32 rounding and the division differ, so 2e-6 * max(1, |value|) holds them.
Against the recording: docs/design/15's contract, e_hip <= max(floor, 1.25 * e_ref) with e = max|. - fp64|, e_ref the recorded
reference's own distance, floor 2e-6 * max(1, |fp64|) for a loss and 2e-6 * max|g64| for a gradient tensor.  At the shapes that
are not recorded the fused gradients are held to the same rule against the composition of the library's existing kernels
(``map_loss_bwd``, ``bilinear_scale_bwd``, the chain rule for the taps), built here: e_fused <= max(floor, 1.25 * e_composition)."""
import pytest
import torch

from densematchingbenchmark_amd import ops, ops_deeppruner
from densematchingbenchmark_amd.config import Config
from tests import _deeppruner_loss_ref as R

pytestmark = pytest.mark.gpu
BOUNDS = (0.0, float(R.MAX_DISP), 0.0, float(R.MAX_DISP))
# docs/design/16's rule for a gradient row above 1.25 and above its floor: the measured ratio plus a quarter, never above 3
# (docs/design/19-deeppruner-loss.md has the measured ratios).  (case, index in the list maps + [min, max]) -> factor
FACTORS = {("4x", 1): 1.68}      # measured 1.43: e_hip 1.28e-7 against e_ref 8.95e-8, floor 2.5e-8


def _on(dev, name, grad=False):
    disps, lo, hi, gt = R.inputs(name)
    maps = [t.to(dev).requires_grad_(grad) for t in disps + [lo, hi]]
    return maps[:-2], maps[-2], maps[-1], gt.to(dev)


def _ieee_div(t, n):
    return torch.div(t, torch.full((), float(n), dtype=t.dtype, device=t.device))     # (tests/_deeppruner_model_ref.py)


def _smooth_l1(v, g):
    d = (v - g).abs()
    return torch.where(d < 1, 0.5 * d * d, d - 0.5)


_yardstick = {}


def _fp64_terms(name):
    """FP64 autograd of the restatement on the CPU, computed once per case: (K + 4 terms, gradients of R.total of them)."""
    if name not in _yardstick:
        disps, lo, hi, gt = R.inputs(name, torch.float64)
        leaves = [t.requires_grad_() for t in disps + [lo, hi]]
        terms = R.terms(leaves[:-2], leaves[-2], leaves[-1], gt, R.CASES[name][5])
        R.total(terms).backward()
        _yardstick[name] = ([t.detach() for t in terms], [t.grad for t in leaves])
    return _yardstick[name]


@pytest.mark.parametrize("name", list(R.CASES))
def test_forward_values(dev, name):
    theta = R.CASES[name][5]
    disps, lo, hi, gt = _on(dev, name)
    K, size = len(disps), tuple(gt.shape[-2:])
    out, stats = ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS, theta)
    maps = ops_deeppruner.deeppruner_final_maps(disps, lo, hi, size)[:K + 2]
    Mn, Mx = ops_deeppruner.deeppruner_final_maps([lo, hi], lo, hi, size)[:2]
    mask = (gt > 0) & (gt < R.MAX_DISP)
    n = int(mask.sum())
    assert n > 0 and stats.cpu().tolist() == [float(n), float(n)]
    th, th1 = torch.tensor(theta, dtype=torch.float32, device=dev), torch.tensor(1 - theta, dtype=torch.float32, device=dev)
    want = [_smooth_l1(m, gt)[mask].double().sum() / n for m in maps]
    for M, c in ((Mn, th), (Mx, th1)):
        x = gt - M
        want.append((x * (c - (x < 0).float()))[mask].double().sum() / n)
    f64 = _fp64_terms(name)[0]
    for i, (g, w) in enumerate(zip(out.cpu().tolist(), want)):
        w = w.item()
        print("%s term %d: hip %.9g  fp64 sum of fp32 terms %.9g  diff %.3g   (restatement in fp64: %.9g)" % (name, i, g, w, abs(g - w), f64[i]))
        assert abs(g - w) <= 2e-6 * max(1.0, abs(w)), (name, i, g, w)
        assert abs(g - f64[i].item()) <= 1e-4 * max(1.0, abs(w)), (name, i)        # (and it is the quantity the restatement names)


def _loss(name):
    from densematchingbenchmark_amd.modeling.stereo.losses import DeepPrunerLoss
    return DeepPrunerLoss(Config(R.settings(name)))


@pytest.mark.parametrize("name", R.RECORDED)
def test_against_the_recording(dev, name):
    z = R.recording()
    disps, lo, hi, gt = _on(dev, name, grad=True)
    gt.requires_grad_()
    d = _loss(name)(disps, lo, hi, gt)
    assert list(d) == [str(k) for k in z[name + "/keys"]] and all(v.dim() == 0 for v in d.values())
    R.total(d).backward()
    assert gt.grad is None                                                          # nothing reaches the ground truth
    for k, v, l32, l64 in zip(d, d.values(), z[name + "/loss32"], z[name + "/loss64"]):
        e_hip, e_ref, floor = abs(v.item() - l64), abs(float(l32) - l64), 2e-6 * max(1.0, abs(l64))
        print("%s %s: fp64 %.9g  e_hip %.3g  e_ref %.3g  floor %.3g" % (name, k, l64, e_hip, e_ref, floor))
        assert e_hip <= max(floor, 1.25 * e_ref), (name, k, e_hip, e_ref, floor)
    late = []
    for i, t in enumerate(disps + [lo, hi]):
        g32, g64 = torch.from_numpy(z["%s/grad32_%d" % (name, i)]), torch.from_numpy(z["%s/grad64_%d" % (name, i)])
        e_hip, e_ref = (t.grad.cpu().double() - g64).abs().max().item(), (g32.double() - g64).abs().max().item()
        floor, factor = 2e-6 * g64.abs().max().item(), FACTORS.get((name, i), 1.25)
        print("%s grad %d %s: max|g64| %.4g  e_hip %.3g  e_ref %.3g  floor %.3g  ratio %.3g  (factor %.2f)"
              % (name, i, tuple(g64.shape), g64.abs().max(), e_hip, e_ref, floor, e_hip / e_ref, factor))
        if t.grad.shape != g64.shape or not e_hip <= max(floor, factor * e_ref):
            late.append((name, i, e_hip, e_ref, floor, factor))
    assert not late, late


def _composition(disps, lo, hi, gt, coef, theta):
    """The backward the fused kernel replaces, from the library's existing kernels and elementwise torch on the device."""
    K, (H, W) = len(disps), gt.shape[-2:]
    mask = ((gt > 0) & (gt < R.MAX_DISP)).float()
    nq = mask.sum()

    def up_(d):
        return ops.bilinear_scale(_ieee_div(d * W, d.shape[-1]), (H, W), 1.0)

    def l1_grad(full, c):
        out = ops.map_loss_fwd(full, gt, 0.0, float(R.MAX_DISP), 1)
        return ops.map_loss_bwd(full, gt, out, torch.full((1,), c, dtype=torch.float32, device=gt.device), 0.0, float(R.MAX_DISP), 1)

    def down(g, d):       # the adjoint of the interpolation, then of (d * W) / w
        return ops.bilinear_scale_bwd(g, tuple(d.shape[-2:]), 1.0) * (W / d.shape[-1])

    grads = [down(l1_grad(up_(d), coef[k]), d) for k, d in enumerate(disps)]
    for j, (m, c) in enumerate(((lo, theta), (hi, 1 - theta))):
        M = up_(m)
        g = l1_grad(_ieee_div(M * W, W), coef[K + j])                                    # the second scaling differentiates to 1
        g = g - (coef[K + 2 + j] / nq) * mask * (torch.tensor(c, dtype=torch.float32, device=gt.device) - (gt - M < 0).float())
        grads.append(down(g, m))
    return grads


@pytest.mark.parametrize("name", list(R.CASES))
def test_gradients_against_fp64_and_the_composition(dev, name):
    theta = R.CASES[name][5]
    disps, lo, hi, gt = _on(dev, name)
    K = len(disps)
    coef = R.coefficients(K + 4)
    assert len(set(coef)) == K + 4
    out, stats = ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS, theta)
    go = torch.tensor(coef, dtype=torch.float32, device=dev)
    g_disps, g_lo, g_hi = ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, stats, go, *BOUNDS, theta)
    composed = _composition(disps, lo, hi, gt, coef, theta)
    late = []
    for i, (g, c, g64) in enumerate(zip(g_disps + [g_lo, g_hi], composed, _fp64_terms(name)[1])):
        e_fused, e_comp = (g.cpu().double() - g64).abs().max().item(), (c.cpu().double() - g64).abs().max().item()
        floor = 2e-6 * g64.abs().max().item()
        print("%s grad %d %s: max|g64| %.4g  e_fused %.3g  e_composition %.3g  floor %.3g" % (name, i, tuple(g64.shape), g64.abs().max(),
                                                                                             e_fused, e_comp, floor))
        assert g.shape == g64.shape and g64.abs().max() > 0
        if not e_fused <= max(floor, 1.25 * e_comp):
            late.append((name, i, e_fused, e_comp, floor))
    assert not late, late


@pytest.mark.parametrize("name", ["8x", "partial_tiles"])
def test_two_runs_are_equal(dev, name):
    theta = R.CASES[name][5]
    disps, lo, hi, gt = _on(dev, name)
    go = torch.tensor(R.coefficients(len(disps) + 4), dtype=torch.float32, device=dev)
    runs = []
    for _ in range(2):
        out, stats = ops_deeppruner.deeppruner_loss_fwd(disps, lo, hi, gt, *BOUNDS, theta)
        g_disps, g_lo, g_hi = ops_deeppruner.deeppruner_loss_bwd(disps, lo, hi, gt, stats, go, *BOUNDS, theta)
        runs.append([out, stats] + g_disps + [g_lo, g_hi])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_empty_masks(dev):
    """No valid pixel: 0 per smooth-L1 level, NaN for the quantile terms, zero gradients -- the reference's recorded behaviour."""
    z = R.recording()
    disps, lo, hi, gt = R.inputs("4x", empty=True)
    maps = [t.to(dev).requires_grad_() for t in disps + [lo, hi]]
    d = _loss("4x")(maps[:-2], maps[-2], maps[-1], gt.to(dev))
    got, rec = torch.stack(list(d.values())).cpu(), torch.from_numpy(z["4x/empty_loss32"])
    assert torch.equal(torch.isnan(got), torch.isnan(rec)) and torch.equal(got[1:], rec[1:]) and bool(torch.isnan(got[0]))
    R.total({k: v for k, v in d.items()}).backward()
    assert float(z["4x/empty_grad_max"].max()) == 0.0 and all(t.grad is not None and int(t.grad.ne(0).sum()) == 0 for t in maps)


@pytest.mark.parametrize("name", ["4x", "k1"])
def test_quantile_loss_drop_in(dev, name):
    """On full-size maps, against the reference's formula in FP64; the FP32 restatement on the CPU gives e_ref."""
    from densematchingbenchmark_amd.modeling.stereo.losses.utils import quantile_loss
    theta = R.CASES[name][5]
    _, lo, hi, gt = R.inputs(name)
    size = tuple(gt.shape[-2:])
    Mn, Mx = R.up(lo, size), R.up(hi, size)

    def cpu(dtype):
        a, b = Mn.to(dtype).clone().requires_grad_(), Mx.to(dtype).clone().requires_grad_()
        t = R.quantile_terms(a, b, gt.to(dtype), 0, R.MAX_DISP, theta)
        loss = (t[0] + t[1]) * 0.7
        loss.backward()
        return loss.detach(), a.grad, b.grad

    l64, a64, b64 = cpu(torch.float64)
    l32, a32, b32 = cpu(torch.float32)
    a, b, g = Mn.to(dev).requires_grad_(), Mx.to(dev).requires_grad_(), gt.to(dev).requires_grad_()
    loss = quantile_loss(a, b, g, R.MAX_DISP, weight=0.7, theta=theta)
    assert loss.dim() == 0
    loss.backward()
    assert g.grad is None
    e_hip, e_ref = abs(loss.item() - l64.item()), abs(l32.item() - l64.item())
    print("%s quantile_loss: fp64 %.9g  e_hip %.3g  e_ref %.3g" % (name, l64, e_hip, e_ref))
    assert e_hip <= max(2e-6 * max(1.0, abs(l64.item())), 1.25 * e_ref)
    for t, g32, g64 in ((a, a32, a64), (b, b32, b64)):
        e_hip, e_ref = (t.grad.cpu().double() - g64).abs().max().item(), (g32.double() - g64).abs().max().item()
        print("%s quantile_loss gradient: max|g64| %.4g  e_hip %.3g  e_ref %.3g" % (name, g64.abs().max(), e_hip, e_ref))
        assert e_hip <= max(2e-6 * g64.abs().max().item(), 1.25 * e_ref)


def test_forward_and_backward_capture_in_a_graph(dev):
    """What the reference's boolean indexing cannot have: one DeepPrunerLoss forward plus backward captured on one stream replays
    to the eager losses and gradients bit for bit, on inputs written after the capture."""
    loss = _loss("8x")
    disps, lo, hi, gt = _on(dev, "8x", grad=True)
    leaves = disps + [lo, hi]

    def step():
        d = loss(disps, lo, hi, gt)
        R.total(d).backward()
        return torch.stack(list(d.values()))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # the warm-up differentiates clones, so that the captured leaves are fresh to autograd
        warm = [t.detach().clone().requires_grad_() for t in leaves]
        R.total(loss(warm[:-2], warm[-2], warm[-1], gt)).backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    static_grads = [t.grad for t in leaves]
    other = R.inputs("8x")
    fresh = [t.flip(-1).contiguous() for t in other[0] + [other[1], other[2], other[3]]]      # other values, the same shapes
    with torch.no_grad():
        for t, f in zip(leaves + [gt], fresh):
            t.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    got = [captured.clone()] + [g.clone() for g in static_grads]
    for t in leaves:
        t.grad = None
    eager = [step()] + [t.grad for t in leaves]
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, eager)) and bool(torch.isfinite(got[0]).all())
