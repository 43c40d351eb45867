"""The backward of DeepPruner's sampler on the MI355X (csrc/patch_match.hip: dmb_patch_match_step_bwd_f32,
dmb_deeppruner_uniform_samples_bwd_f32; train_fn.PatchMatchFn / UniformSamplesFn / deeppruner_sampler).

Yardsticks: autograd through the functional restatement (tests/_deeppruner_ref.py) on the CPU in FP64 and in FP32, and the real
reference's recorded gradients (tests/golden/deeppruner_sampler_grads.npz).  The bound is the project's
(tests/test_unit_grads_gpu.py:_compare, restated as ``bound_check`` in tests/_deeppruner_sampler_bwd_cases.py):

    max |hip - fp64| <= 4 * max |ref32 - fp64| + 2e-6 * max |fp64|      per tensor.

The cell rule: a gradient with respect to a sample jumps where a candidate's column coordinate crosses an integer, so every
max-norm test runs on inputs whose FP64 coordinates keep a margin from the integers (1e-3 for one half-iteration, 1e-4 over the
six steps of the chain); where cells cannot be controlled (config-like sizes) the contract is by share, see ``test_config_like``.
"""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import ops
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import fast_cat_fms
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler
from densematchingbenchmark_amd.modeling.stereo.layers import train_fn
from tests import _deeppruner_ref as R
from tests import _deeppruner_sampler_bwd_cases as K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_sampler_grads.npz")


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ----------------------------------------------------------------------------------------------------- one half-iteration
STEP_SHAPES = {"17x41_p12": ((17, 41), 12, 24), "9x12_p2": ((9, 12), 2, 6), "6x10_p3": ((6, 10), 3, 8), "2x2_p1": ((2, 2), 1, 3),
               "2x300_p5": ((2, 300), 5, 48), "9x23_p3": ((9, 23), 3, 11)}
STEP_CHANNELS = (8, 32, 33, 64)
STEP_MODES = ("gS", "gN", "both")


def _step_reference(left, right, noise, lo, hi, gS, gN, vertical, dtype):
    left, right, noise = (t.to(dtype).clone().requires_grad_() for t in (left, right, noise))
    s, n = R.half_iteration(left, right, noise, lo.to(dtype), hi.to(dtype), vertical)
    loss = 0
    if gS is not None:
        loss = loss + (s * gS.to(dtype)).sum()
    if gN is not None:
        loss = loss + (n * gN.to(dtype)).sum()
    return torch.autograd.grad(loss, (left, right, noise))


@pytest.mark.parametrize("maps", [False, True], ids=["consts", "maps"])
@pytest.mark.parametrize("shape", list(STEP_SHAPES))
def test_half_iteration(dev, shape, maps):
    """ops.patch_match_step_bwd against the restatement's autograd: every channel count, both batch sizes, both directions, the
    three combinations of upstream gradients; dL and d_noise_in bit-identical on a second run and for pair 0 alone."""
    (H, W), P, max_disp = STEP_SHAPES[shape]
    fails = []
    for ci, (C, B) in enumerate((C, B) for C in STEP_CHANNELS for B in (1, 2)):
        for vertical in (False, True):
            seed = 100 * ci + 10 * int(vertical) + int(maps) + 1
            left, right, noise, lo, hi, gS, gN = K.step_inputs((B, C, H, W), P, max_disp, vertical, maps, seed)
            d = [t.to(dev) for t in (left, right, noise, lo, hi, gS, gN)]
            kw = dict(vertical=vertical, temperature=R.TEMPERATURE, bounds=(0.0, float(max_disp)))
            rng = (d[3], d[4]) if maps else (None, None)
            for mode in STEP_MODES:
                s_cpu, n_cpu = (gS if mode != "gN" else None), (gN if mode != "gS" else None)
                s_dev, n_dev = (d[5] if mode != "gN" else None), (d[6] if mode != "gS" else None)
                got = ops.patch_match_step_bwd(d[0], d[1], d[2], *rng, grad_samples=s_dev, grad_noise=n_dev, **kw)
                r64 = _step_reference(left, right, noise, lo, hi, s_cpu, n_cpu, vertical, torch.float64)
                r32 = _step_reference(left, right, noise, lo, hi, s_cpu, n_cpu, vertical, torch.float32)
                tag = "%s C%d B%d %s %s" % (shape, C, B, "vertical" if vertical else "horizontal", mode)
                for name, g, a, b in zip(("dL", "dR", "d_noise"), got, r64, r32):
                    K.bound_check("%s %s" % (tag, name), g, a, b, fails)
                if mode != "both":
                    continue
                again = ops.patch_match_step_bwd(d[0], d[1], d[2], *rng, grad_samples=s_dev, grad_noise=n_dev, **kw)
                if not (_same_bits(got[0], again[0]) and _same_bits(got[2], again[2])):
                    fails.append("%s: dL / d_noise differ on a second run" % tag)
                if B == 2:
                    one = [t[:1].contiguous() for t in d]
                    alone = ops.patch_match_step_bwd(one[0], one[1], one[2], *((one[3], one[4]) if maps else (None, None)),
                                                     grad_samples=one[5], grad_noise=one[6], **kw)
                    if not (_same_bits(got[0][:1], alone[0]) and _same_bits(got[2][:1], alone[2])):
                        fails.append("%s: pair 0 alone differs from pair 0 in the batch (dL / d_noise)" % tag)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("maps", [False, True], ids=["consts", "maps"])
def test_half_iteration_at_the_width_limit(dev, maps):
    """W = 1024 = DMB_PATCH_MATCH_BWD_MAX_W: the launch is accepted with its 32 KiB of dynamic LDS and the row phase's four
    column passes of 256 scatter into the right columns.  With range maps both directions run; with the constant range only the
    horizontal one: in a vertical step every pixel of the first and last row has a border candidate (noise 0, s = max_disp / 2),
    and over 1024 columns (x - s) / 1023 passes 0.5 within 4.9e-4 of some column whatever max_disp is, so the cell rule's margin
    of 1e-3 cannot be had there."""
    shape, P, max_disp = (1, 8, 2, 1024), 1, 48
    fails = []
    for vertical in ((False, True) if maps else (False,)):
        left, right, noise, lo, hi, gS, gN = K.step_inputs(shape, P, max_disp, vertical, maps, 40 + int(vertical))
        d = [t.to(dev) for t in (left, right, noise, lo, hi, gS, gN)]
        got = ops.patch_match_step_bwd(d[0], d[1], d[2], *((d[3], d[4]) if maps else (None, None)), grad_samples=d[5],
                                       grad_noise=d[6], vertical=vertical, temperature=R.TEMPERATURE, bounds=(0.0, float(max_disp)))
        r64 = _step_reference(left, right, noise, lo, hi, gS, gN, vertical, torch.float64)
        r32 = _step_reference(left, right, noise, lo, hi, gS, gN, vertical, torch.float32)
        for name, g, a, b in zip(("dL", "dR", "d_noise"), got, r64, r32):
            K.bound_check("W 1024 %s %s" % ("vertical" if vertical else "horizontal", name), g, a, b, fails)
    assert not fails, "\n".join(fails)


def test_half_iteration_accumulates_and_reads_the_padded_gradient(dev):
    """``grad_left_acc`` / ``grad_right_acc`` are added (and left untouched); a [B, P + 2, H, W] ``grad_samples`` is read at
    channels 1 .. P."""
    (H, W), P, max_disp = STEP_SHAPES["9x23_p3"]
    left, right, noise, lo, hi, gS, gN = (t.to(dev) for t in K.step_inputs((2, 5, H, W), P, max_disp, False, False, 3))
    kw = dict(temperature=R.TEMPERATURE, bounds=(0.0, float(max_disp)))
    dl, dr, dn = ops.patch_match_step_bwd(left, right, noise, grad_samples=gS, grad_noise=gN, **kw)
    padded = torch.cat((torch.full_like(gS[:, :1], 1e30), gS, torch.full_like(gS[:, :1], -1e30)), 1)
    accl, accr = torch.randn_like(left), torch.randn_like(right)
    keep = accl.clone(), accr.clone()
    dl2, dr2, dn2 = ops.patch_match_step_bwd(left, right, noise, grad_samples=padded, grad_noise=gN, grad_left_acc=accl,
                                             grad_right_acc=accr, **kw)
    assert _same_bits(dn, dn2) and _same_bits(dl2, accl + dl)
    assert torch.equal(accl, keep[0]) and torch.equal(accr, keep[1])
    assert (dr2 - (accr + dr)).abs().max().item() <= 1e-5 * max(1.0, dr.abs().max().item())    # (LDS row sums: hardware order)


# ------------------------------------------------------------------------------------------------------------ whole chain
def _sampler(name):
    _, P, max_disp = K.CHAIN_CASES[name]
    return DeepPrunerSampler(max_disp=max_disp, iterations=R.ITERATIONS, temperature=R.TEMPERATURE,
                             patch_match_disparity_sample_number=P + 2).eval()


@pytest.mark.parametrize("name", list(K.CHAIN_CASES))
def test_chain(dev, name):
    """train_fn.deeppruner_sampler, stage "pre", 3 iterations: the three gradients against the restatement (FP64 / FP32) and
    against the reference's recording; the forward equals DeepPrunerSampler under no_grad bit for bit."""
    z = np.load(GOLDEN)
    seed = K.chain_seed(name)                  # (raises when no seed of 0 .. 19 qualifies)
    assert int(z[name + "/seed"]) == seed
    sampler = _sampler(name)
    left, right, noise, g = K.chain_inputs(name, seed)
    dl, dr, dn = (t.to(dev).requires_grad_() for t in (left, right, noise))
    out = train_fn.deeppruner_sampler(sampler, 'pre', dl, dr, noise=dn)
    with torch.no_grad():
        plain = sampler('pre', left.to(dev), right.to(dev), noise=noise.to(dev))
    assert _same_bits(out.detach(), plain)
    got = torch.autograd.grad(out, (dl, dr, dn), g.to(dev))
    r64, r32 = K.chain_grads(name, seed, torch.float64), K.chain_grads(name, seed, torch.float32)
    fails = []
    e32 = (r32[0].double() - r64[0]).abs().max().item()
    print("%s seed %d: fp32 restatement within %.3g of fp64 (largest element %.3g)" % (name, seed, e32, r64[0].abs().max()))
    K.bound_check(name + " out", out, r64[0], r32[0], fails)
    for what, t, a, b in zip(("d_left", "d_right", "d_noise"), got, r64[1:], r32[1:]):
        K.bound_check("%s %s" % (name, what), t, a, b, fails)
    # the recording (the real reference's FP32 autograd) in the place of ref32: its FP64 error is taken from the restatement
    for what, t, a in (("d_left", got[0], r64[1]), ("d_right", got[1], r64[2])):
        K.bound_check("%s %s with the recording's error" % (name, what), t, a, torch.from_numpy(z["%s/%s" % (name, what)]), fails)
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------ config-like sizes
@pytest.mark.parametrize("name", list(R.GOLDEN_CASES))
def test_config_like(dev, name):
    """Cells cannot be controlled at these sizes, so the contract is by share: with q the 99.9th percentile of |ref32 - fp64|
    of a gradient tensor, at most 0.2 % of |hip - fp64| may exceed 4 q + 2e-6 max|fp64|, and max|hip - fp64| <= 10 max|ref32 - fp64|.

    Measured on an MI355X (share beyond the bound; max|hip - fp64| / max|ref32 - fp64|), d_left / d_right / d_noise:
        a  2e-5, 1.20 / 2e-5, 1.47 / 6e-5, 1.60      b  0, 1.29 / 0, 1.06 / 0, 0.91      c  3.1e-4, 1.00 / 0, 1.00 / 9.6e-4, 1.00
    (docs/design/14, "Backward")."""
    (B, C, H, W), max_disp, _, seed = R.GOLDEN_CASES[name]
    left, right, noise, _, _ = R.golden_inputs(name)
    g = torch.randn((B, R.PATCH_MATCH_SAMPLES, H, W), generator=torch.Generator().manual_seed(seed + 50))
    sampler = DeepPrunerSampler(max_disp=max_disp).eval()
    dl, dr, dn = (t.to(dev).requires_grad_() for t in (left, right, noise))
    got = torch.autograd.grad(train_fn.deeppruner_sampler(sampler, 'pre', dl, dr, noise=dn), (dl, dr, dn), g.to(dev))

    def ref(dtype):
        a, b, n = (t.to(dtype).clone().requires_grad_() for t in (left, right, noise))
        return torch.autograd.grad(R.sampler('pre', a, b, noise=n, max_disp=max_disp), (a, b, n), g.to(dtype))
    r64, r32 = ref(torch.float64), ref(torch.float32)
    fails = []
    for what, t, a, b in zip(("d_left", "d_right", "d_noise"), got, r64, r32):
        e_hip, e_ref = (t.cpu().double() - a).abs().view(-1), (b.double() - a).abs().view(-1)
        q = torch.quantile(e_ref, 0.999).item()
        share = (e_hip > 4 * q + 2e-6 * a.abs().max().item()).double().mean().item()
        ratio = e_hip.max().item() / e_ref.max().item()
        print("%s %s: share beyond the bound %.5f, max ratio %.3f (q %.3g, ref max %.3g)" % (name, what, share, ratio, q, e_ref.max()))
        if not share <= 0.002:
            fails.append("%s %s: %.4f %% of the elements beyond 4 q" % (name, what, 100 * share))
        if not ratio <= 10.0:
            fails.append("%s %s: max error %.3e > 10 x the reference's %.3e" % (name, what, e_hip.max(), e_ref.max()))
    assert not fails, "\n".join(fails)


# ------------------------------------------------------------------------------------------------------------ stage "post"
@pytest.mark.parametrize("range_head", [True, False], ids=["head", "plain"])
@pytest.mark.parametrize("name", list(K.POST_CASES))
def test_post(dev, name, range_head):
    shape, N, max_disp, _ = K.POST_CASES[name]
    lo, hi, g = K.post_inputs(name)
    assert (lo > hi).any() and ((torch.min(lo, hi) + N - torch.max(lo, hi)) > 0).any()
    pre = K.post_decisions(lo.double(), hi.double(), N, max_disp)
    assert (pre[2] < 0).any() and (pre[5] > 0).any()                # both clamps active
    r64 = K.post_grads(lo, hi, g, N, max_disp, torch.float64, range_head)
    r32 = K.post_grads(lo, hi, g, N, max_disp, torch.float32, range_head)
    fails = []
    glo, ghi = ops.deeppruner_uniform_samples_bwd(lo.to(dev), hi.to(dev), g.to(dev), max_disp if range_head else None)
    K.bound_check(name + " d_min (op)", glo, r64[1], r32[1], fails)
    K.bound_check(name + " d_max (op)", ghi, r64[2], r32[2], fails)
    if range_head:      # through the Function, and against the reference's recording
        sampler = DeepPrunerSampler(max_disp=max_disp, uniform_disparity_sample_number=N).eval()
        a, b = lo.to(dev).requires_grad_(), hi.to(dev).requires_grad_()
        out = train_fn.deeppruner_sampler(sampler, 'post', None, None, a, b)
        with torch.no_grad():
            assert _same_bits(out.detach(), sampler('post', None, None, lo.to(dev), hi.to(dev)))
        fa, fb = torch.autograd.grad(out, (a, b), g.to(dev))
        assert _same_bits(fa, glo) and _same_bits(fb, ghi)
        z = np.load(GOLDEN)
        assert torch.equal(out.detach().cpu(), torch.from_numpy(z[name + "/post"]))
        for what, t, a64 in (("d_lo", fa, r64[1]), ("d_hi", fb, r64[2])):
            K.bound_check("%s %s with the recording's error" % (name, what), t, a64, torch.from_numpy(z["%s/%s" % (name, what)]), fails)
    assert not fails, "\n".join(fails)


def test_post_ties_and_clamp_edges_are_torchs(dev):
    """min == max, a shortfall of exactly 0 and pre-clamp values exactly on 0 and on max_disp, with integer upstream gradients and
    N - 1 a power of two: every product is exact, so the result must EQUAL torch's own subgradients."""
    max_disp = 48.0
    for N in (3, 9):
        lo = torch.tensor([5.0, 7.0, 20.0, 20.0 + N, 0.0, float(N), 96.0, 96.0 - N, -8.0, 3.0, 200.0, 11.5])
        hi = torch.tensor([5.0, 7.0, 20.0 + N, 20.0, float(N), 0.0, 96.0 - N, 96.0, 3.0, -8.0, 11.5, 200.0])
        lo, hi = lo.view(1, 1, 2, 6), hi.view(1, 1, 2, 6)
        g = torch.randint(-8, 9, (1, N, 2, 6), generator=torch.Generator().manual_seed(N)).float() * 4.0
        for range_head in (True, False):
            want = K.post_grads(lo, hi, g, N, max_disp, torch.float32, range_head)
            got = ops.deeppruner_uniform_samples_bwd(lo.to(dev), hi.to(dev), g.to(dev), max_disp if range_head else None)
            assert torch.equal(got[0].cpu(), want[1]) and torch.equal(got[1].cpu(), want[2]), (N, range_head, got, want)


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_no_gradient_where_none_is_required(dev):
    name = "h6w10"
    sampler = _sampler(name)
    left, right, noise, g = (t.to(dev) for t in K.chain_inputs(name, 1))
    a = left.clone().requires_grad_()
    out = train_fn.deeppruner_sampler(sampler, 'pre', a, right, noise=noise)
    out.backward(g)
    assert a.grad is not None and right.grad is None and noise.grad is None
    full = torch.autograd.grad(train_fn.deeppruner_sampler(sampler, 'pre', a, right.clone().requires_grad_(), noise=noise), a, g)[0]
    assert _same_bits(full, a.grad)
    lo, hi, gp = (t.to(dev) for t in K.post_inputs("n9"))
    b = hi.clone().requires_grad_()
    s9 = DeepPrunerSampler(max_disp=48).eval()
    train_fn.deeppruner_sampler(s9, 'post', left, right, lo, b).backward(gp)
    assert b.grad is not None and lo.grad is None
    with torch.no_grad():
        assert not train_fn.deeppruner_sampler(sampler, 'pre', a, right, noise=noise).requires_grad
    with pytest.raises(NotImplementedError, match="backward"):
        sampler('pre', a, right, noise=noise)                      # the module's own forward keeps refusing


def test_double_backward_is_refused(dev):
    """``create_graph=True`` with a plain upstream gradient (a gradient penalty): both stages refuse in the backward instead of
    returning a first gradient without a graph, whose second-order term would be dropped silently."""
    name = "h6w10"
    sampler = _sampler(name)
    left, right, noise, g = (t.to(dev) for t in K.chain_inputs(name, 1))
    a = left.clone().requires_grad_()
    out = train_fn.deeppruner_sampler(sampler, 'pre', a, right, noise=noise)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(out, a, g, create_graph=True)
    first = torch.autograd.grad(out, a, g)[0]                       # the same graph still gives its first gradient
    assert torch.isfinite(first).all() and not first.requires_grad
    lo, hi, gp = (t.to(dev) for t in K.post_inputs("n9"))
    b = lo.clone().requires_grad_()
    out = train_fn.deeppruner_sampler(DeepPrunerSampler(max_disp=48).eval(), 'post', left, right, b, hi)
    with pytest.raises(NotImplementedError, match="double backward"):
        torch.autograd.grad(out, b, gp, create_graph=True)


def test_samples_hand_over_to_the_volume(dev):
    """The samples feed fast_cat_fms(..., disp_sample=samples) under autograd: ``left`` and ``right`` receive a gradient through
    the volume AND through the sampler."""
    name = "h9w12"
    shape, P, max_disp = K.CHAIN_CASES[name]
    sampler = _sampler(name)
    seed = K.chain_seed(name)
    left, right, noise, _ = K.chain_inputs(name, seed)
    gvol = torch.randn((shape[0], 2 * shape[1], P + 2) + shape[2:], generator=torch.Generator().manual_seed(5))

    def hip():
        a, b = left.to(dev).requires_grad_(), right.to(dev).requires_grad_()
        samples = train_fn.deeppruner_sampler(sampler, 'pre', a, b, noise=noise.to(dev))
        assert samples.requires_grad
        vol = fast_cat_fms(a, b, disp_sample=samples)
        direct = torch.autograd.grad(fast_cat_fms(a, b, disp_sample=samples.detach()), (a, b), gvol.to(dev))
        return torch.autograd.grad(vol, (a, b), gvol.to(dev)), direct

    def ref(dtype):
        a, b = left.to(dtype).requires_grad_(), right.to(dtype).requires_grad_()
        samples = R.sampler('pre', a, b, noise=noise.to(dtype), max_disp=max_disp)
        warped = R.inverse_warp_3d(b, -samples)
        B, C, D, H, W = warped.shape
        vol = torch.cat((a.unsqueeze(2).expand(B, C, D, H, W) * (warped > 0).to(dtype), warped), 1)
        return torch.autograd.grad(vol, (a, b), gvol.to(dtype))
    (got, direct), r64, r32 = hip(), ref(torch.float64), ref(torch.float32)
    fails = []
    for what, t, d, a, b in zip(("d_left", "d_right"), got, direct, r64, r32):
        K.bound_check(what, t, a, b, fails)
        assert (t - d).abs().max().item() > 1e-3 * a.abs().max().item(), "%s: nothing arrived through the sampler" % what
    assert not fails, "\n".join(fails)


def test_graph_capture(dev):
    """Forward plus backward captured in a graph and replayed on fresh inputs: outputs, dL and d_noise equal eager bit for bit,
    dR within the bound."""
    name = "h6w10_b2"
    sampler = _sampler(name)
    seed = K.chain_seed(name)
    first = [t.to(dev) for t in K.chain_inputs(name, 7)]
    static = [t.clone() for t in first]
    leaves = [t.requires_grad_() for t in static[:3]]

    def run():
        out = train_fn.deeppruner_sampler(sampler, 'pre', *leaves[:2], noise=leaves[2])
        return (out,) + torch.autograd.grad(out, leaves, static[3])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                   # warm-up outside the capture (the library loads, the allocator fills)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = run()
    fresh = [t.to(dev) for t in K.chain_inputs(name, seed)]
    with torch.no_grad():
        for s, f in zip(static, fresh):
            s.copy_(f)
    graph.replay()
    torch.cuda.synchronize()
    eager_leaves = [t.clone().requires_grad_() for t in fresh[:3]]
    out = train_fn.deeppruner_sampler(sampler, 'pre', *eager_leaves[:2], noise=eager_leaves[2])
    eager = (out,) + torch.autograd.grad(out, eager_leaves, fresh[3])
    assert _same_bits(res[0].detach(), eager[0].detach()) and _same_bits(res[1], eager[1]) and _same_bits(res[3], eager[3])
    r64, r32 = K.chain_grads(name, seed, torch.float64), K.chain_grads(name, seed, torch.float32)
    fails = []
    K.bound_check("replayed d_right", res[2], r64[2], r32[2], fails)
    assert not fails, fails


def test_peak_memory_stays_below_one_expanded_tensor(dev):
    """[1, 32, 136, 240], P = 12: forward plus backward raise the peak allocated memory by less than ONE expanded
    [B, C, 3P, H, W] tensor (150 MB); stock autograd holds dozens of them."""
    B, C, H, W, P = 1, 32, 136, 240, 12
    g = torch.Generator().manual_seed(9)
    left, right = (torch.randn((B, C, H, W), generator=g).to(dev).requires_grad_() for _ in range(2))
    noise = torch.rand((B, P, H, W), generator=g).to(dev)
    up = torch.randn((B, P + 2, H, W), generator=g).to(dev)
    sampler = DeepPrunerSampler(max_disp=48).eval()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = train_fn.deeppruner_sampler(sampler, 'pre', left, right, noise=noise)
    grads = torch.autograd.grad(out, (left, right), up)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print("peak rise %.1f MB" % (rise / 2 ** 20))
    assert all(torch.isfinite(t).all() for t in grads)
    assert rise < B * C * 3 * P * H * W * 4
