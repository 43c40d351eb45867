"""Inputs of the sampler's backward tests, shared by scripts/gen_golden_deeppruner_sampler_grads.py (the recording of the real
reference's autograd), tests/test_deeppruner_sampler_bwd_host.py and tests/test_deeppruner_sampler_bwd_gpu.py.

The cell rule: the gradient with respect to a sample jumps where a candidate's column coordinate
``ix = (x - s) * W / (W - 1) - 0.5`` crosses an integer, so every max-norm comparison runs on inputs whose FP64 ``ix`` keep a
margin from the integers: FP32 and FP64 then agree on every cell.  Everything here is CPU torch on tests/_deeppruner_ref.py."""
import torch

from tests import _deeppruner_ref as R

# name -> (B, C, H, W), P, max_disp: the whole chain, 3 iterations (the small cases of the recording)
CHAIN_CASES = {
    "h9w12": ((1, 8, 9, 12), 2, 6),
    "h6w10": ((1, 5, 6, 10), 3, 8),
    "h6w10_b2": ((2, 4, 6, 10), 3, 8),
    "h9w12_c7": ((1, 7, 9, 12), 2, 6),
}
CHAIN_MARGIN, CHAIN_SEEDS = 1e-4, range(20)

# name -> (B, 1, H, W), N, max_disp, seed: stage "post"
POST_CASES = {
    "n2": ((2, 1, 5, 13), 2, 24, 7101),
    "n3": ((1, 1, 7, 22), 3, 24, 7102),
    "n9": ((2, 1, 6, 17), 9, 48, 7103),
    "n10": ((1, 1, 9, 31), 10, 48, 7104),
}
POST_MARGIN = 1e-3


def candidate_ix(noise, lo, hi, vertical):
    """[B, 3P, H, W]: the column coordinate of every candidate of one half-iteration, in the dtype of the operands."""
    P, W = noise.shape[1], noise.shape[3]
    width, interval_min = R.intervals(lo, hi, P)
    samples = (hi - lo) * width * R.propagate(noise, vertical) + interval_min
    x = torch.arange(W, dtype=noise.dtype).view(1, 1, 1, W)
    return (x - samples) * W / (W - 1) - 0.5


def cell_margin(ix):
    return (ix - ix.round()).abs()


def unpropagate(flags, vertical):
    """[B, 3P, H, W] flags of candidates -> [B, P, H, W] flags of the noise entries they read, and the flags of the border
    candidates (noise 0, nothing to redraw)."""
    B, D, H, W = flags.shape
    f = flags.view(B, D // 3, 3, H, W)
    before, mid, after = f[:, :, 0], f[:, :, 1], f[:, :, 2]
    hit = mid.clone()
    border = torch.zeros_like(mid)
    if vertical:
        hit[:, :, :-1] |= before[:, :, 1:]
        hit[:, :, 1:] |= after[:, :, :-1]
        border[:, :, 0] |= before[:, :, 0]
        border[:, :, -1] |= after[:, :, -1]
    else:
        hit[..., :-1] |= before[..., 1:]
        hit[..., 1:] |= after[..., :-1]
        border[..., 0] |= before[..., 0]
        border[..., -1] |= after[..., -1]
    return hit, border


def step_inputs(shape, P, max_disp, vertical, maps, seed, margin=1e-3, rounds=200):
    """left, right, noise, lo, hi, gS, gN (FP32, CPU) of one half-iteration; no candidate's FP64 ``ix`` within ``margin`` of an
    integer.  ``maps``: the range is two maps that push x - s off the image on both sides, else the constants [0, max_disp] (as
    full maps, for the restatement).  Raises if the redrawing does not converge."""
    B, C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    left, right = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    noise = torch.rand((B, P, H, W), generator=g)
    gS, gN = torch.randn((B, P, H, W), generator=g), torch.randn((B, P, H, W), generator=g)

    def draw_maps():
        lo = torch.rand((B, 1, H, W), generator=g) * (1.4 * W) - 1.2 * W
        return lo, lo + torch.rand((B, 1, H, W), generator=g) * (2.1 * W) + 0.3 * W
    if maps:
        lo, hi = draw_maps()
    else:
        lo, hi = torch.zeros((B, 1, H, W)), torch.full((B, 1, H, W), float(max_disp))
    for _ in range(rounds):
        bad = cell_margin(candidate_ix(noise.double(), lo.double(), hi.double(), vertical)) < margin
        if not bad.any():
            return left, right, noise, lo, hi, gS, gN
        hit, border = unpropagate(bad, vertical)
        noise = torch.where(hit, torch.rand(noise.shape, generator=g), noise)
        if border.any():
            if not maps:
                raise AssertionError("a border candidate (noise 0) lies within %g of an integer: shape %s, P %d, max_disp %d"
                                     % (margin, shape, P, max_disp))
            nlo, nhi = draw_maps()
            sel = border.any(1, keepdim=True)
            lo, hi = torch.where(sel, nlo, lo), torch.where(sel, nhi, hi)
    raise AssertionError("the cell construction did not converge: shape %s, P %d, vertical %s, maps %s" % (shape, P, vertical, maps))


def chain_inputs(name, seed):
    """left, right, noise, g (the upstream gradient of the [B, P + 2, H, W] result) of a whole-chain case, FP32 on the CPU."""
    shape, P, _ = CHAIN_CASES[name]
    B, _, H, W = shape
    g = torch.Generator().manual_seed(1000 * seed + 17)
    left, right = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    noise = torch.rand((B, P, H, W), generator=g)
    return left, right, noise, torch.randn((B, P + 2, H, W), generator=g)


def chain_margin(name, seed, iterations=R.ITERATIONS):
    """The smallest distance of any candidate's FP64 ``ix`` to an integer over the ``2 * iterations`` half-iterations."""
    shape, P, max_disp = CHAIN_CASES[name]
    left, right, noise, _ = (t.double() for t in chain_inputs(name, seed))
    lo = torch.zeros((shape[0], 1) + shape[2:], dtype=torch.float64)
    hi = lo + max_disp
    worst = float("inf")
    with torch.no_grad():
        for _ in range(iterations):
            for vertical in (False, True):
                worst = min(worst, cell_margin(candidate_ix(noise, lo, hi, vertical)).min().item())
                _, noise = R.half_iteration(left, right, noise, lo, hi, vertical)
    return worst


_SEEDS = {}


def chain_seed(name):
    """The first of seeds 0 .. 19 whose FP64 evaluation keeps every candidate of all six steps CHAIN_MARGIN from an integer."""
    if name not in _SEEDS:
        ok = [s for s in CHAIN_SEEDS if chain_margin(name, s) >= CHAIN_MARGIN]
        if not ok:
            raise AssertionError("no seed of 0 .. 19 keeps every candidate of %s %g from an integer" % (name, CHAIN_MARGIN))
        _SEEDS[name] = ok[0]
    return _SEEDS[name]


def chain_grads(name, seed, dtype):
    """(out, d left, d right, d noise) of the restatement's autograd on the CPU in ``dtype``."""
    _, _, max_disp = CHAIN_CASES[name]
    left, right, noise, g = (t.to(dtype) for t in chain_inputs(name, seed))
    left, right, noise = (t.requires_grad_() for t in (left, right, noise))
    out = R.sampler('pre', left, right, noise=noise, max_disp=max_disp)
    return (out.detach(),) + torch.autograd.grad(out, (left, right, noise), g)


def post_decisions(lo, hi, N, max_disp):
    """The quantities whose sign or order switches a subgradient of the range head (FP64 in, [4 + 2, ...] out): min - max, the
    shortfall, and the two pre-clamp values against 0 and max_disp."""
    gmin, gmax = torch.min(lo, hi), torch.max(lo, hi)
    v = gmin + N - gmax
    over = v.clamp(min=0)
    a, c = (gmin - over) / 2.0, (gmax + over) / 2.0
    return torch.stack((lo - hi, v, a, a - max_disp, c, c - max_disp))


def post_inputs(name, rounds=200):
    """lo, hi [B, 1, H, W] and g [B, N, H, W] (FP32, CPU): min > max, ranges narrower than N (stretched) and both clamps active at
    some pixels, every decision quantity at least POST_MARGIN from its switch in FP64."""
    shape, N, max_disp, seed = POST_CASES[name]
    g = torch.Generator().manual_seed(seed)

    def draw():
        lo = torch.rand(shape, generator=g) * (max_disp * 3.0) - max_disp * 0.5      # halved by the head: both clamps are reached
        return lo, lo + (torch.rand(shape, generator=g) * 30.0 - 6.0)
    lo, hi = draw()
    grad = torch.randn((shape[0], N) + shape[2:], generator=g)
    for _ in range(rounds):
        bad = (post_decisions(lo.double(), hi.double(), N, max_disp).abs() < POST_MARGIN).any(0)
        if not bad.any():
            return lo, hi, grad
        nlo, nhi = draw()
        lo, hi = torch.where(bad, nlo, lo), torch.where(bad, nhi, hi)
    raise AssertionError("the stage-post construction did not converge: %s" % name)


def post_grads(lo, hi, g, N, max_disp, dtype, range_head=True):
    """(out, d lo, d hi) of the restatement's autograd on the CPU in ``dtype``."""
    lo, hi = (t.to(dtype).clone().requires_grad_() for t in (lo, hi))
    if range_head:
        out = R.sampler('post', None, None, lo, hi, max_disp=max_disp, uniform_sample_number=N)
    else:
        out = R.uniform_samples(lo, hi, N)
    return (out.detach(),) + torch.autograd.grad(out, (lo, hi), g.to(dtype))


def bound_check(tag, got, r64, r32, fails):
    """The project's rule (tests/test_unit_grads_gpu.py:_compare), per tensor: max |got - fp64| <= 4 * max |ref32 - fp64| +
    2e-6 * max |fp64|.  Appends a line to ``fails`` when it does not hold (NaN fails too); returns (error, bound)."""
    got, r64, r32 = got.detach().cpu().double(), r64.detach().double(), r32.detach().double()
    if got.shape != r64.shape:
        fails.append("%s: shape %s != %s" % (tag, tuple(got.shape), tuple(r64.shape)))
        return None
    scale = r64.abs().max().item()
    err, own = (got - r64).abs().max().item(), (r32 - r64).abs().max().item()
    bound = 4 * own + 2e-6 * scale
    if not err <= bound:
        fails.append("%s: error %.3e > bound %.3e (fp32 error %.3e, range %.3e)" % (tag, err, bound, own, scale))
    return err, bound
