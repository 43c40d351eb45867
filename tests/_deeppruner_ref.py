"""Functional restatement of the reference's DeepPruner disparity sampler (disp_samplers/DeepPruner.py and
disp_samplers/utils/patch_match.py) on stock torch: shifts for the propagation (the reference convolves with one-hot filters),
``F.grid_sample`` for the warp (layers/inverse_warp_3d.py).  Any dtype, any device -- the reference itself is pinned to FP32 by
its one-hot filter and ``linspace`` grids, so this is also the FP64 yardstick, and what the GPU tests compare against.

In FP32 on the CPU it performs the reference's tensor operations in the reference's order: tests/test_deeppruner_sampler_host.py
pins it bit for bit against the real reference's recorded outputs (tests/golden/deeppruner_sampler.npz)."""
import torch
import torch.nn.functional as F

# name -> (B, C, H, W), max_disp, input scale, seed; recorded by scripts/gen_golden_deeppruner_sampler.py
GOLDEN_CASES = {
    "a": ((2, 32, 32, 64), 48, 1.0, 4101),
    "b": ((2, 32, 32, 64), 48, 0.3, 4102),
    "c": ((1, 32, 17, 41), 24, 1.0, 4103),
}
PATCH_MATCH_SAMPLES, UNIFORM_SAMPLES, ITERATIONS, TEMPERATURE = 14, 9, 3, 7


def golden_inputs(name, dtype=torch.float32):
    """left, right [B, C, H, W], the PatchMatch noise [B, 12, H, W] in [0, 1) and the "post" stage's range maps [B, 1, H, W]:
    some with min > max, some narrower than the sample count, some beyond [0, max_disp] on either side."""
    (B, C, H, W), max_disp, scale, seed = GOLDEN_CASES[name]
    g = torch.Generator().manual_seed(seed)
    left = torch.randn((B, C, H, W), generator=g) * scale
    right = torch.randn((B, C, H, W), generator=g) * scale
    noise = torch.rand((B, PATCH_MATCH_SAMPLES - 2, H, W), generator=g)
    lo = torch.rand((B, 1, H, W), generator=g) * (max_disp * 1.5) - max_disp * 0.25
    hi = lo + (torch.rand((B, 1, H, W), generator=g) * 30.0 - 6.0)
    return tuple(t.to(dtype) for t in (left, right, noise, lo, hi))


def propagate(noise, vertical):
    """patch_match.py:119-174: [B, P, H, W] -> [B, 3P, H, W], channel 3p + j = interval p at offset j - 1 along x (y), 0 outside."""
    B, P, H, W = noise.shape
    if vertical:
        before, after = F.pad(noise, (0, 0, 1, 0))[:, :, :H], F.pad(noise, (0, 0, 0, 1))[:, :, 1:]
    else:
        before, after = F.pad(noise, (1, 0))[..., :W], F.pad(noise, (0, 1))[..., 1:]
    return torch.stack((before, noise, after), dim=2).reshape(B, 3 * P, H, W)


def inverse_warp_3d(img, disp):
    """layers/inverse_warp_3d.py:4-52 for a 4-D image: a (size - 1)-normalised grid, sampled with align_corners=False."""
    B, D, H, W = disp.shape
    C = img.shape[1]
    img = img.unsqueeze(2).expand(B, C, D, H, W)
    kw = dict(dtype=disp.dtype, device=disp.device)
    grid_d = torch.arange(D, **kw).view(1, D, 1, 1).expand(B, D, H, W)
    grid_h = torch.arange(H, **kw).view(1, 1, H, 1).expand(B, D, H, W)
    grid_w = torch.arange(W, **kw).view(1, 1, 1, W).expand(B, D, H, W)
    grid_w = grid_w + disp
    grid_d = (grid_d / (D - 1) * 2) - 1
    grid_h = (grid_h / (H - 1) * 2) - 1
    grid_w = (grid_w / (W - 1) * 2) - 1
    grid = torch.stack((grid_w, grid_h, grid_d), dim=4)
    return F.grid_sample(img, grid, mode='bilinear', padding_mode='zeros', align_corners=False)


def evaluate(left, right, samples, noise, temperature):
    """patch_match.py:218-253: samples, noise [B, 3P, H, W] -> [B, P, H, W] each."""
    B, C, H, W = left.shape
    D = samples.shape[1]
    warped = inverse_warp_3d(right, -samples)
    cost = torch.mean(left.unsqueeze(2).expand(B, C, D, H, W) * warped, dim=1) * temperature
    cost = cost.view(B, D // 3, 3, H, W).permute(0, 2, 1, 3, 4)
    samples = samples.view(B, D // 3, 3, H, W).permute(0, 2, 1, 3, 4)
    noise = noise.view(B, D // 3, 3, H, W).permute(0, 2, 1, 3, 4)
    prob = F.softmax(cost, dim=1)
    return torch.sum(prob * samples, dim=1), torch.sum(prob * noise, dim=1)


def intervals(min_disparity, max_disparity, P):
    """patch_match.py:65-81, 323-325: the interval width factor and each interval's lower end, repeated per candidate."""
    B, _, H, W = min_disparity.shape
    index = torch.arange(1, P + 1, 1, dtype=min_disparity.dtype, device=min_disparity.device) / (P + 1)
    index = index.view(1, P, 1, 1).expand(B, P, H, W)
    interval_min = min_disparity + (max_disparity - min_disparity) * index
    interval_min = interval_min.unsqueeze(2).repeat(1, 1, 3, 1, 1).view(B, 3 * P, H, W)
    return 1.0 / (P + 1), interval_min


def half_iteration(left, right, noise, min_disparity, max_disparity, vertical, temperature=TEMPERATURE):
    """One propagate + evaluate step (patch_match.py:333-343 / 347-356): (samples, noise), [B, P, H, W] each."""
    width, interval_min = intervals(min_disparity, max_disparity, noise.shape[1])
    noise = propagate(noise, vertical)
    samples = (max_disparity - min_disparity) * width * noise + interval_min
    return evaluate(left, right, samples, noise, temperature)


def patch_match(left, right, min_disparity, max_disparity, noise, iterations=ITERATIONS, temperature=TEMPERATURE):
    """patch_match.py:305-361 with the initial noise given: [B, P + 2, H, W]."""
    samples = None
    for _ in range(iterations):
        for vertical in (False, True):
            samples, noise = half_iteration(left, right, noise, min_disparity, max_disparity, vertical, temperature)
    return torch.cat((min_disparity, samples, max_disparity), dim=1)


def range_head_post(min_disparity, max_disparity, sample_number, max_disp):
    """DeepPruner.py:48-66."""
    gmin = torch.min(min_disparity, max_disparity)
    gmax = torch.max(min_disparity, max_disparity)
    overflow = torch.clamp((gmin + sample_number - gmax), min=0)
    return (torch.clamp((gmin - overflow) / 2.0, min=0.0, max=max_disp),
            torch.clamp((gmax + overflow) / 2.0, min=0.0, max=max_disp))


def uniform_samples(min_disparity, max_disparity, sample_number):
    """DeepPruner.py:99-115."""
    n = sample_number
    index = torch.arange(1.0, n - 2 + 1, 1, dtype=min_disparity.dtype, device=min_disparity.device)
    index = index.view(n - 2, 1, 1) / (n - 2 + 1)
    inner = min_disparity + (max_disparity - min_disparity) * index
    return torch.cat((min_disparity, inner, max_disparity), dim=1)


def sampler(stage, left, right, min_disparity=None, max_disparity=None, noise=None, max_disp=48, iterations=ITERATIONS,
            temperature=TEMPERATURE, uniform_sample_number=UNIFORM_SAMPLES):
    """DeepPruner.py:176-191."""
    if stage == 'pre':
        B, _, H, W = left.shape
        lo = torch.zeros((B, 1, H, W), dtype=left.dtype, device=left.device)
        hi = torch.zeros((B, 1, H, W), dtype=left.dtype, device=left.device) + max_disp
        return patch_match(left, right, lo, hi, noise, iterations, temperature)
    lo, hi = range_head_post(min_disparity, max_disparity, uniform_sample_number, max_disp)
    return uniform_samples(lo, hi, uniform_sample_number)
