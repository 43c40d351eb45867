"""DeepPruner's disparity sampler on the MI355X (csrc/patch_match.hip) against the real reference's recording
(tests/golden/deeppruner_sampler.npz) and the functional restatement (tests/_deeppruner_ref.py) in FP64, with the FP32
reference / restatement's own distance from FP64 as the scale.

The contract of the "pre" stage (``_check_fp32_work``): with e_ref = max|reference - fp64| and e_hip = max|hip - fp64|,
e_hip <= max(1e-4, 1.25 * e_ref) and mean|hip - fp64| <= 1.25 * mean|reference - fp64|.  The "post" stage is bit-exact.

Measured on an MI355X, stage "pre", 3 iterations, recorded noise (fixture cases a / b / c):
    e_hip 1.601e-05 / 9.973e-06 / 4.811e-06    e_ref 1.601e-05 / 9.973e-06 / 3.993e-06
    mean  1.473e-06 / 1.420e-06 / 6.971e-07    reference's mean 1.476e-06 / 1.419e-06 / 6.970e-07
At the configs' feature sizes against the restatement on the device (1x136x240 / 4x136x240 / 1x68x120):
    e_hip 9.10e-05 / 1.47e-04 / 1.57e-05       e_ref 1.00e-04 / 1.79e-04 / 3.38e-05
    mean  1.804e-06 / 1.801e-06 / 7.06e-07     restatement's mean 2.043e-06 / 2.047e-06 / 7.97e-07
"""
import os

import numpy as np
import pytest
import torch

from densematchingbenchmark_amd import ops
from densematchingbenchmark_amd.modeling.stereo.cost_processors.utils.cat_fms import fast_cat_fms
from densematchingbenchmark_amd.modeling.stereo.disp_samplers import DeepPrunerSampler, PatchMatch, UniformSampler
from tests import _deeppruner_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "deeppruner_sampler.npz")


def _check_fp32_work(hip, ref32, ref64, what):
    hip, ref32, ref64 = hip.double().cpu(), ref32.double().cpu(), ref64.double().cpu()
    d_hip, d_ref = (hip - ref64).abs(), (ref32 - ref64).abs()
    e_hip, e_ref, m_hip, m_ref = d_hip.max().item(), d_ref.max().item(), d_hip.mean().item(), d_ref.mean().item()
    print("%s: e_hip %.4g e_ref %.4g mean_hip %.4g mean_ref %.4g" % (what, e_hip, e_ref, m_hip, m_ref))
    assert torch.isfinite(hip).all(), what
    assert e_hip <= max(1e-4, 1.25 * e_ref), (what, e_hip, e_ref)
    assert m_hip <= 1.25 * m_ref, (what, m_hip, m_ref)


def _sampler(max_disp, **kw):
    return DeepPrunerSampler(max_disp=max_disp, **kw).eval()


def _random_case(B, C, H, W, P, seed, dev, wide_range=True):
    g = torch.Generator().manual_seed(seed)
    left, right = torch.randn((B, C, H, W), generator=g), torch.randn((B, C, H, W), generator=g)
    noise = torch.rand((B, P, H, W), generator=g)
    # non-constant range maps; the upper end beyond the image width, so that x - s leaves the image on the left, and a lower
    # end below 0, so that it leaves it on the right
    lo = torch.rand((B, 1, H, W), generator=g) * (0.3 * W) - 2.0
    hi = lo + (2.0 + W * (1.0 + 0.5 * torch.rand((B, 1, H, W), generator=g)) if wide_range
               else 0.5 + 0.5 * W * torch.rand((B, 1, H, W), generator=g))
    return left, right, noise, lo, hi


# --------------------------------------------------------------------------------------------------------------- post stage
def test_post_stage_bit_exact_against_recording(dev):
    z = np.load(GOLDEN)
    for name, (shape, max_disp, _, _) in R.GOLDEN_CASES.items():
        left, right, _, lo, hi = R.golden_inputs(name)
        got = _sampler(max_disp)('post', left.to(dev), right.to(dev), lo.to(dev), hi.to(dev))
        assert torch.equal(got.cpu(), torch.from_numpy(z[name + "/post"])), name


@pytest.mark.parametrize("N", [3, 9, 10, 2])
def test_post_stage_bit_exact_against_restatement(dev, N):
    max_disp = 24
    g = torch.Generator().manual_seed(77 + N)
    lo = torch.rand((2, 1, 19, 37), generator=g) * 60.0 - 20.0          # below 0 and above max_disp
    hi = lo + (torch.rand((2, 1, 19, 37), generator=g) * 40.0 - 12.0)   # min > max on a third, narrower than N on another part
    lo[0, 0, 0, :4] = torch.tensor([0.0, -0.0, 24.0, 7.5])
    hi[0, 0, 0, :4] = torch.tensor([0.0, 30.0, 24.0, 7.5])
    assert (lo > hi).any() and ((hi - lo).abs() < N).any() and ((hi - lo) > N).any()
    want = R.sampler('post', None, None, lo, hi, max_disp=max_disp, uniform_sample_number=N)
    assert (want == 0).any() and (want == max_disp).any()               # both clamps are reached
    feat = torch.zeros((2, 4, 19, 37), device=dev)
    got = _sampler(max_disp, uniform_disparity_sample_number=N)('post', feat, feat, lo.to(dev), hi.to(dev))
    assert got.shape == (2, N, 19, 37) and got.is_contiguous()
    assert torch.equal(got.cpu(), want)
    # the uniform sampler alone (no range head)
    lo2, hi2 = R.range_head_post(lo, hi, N, max_disp)
    assert torch.equal(UniformSampler(N)(lo2.to(dev), hi2.to(dev)).cpu(), R.uniform_samples(lo2, hi2, N))


# ---------------------------------------------------------------------------------------------------------------- pre stage
def test_pre_stage_against_reference_recording(dev):
    z = np.load(GOLDEN)
    for name, (shape, max_disp, _, _) in R.GOLDEN_CASES.items():
        left, right, noise, _, _ = R.golden_inputs(name)
        with torch.no_grad():
            f64 = R.sampler('pre', left.double(), right.double(), noise=noise.double(), max_disp=max_disp)
            got = _sampler(max_disp)('pre', left.to(dev), right.to(dev), noise=noise.to(dev))
        _check_fp32_work(got, torch.from_numpy(z[name + "/pre"]), f64, "pre stage, recording " + name)


STEP_CASES = [
    # B, C, H, W, P
    (2, 32, 17, 41, 12),
    (1, 8, 17, 41, 5),
    (1, 64, 17, 41, 1),
    (1, 8, 2, 2, 1),
    (2, 32, 2, 2, 12),
    (1, 64, 9, 2, 5),
    (1, 32, 9, 2, 1),
    (1, 8, 2, 300, 12),     # one wide row (and its neighbour)
    (1, 64, 2, 300, 5),
    (1, 33, 6, 7, 3),       # a channel count that is no multiple of 4
]


@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("case", STEP_CASES)
def test_one_half_iteration(dev, case, vertical):
    B, C, H, W, P = case
    left, right, noise, lo, hi = _random_case(B, C, H, W, P, 1000 + 7 * C + H + P, dev)
    with torch.no_grad():
        s32, n32 = R.half_iteration(left, right, noise, lo, hi, vertical, 7)
        s64, n64 = R.half_iteration(*(t.double() for t in (left, right, noise, lo, hi)), vertical, 7)
    # the candidates do leave the image, on both sides
    assert (hi.max() > W - 1) and (lo.min() < 0)
    gs, gn = ops.patch_match_step(left.to(dev), right.to(dev), noise.to(dev), lo.to(dev), hi.to(dev), vertical=vertical,
                                  temperature=7)
    what = "half-iteration %s %s" % (case, "vertical" if vertical else "horizontal")
    _check_fp32_work(gs, s32, s64, what + " samples")
    _check_fp32_work(gn, n32, n64, what + " noise")
    # the same step writing into the result's channels, ends in place, no new noise
    out = torch.full((B, P + 2, H, W), float("nan"), device=dev)
    res, none = ops.patch_match_step(left.to(dev), right.to(dev), noise.to(dev), lo.to(dev), hi.to(dev), vertical=vertical,
                                     temperature=7, want_noise=False, out=out)
    assert none is None and res is out
    assert torch.equal(out[:, 1:-1], gs) and torch.equal(out[:, :1].cpu(), lo) and torch.equal(out[:, -1:].cpu(), hi)


def test_result_structure(dev):
    for name, (shape, max_disp, _, _) in R.GOLDEN_CASES.items():
        left, right, noise, _, _ = R.golden_inputs(name)
        out = _sampler(max_disp)('pre', left.to(dev), right.to(dev), noise=noise.to(dev)).cpu()
        P = out.shape[1] - 2
        assert out.shape == (shape[0], 14) + shape[2:] and out.is_contiguous()
        assert (out[:, 0] == 0).all() and (out[:, -1] == max_disp).all()
        for p in range(P):
            assert (out[:, 1 + p] >= max_disp * (p + 1) / (P + 1) - 1e-4).all(), (name, p)
            assert (out[:, 1 + p] <= max_disp * (p + 2) / (P + 1) + 1e-4).all(), (name, p)
        assert (out[:, 1:] >= out[:, :-1]).all(), name
    # range maps instead of the constant range: the ends are the maps, exactly
    left, right, noise, lo, hi = _random_case(2, 32, 17, 41, 5, 31, dev, wide_range=False)
    pm = PatchMatch(disparity_sample_number=7, iterations=2, temperature=7)
    out = pm(left.to(dev), right.to(dev), lo.to(dev), hi.to(dev), noise=noise.to(dev)).cpu()
    assert torch.equal(out[:, :1], lo) and torch.equal(out[:, -1:], hi)
    for p in range(5):
        low, high = lo + (hi - lo) * ((p + 1) / 6), lo + (hi - lo) * ((p + 2) / 6)
        assert (out[:, 1 + p:2 + p] >= low - 1e-4).all() and (out[:, 1 + p:2 + p] <= high + 1e-4).all()
    with torch.no_grad():
        want = R.patch_match(*(t.double() for t in (left, right, lo, hi, noise)), iterations=2, temperature=7)
        w32 = R.patch_match(left, right, lo, hi, noise, iterations=2, temperature=7)
    _check_fp32_work(out, w32, want, "PatchMatch on range maps")


def test_invariance_and_graph_replay(dev):
    g = torch.Generator().manual_seed(5)
    left, right = torch.randn((4, 32, 24, 56), generator=g).to(dev), torch.randn((4, 32, 24, 56), generator=g).to(dev)
    noise = torch.rand((4, 12, 24, 56), generator=g).to(dev)
    s = _sampler(48)
    keep = noise.clone()
    full = s('pre', left, right, noise=noise)
    assert torch.equal(noise, keep)                                   # the caller's noise is read, never written
    assert torch.equal(s('pre', left, right, noise=noise), full)      # two runs
    for i in range(4):
        alone = s('pre', left[i:i + 1].contiguous(), right[i:i + 1].contiguous(), noise=noise[i:i + 1].contiguous())
        assert torch.equal(alone, full[i:i + 1]), i
    # capture the eager call; replay it on the same and on new noise
    static = noise.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        s('pre', left, right, noise=static)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph), torch.no_grad():
        out = s('pre', left, right, noise=static)
        post = s('post', left, right, out[:, 3:4], out[:, 9:10])
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, full)
    assert torch.equal(post, s('post', left, right, full[:, 3:4], full[:, 9:10]))
    noise2 = torch.rand((4, 12, 24, 56), generator=g).to(dev)
    static.copy_(noise2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, s('pre', left, right, noise=noise2)) and not torch.equal(out, full)


def test_noise_contract(dev):
    left, right, noise, lo, hi = (t.to(dev) for t in R.golden_inputs("c"))
    s = _sampler(24)
    torch.manual_seed(11)
    a = s('pre', left, right)
    torch.manual_seed(11)
    b = s('pre', left, right)
    torch.manual_seed(12)
    c = s('pre', left, right)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert a.shape == (1, 14, 17, 41) and torch.isfinite(a).all()
    for bad in (noise[:, :5], noise.double(), noise[..., :-1].contiguous(), noise.cpu(), [1.0]):
        with pytest.raises(ValueError, match="noise"):
            s('pre', left, right, noise=bad)
    with pytest.raises(NotImplementedError, match="backward"):
        s('pre', left.clone().requires_grad_(), right, noise=noise)
    with pytest.raises(NotImplementedError, match="backward"):
        s('pre', left, right, noise=noise.clone().requires_grad_())
    with pytest.raises(NotImplementedError, match="backward"):
        s('post', left, right, lo, hi.clone().requires_grad_())
    with torch.no_grad():                                             # grad mode off: nothing to refuse
        assert torch.equal(s('pre', left.clone().requires_grad_(), right, noise=noise), s('pre', left, right, noise=noise))


def test_unsupported_shapes_are_refused(dev):
    from densematchingbenchmark_amd import _lib
    one_row = torch.zeros((1, 8, 1, 16), device=dev)
    with pytest.raises(NotImplementedError):
        _sampler(24)('pre', one_row, one_row)
    with pytest.raises(_lib.DmbLibraryError, match="100002"):
        ops.patch_match_step(one_row, one_row, torch.zeros((1, 3, 1, 16), device=dev), bounds=(0.0, 24.0))
    feat = torch.zeros((1, 8, 4, 4), device=dev)
    with pytest.raises(_lib.DmbLibraryError, match="100002"):
        ops.patch_match_step(feat, feat, torch.zeros((1, ops.PATCH_MATCH_MAX_SAMPLES + 1, 4, 4), device=dev), bounds=(0.0, 24.0))
    # the documented upper bound itself works
    out, _ = ops.patch_match_step(feat, feat, torch.rand((1, ops.PATCH_MATCH_MAX_SAMPLES, 4, 4), device=dev), bounds=(0.0, 24.0))
    assert torch.isfinite(out).all()


# --------------------------------------------------------------------------------------------------- the configs' feature sizes
@pytest.mark.parametrize("B,H,W,max_disp", [(1, 136, 240, 48), (4, 136, 240, 48), (1, 68, 120, 24)])
def test_config_feature_sizes_against_restatement(dev, B, H, W, max_disp):
    g = torch.Generator().manual_seed(900 + B + H)
    left, right = torch.randn((B, 32, H, W), generator=g).to(dev), torch.randn((B, 32, H, W), generator=g).to(dev)
    noise = torch.rand((B, 12, H, W), generator=g).to(dev)
    got = _sampler(max_disp)('pre', left, right, noise=noise)
    with torch.no_grad():     # stock torch on the device, one pair at a time (the FP64 volumes are 0.3 GB each per pair)
        r32 = torch.cat([R.sampler('pre', left[i:i + 1], right[i:i + 1], noise=noise[i:i + 1], max_disp=max_disp)
                         for i in range(B)])
        r64 = torch.cat([R.sampler('pre', left[i:i + 1].double(), right[i:i + 1].double(), noise=noise[i:i + 1].double(),
                                   max_disp=max_disp) for i in range(B)])
    _check_fp32_work(got, r32, r64, "pre stage %dx%dx%d max_disp %d" % (B, H, W, max_disp))


def test_no_expanded_volume(dev):
    g = torch.Generator().manual_seed(3)
    left, right = torch.randn((1, 32, 136, 240), generator=g).to(dev), torch.randn((1, 32, 136, 240), generator=g).to(dev)
    s = _sampler(48)
    s('pre', left, right)                      # first use: anything the runtime allocates once
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = s('pre', left, right)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    result_bytes = out.numel() * 4
    print("peak rise %d bytes = %.2f x the result" % (rise, rise / result_bytes))
    assert rise <= 8 * result_bytes, (rise, result_bytes)


def test_hand_over_to_the_volume_builder(dev):
    """``fast_cat_fms`` takes the sampler's tensor as it is.  The target half of the volume is piecewise linear in the sample
    with slope at most 2 * max|R| * W / (W - 1) per unit of disparity, so samples within 1e-4 (the sampler's contract) move it by
    at most that slope times 1e-4; the FP32 builder's own distance from the FP64 warp is the other scale."""
    name = "a"
    shape, max_disp, _, _ = R.GOLDEN_CASES[name]
    left, right, noise, _, _ = R.golden_inputs(name)
    W = shape[3]
    samples = _sampler(max_disp)('pre', left.to(dev), right.to(dev), noise=noise.to(dev))
    assert samples.is_contiguous() and samples.shape == (shape[0], 14) + shape[2:]
    vol = fast_cat_fms(left.to(dev), right.to(dev), disp_sample=samples)
    assert vol.shape == (shape[0], 64, 14) + shape[2:]
    with torch.no_grad():
        s32 = R.sampler('pre', left, right, noise=noise, max_disp=max_disp)
        s64 = R.sampler('pre', left.double(), right.double(), noise=noise.double(), max_disp=max_disp)
        t64 = R.inverse_warp_3d(right.double(), -s64)
    vol_ref = fast_cat_fms(left.to(dev), right.to(dev), disp_sample=s32.to(dev))
    e_hip = (vol[:, 32:].double().cpu() - t64).abs().max().item()
    e_ref = (vol_ref[:, 32:].double().cpu() - t64).abs().max().item()
    slope = 2.0 * right.abs().max().item() * W / (W - 1)
    print("hand-over: e_hip %.4g e_ref %.4g slope bound %.4g" % (e_hip, e_ref, slope * 1e-4))
    assert e_hip <= max(1.25 * e_ref, slope * 1e-4)
    # the reference half is the left feature masked where the warped target is positive: the same wherever the target is not
    # within that distance of 0
    clear = (t64.abs() > max(1.25 * e_ref, slope * 1e-4)).to(dev)
    assert torch.equal(vol[:, :32][clear], vol_ref[:, :32][clear])
