"""The two kernels of csrc/deeppruner_heads.hip on the MI355X.

``deeppruner_volume``: bit for bit the composition it replaces, ``torch.cat((ops.fast_cat_fms(L, R, s), s.unsqueeze(1)[, the two
feature maps on every plane]), 1)`` computed on the device -- the sampler arithmetic is the same warp_taps.h code, the rest copies.

``conv2d_k5_small``: against ``F.conv2d`` on the CPU in FP32 and FP64 under the project's single-layer bound
(docs/design/15-deeppruner-aggregator.md):  max|hip - fp64| <= max(2e-5, 1.25 * max|F.conv2d - fp64|)  with |x| ~ 1 and weights
~ 1 / sqrt(Ci * 25), so outputs are of order one; and batch item 1 of a batch of 2 equals the same item run alone bit for bit (one
ascending fmaf chain per output, independent of the launch).  Measured maxima: docs/design/16-deeppruner-processor.md."""
import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import ops, ops_deeppruner

pytestmark = pytest.mark.gpu

# (B, C, D, H, W, P): the three cases of the processor tests in both stages' forms, the smallest volume the builder takes, widths
# with W % 4 in {1, 2} and more than one block along x (H * W > 256), and a single feature channel
VOLUMES = {"a_pre": (1, 4, 5, 16, 24, 0), "a_post": (1, 4, 3, 16, 24, 5), "b_pre": (2, 6, 14, 8, 40, 0), "b_post": (2, 6, 9, 8, 40, 14),
           "c_pre": (1, 4, 2, 24, 8, 0), "c_post": (1, 4, 2, 24, 8, 2), "minimum": (2, 3, 2, 2, 2, 3), "w13": (2, 5, 3, 5, 13, 4),
           "w70_blocks": (1, 3, 4, 9, 70, 2), "p1": (2, 2, 3, 6, 10, 1)}


@pytest.mark.parametrize("name", list(VOLUMES))
def test_volume_equals_the_composition(dev, name):
    B, C, D, H, W, P = VOLUMES[name]
    g = torch.Generator().manual_seed(700 + list(VOLUMES).index(name))
    left, right = torch.randn((B, C, H, W), generator=g).to(dev), torch.randn((B, C, H, W), generator=g).to(dev)
    # samples from -0.3 W to 1.4 W: some fall left of the image, some right of it
    s = (torch.rand((B, D, H, W), generator=g) * (1.7 * W) - 0.3 * W).to(dev)
    assert (s < 0).any() and (s > W).any()
    fmin, fmax = (torch.randn((B, max(P, 1), H, W), generator=g).to(dev) for _ in range(2))
    base = torch.cat((ops.fast_cat_fms(left, right, s), s.unsqueeze(1)), 1)
    out = ops_deeppruner.deeppruner_volume(left, right, s)
    assert out.shape == (B, 2 * C + 1, D, H, W) and torch.equal(out, base)
    kept = (out[:, C:2 * C] > 0).float().mean().item()
    assert 0.05 < kept < 0.95, kept                          # both branches of T > 0
    if P:
        want = torch.cat((base, fmin.unsqueeze(2).expand(-1, -1, D, -1, -1), fmax.unsqueeze(2).expand(-1, -1, D, -1, -1)), 1)
        out = ops_deeppruner.deeppruner_volume(left, right, s, fmin, fmax)
        assert out.shape == (B, 2 * C + 1 + 2 * P, D, H, W) and torch.equal(out, want)


def test_volume_refusals(dev):
    from densematchingbenchmark_amd._lib import DmbLibraryError
    a, s, f = torch.zeros((1, 3, 4, 6), device=dev), torch.zeros((1, 2, 4, 6), device=dev), torch.zeros((1, 2, 4, 6), device=dev)
    for args in ((a, a, s, f), (a, a, s, None, f), (a, a, s[:, :, :3]), (a, a, s, f, f[:, :1]), (a, a, s, f[..., :5], f[..., :5]),
                 (a, a[:, :2], s), (a, a, s[0]), (a, a, s[:, :1]), (a.double(), a.double(), s)):
        with pytest.raises(DmbLibraryError):
            ops_deeppruner.deeppruner_volume(*args)


CHANNELS = ((1, 1), (9, 9), (14, 14), (16, 16), (5, 3), (3, 16))
SIZES = ((1, 1, 1), (1, 1, 22), (2, 5, 13), (2, 17, 70), (1, 40, 8))      # B, H, W


@pytest.mark.parametrize("Ci,Co", CHANNELS)
def test_conv5x5_against_f_conv2d(dev, Ci, Co):
    g = torch.Generator().manual_seed(900 + 17 * Ci + Co)
    w = torch.randn((Co, Ci, 5, 5), generator=g) / (Ci * 25) ** 0.5
    bias = torch.rand((Co,), generator=g) - 0.5
    scale = torch.rand((Co,), generator=g) + 0.5
    worst = {}
    for B, H, W in SIZES:
        x = torch.randn((B, Ci, H, W), generator=g)
        for tag, sc, sh, relu in (("none", None, None, False), ("bias_relu", None, bias, True), ("affine_relu", scale, bias, True)):
            def stock(x_, w_, dt):
                y = F.conv2d(x_.to(dt), w_.to(dt), None, stride=1, padding=2)
                if sc is not None:
                    y = y * sc.to(dt).view(1, -1, 1, 1)
                if sh is not None:
                    y = y + sh.to(dt).view(1, -1, 1, 1)
                return F.relu(y) if relu else y
            ref32, fp64 = stock(x, w, torch.float32), stock(x, w, torch.float64)
            hip = ops_deeppruner.conv2d_k5_small(x.to(dev), w.to(dev), None if sc is None else sc.to(dev),
                                                 None if sh is None else sh.to(dev), relu)
            assert hip.shape == fp64.shape and torch.isfinite(hip).all()
            e_hip, e_ref = (hip.cpu().double() - fp64).abs().max().item(), (ref32.double() - fp64).abs().max().item()
            worst[tag] = max(worst.get(tag, (0, 0)), (e_hip, e_ref))
            assert e_hip <= max(2e-5, 1.25 * e_ref), ((Ci, Co), (B, H, W), tag, e_hip, e_ref)
    print("conv5x5 %d -> %d: max|hip - fp64| / max|F.conv2d - fp64| per epilogue: %s"
          % (Ci, Co, {k: "%.3g / %.3g" % v for k, v in worst.items()}))


@pytest.mark.parametrize("Ci,Co", CHANNELS)
def test_conv5x5_batch_item_equals_the_item_alone(dev, Ci, Co):
    g = torch.Generator().manual_seed(1100 + 17 * Ci + Co)
    w = (torch.randn((Co, Ci, 5, 5), generator=g) / (Ci * 25) ** 0.5).to(dev)
    scale, shift = (torch.rand((Co,), generator=g) + 0.5).to(dev), (torch.rand((Co,), generator=g) - 0.5).to(dev)
    for H, W in ((5, 13), (17, 70)):
        x = torch.randn((2, Ci, H, W), generator=g).to(dev)
        both = ops_deeppruner.conv2d_k5_small(x, w, scale, shift, True)
        for i in (0, 1):
            assert torch.equal(both[i:i + 1], ops_deeppruner.conv2d_k5_small(x[i:i + 1].contiguous(), w, scale, shift, True)), (H, W, i)


def test_conv5x5_refusals(dev):
    from densematchingbenchmark_amd._lib import DmbLibraryError
    x, w = torch.zeros((1, 3, 4, 6), device=dev), torch.zeros((2, 3, 5, 5), device=dev)
    for args in ((x, w[:, :2]), (x, w[..., :3, :3]), (x, w, torch.zeros(3, device=dev)), (x, w, None, torch.zeros(3, device=dev)),
                 (x[0], w), (x.double(), w.double()), (torch.zeros((1, 17, 4, 4), device=dev), torch.zeros((2, 17, 5, 5), device=dev)),
                 (x, torch.zeros((17, 3, 5, 5), device=dev)), (x.cpu(), w.cpu())):
        with pytest.raises(DmbLibraryError):
            ops_deeppruner.conv2d_k5_small(*args)
