"""``ops_deeppruner.refine_head_up2`` (csrc/refine_head.hip) on the MI355X: the tail of a DeepPruner refinement stage,
y = up2(2 * relu(conv3x3(x, w) + init)), in one launch.

Shapes: one pixel; one row with 16 channels; B = 2 below one tile with odd sizes; several 32 x 8 tiles with partial ones on both
edges; taller than wide; one row and one column past a tile edge (the ring of a one-pixel tile).

Checks.  (a) With an all-zero weight the output is bit for bit ``ops.bilinear_scale(relu(init), (2H, 2W), 2.0)``: the
interpolation half is the shared code of csrc/bilinear_hp.h.  (b) With weights ~ N(0, 1 / (9 Ci)) and x ~ N(0, 1) the project's
single-layer bound (docs/design/15 and 16): max|hip - fp64| <= max(2e-5 * max(1, max|fp64|), 1.25 * max|torch_cpu_fp32 - fp64|),
the CPU FP32 composition F.conv2d -> + init -> relu -> * 2 -> F.interpolate being the yardstick.  (c) Item 1 of a batch of 2
equals the item run alone bit for bit.  ``init`` ~ N(0, 1) next to a convolution of unit variance: the FP64 result must show
between 5 % and 95 % of the refined values clamped, so the yardstick alone decides that both branches of the ReLU are taken.
The one exception is (1, 1, 1, 1): a single refined value takes one branch, so a share between 5 % and 95 % cannot exist there;
the assertion is made at every shape with at least 20 refined values, which is every other one, and the single pixel's branch
(it is not clamped: its FP64 refined value is positive) is asserted by name."""
import pytest
import torch
import torch.nn.functional as F

from densematchingbenchmark_amd import _lib, ops, ops_deeppruner
from tests._deeppruner_features_ref import refine_tail

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1), (1, 16, 1, 22), (2, 5, 5, 13), (2, 16, 17, 70), (1, 9, 40, 8), (1, 16, 33, 65)]
_cache = {}


def _case(shape):
    """x, w, init on the CPU, the FP64 refined map and output, the CPU FP32 output: computed once, shared, never modified."""
    if shape not in _cache:
        B, Ci, H, W = shape
        g = torch.Generator().manual_seed(1000 + 131 * B + 17 * Ci + 7 * H + W)
        x, w = torch.randn((B, Ci, H, W), generator=g), torch.randn((1, Ci, 3, 3), generator=g) * (1.0 / (9 * Ci)) ** 0.5
        init = torch.randn((B, 1, H, W), generator=g)
        refined64 = F.relu(F.conv2d(x.double(), w.double(), padding=1) + init.double())
        _cache[shape] = (x, w, init, refined64, refine_tail(x.double(), w.double(), init.double()), refine_tail(x, w, init))
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_zero_weight_is_the_shared_interpolation_bit_for_bit(dev, shape):
    B, Ci, H, W = shape
    x, _, init = (t.to(dev) for t in _case(shape)[:3])
    got = ops_deeppruner.refine_head_up2(x, torch.zeros((1, Ci, 3, 3), device=dev), init)
    want = ops.bilinear_scale(torch.relu(init), (2 * H, 2 * W), 2.0)
    assert got.shape == (B, 1, 2 * H, 2 * W) and torch.equal(got, want)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_against_fp64_with_the_cpu_composition_as_yardstick(dev, shape):
    x, w, init, refined64, fp64, cpu32 = _case(shape)
    if refined64.numel() >= 20:
        clamped = (refined64 == 0).double().mean().item()
        assert 0.05 <= clamped <= 0.95, (shape, clamped)
    else:                            # the single pixel: one value, one branch -- the positive one
        assert shape == (1, 1, 1, 1) and refined64.item() > 0
    got = ops_deeppruner.refine_head_up2(x.to(dev), w.to(dev), init.to(dev)).cpu().double()
    assert got.shape == fp64.shape and torch.isfinite(got).all()
    e_hip, e_ref, scale = (got - fp64).abs().max().item(), (cpu32.double() - fp64).abs().max().item(), max(1.0, fp64.abs().max().item())
    print("%s: max|fp64| %.4g  e_hip %.4g  e_ref %.4g  floor %.4g" % (shape, scale, e_hip, e_ref, 2e-5 * scale))
    assert e_hip <= max(2e-5 * scale, 1.25 * e_ref), (shape, e_hip, e_ref)


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] == 2], ids=lambda s: "x".join(str(v) for v in s))
def test_batch_item_equals_the_item_alone_bit_for_bit(dev, shape):
    x, w, init = (t.to(dev) for t in _case(shape)[:3])
    both = ops_deeppruner.refine_head_up2(x, w, init)
    alone = ops_deeppruner.refine_head_up2(x[1:].contiguous(), w, init[1:].contiguous())
    assert torch.equal(both[1:], alone)


def test_wrapper_refusals(dev):
    x, w, init = torch.zeros((2, 5, 4, 6), device=dev), torch.zeros((1, 5, 3, 3), device=dev), torch.zeros((2, 1, 4, 6), device=dev)
    for args in ((x[0], w, init),                                                                # wrong rank
                 (torch.zeros((2, 17, 4, 6), device=dev), torch.zeros((1, 17, 3, 3), device=dev), init),   # Ci = 17
                 (x.double(), w, init), (x, w, init.double()),                                   # double precision
                 (x, w, torch.zeros((2, 1, 4, 5), device=dev)), (x, w, torch.zeros((1, 1, 4, 6), device=dev))):   # mismatched init
        with pytest.raises(_lib.DmbLibraryError):
            ops_deeppruner.refine_head_up2(*args)
