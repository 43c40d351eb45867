"""``ops_deeppruner.deeppruner_final_maps`` (csrc/deeppruner_final_maps.hip) on the MI355X.

Bit for bit (``torch.equal``) against the composition it replaces -- ``ops.bilinear_scale((d * W) / w, (H, W), 1.0)`` per map, the
two rescalings and torch's ``sub`` / ``abs`` on the device (``_deeppruner_model_ref.final_maps_unfused``; its divisions are by a
device tensor, because ATen divides by a Python number on the GPU as a multiplication by the reciprocal) -- for K = 1, 2, 3 list
maps at five output sizes and one case whose ratios are no powers of two; item 1 of a batch of 2 against the item alone; and
against torch's CPU ``F.interpolate`` of the same operands (``_deeppruner_model_ref.final_maps``) to 1e-6 of the maps' magnitude,
the bound docs/design/13-anynet.md gives the same arithmetic.

Sizes.  Output (H, W) with the list at (H >> k, W >> k), k < K, and the range maps at (H >> K, W >> K), as the model has them
(never below one pixel): (4, 4) ends in 1 x 1 maps; (16, 40) has odd W / 4 = 10 / 2 and W / 8 = 5; (24, 72) and (40, 264) span
several 64 x 4 tiles with a partial last column of tiles; B = 2 at two of them."""
import pytest
import torch

from densematchingbenchmark_amd import ops, ops_deeppruner
from tests import _deeppruner_model_ref as R

pytestmark = pytest.mark.gpu
SHAPES = [(1, 4, 4), (2, 8, 24), (1, 16, 40), (2, 24, 72), (1, 40, 264)]


def _operands(B, sizes, range_size, seed):
    """Disparities in [0, 50): the list's maps, then min below max on most pixels."""
    g = torch.Generator().manual_seed(seed)
    disps = [torch.rand((B, 1) + hw, generator=g) * 50.0 for hw in sizes]
    lo = torch.rand((B, 1) + range_size, generator=g) * 30.0
    hi = lo + torch.rand((B, 1) + range_size, generator=g) * 25.0 - 2.0
    return disps, lo, hi


def _model_sizes(K, H, W):
    return [(max(1, H >> k), max(1, W >> k)) for k in range(K)], (max(1, H >> K), max(1, W >> K))


def _check(dev, disps, lo, hi, size):
    K, B = len(disps), disps[0].shape[0]
    d_dev, lo_dev, hi_dev = [t.to(dev) for t in disps], lo.to(dev), hi.to(dev)
    kept = [t.clone() for t in d_dev + [lo_dev, hi_dev]]
    got = ops_deeppruner.deeppruner_final_maps(d_dev, lo_dev, hi_dev, size)
    want = R.final_maps_unfused(ops, d_dev, lo_dev, hi_dev, size)
    assert len(got) == len(want) == K + 4
    assert all(torch.equal(a, b) for a, b in zip(kept, d_dev + [lo_dev, hi_dev]))          # operands untouched
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == (B, 1) + tuple(size) and a.is_contiguous() and torch.equal(a, b), (K, size, i)
    assert got[1].data_ptr() - got[0].data_ptr() == 4 * B * size[0] * size[1]                # views of one [K + 4, B, 1, H, W] tensor
    # against ATen's CPU interpolation of the same operands.  A map's error is a few roundings of its own magnitude; a residual
    # |D - Mn| carries the errors of D and of Mn, so its scale is theirs, not its own
    cpu = R.final_maps(disps, lo, hi, size)
    mags = [m.abs().max().item() for m in cpu]
    scales = mags[:K + 2] + [max(mags[K - 1], mags[K])] + [max(mags[K - 1], mags[K + 1])]
    for i, (a, b, s) in enumerate(zip(got, cpu, scales)):
        err = (a.cpu() - b).abs().max().item()
        assert err <= 1e-6 * s, (K, size, i, err, s)
    return got


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_equals_the_composition_bit_for_bit(dev, B, H, W, K):
    sizes, range_size = _model_sizes(K, H, W)
    disps, lo, hi = _operands(B, sizes, range_size, 100 * K + H)
    got = _check(dev, disps, lo, hi, (H, W))
    if B == 2:          # item 1 of the batch against the item alone
        one = ops_deeppruner.deeppruner_final_maps([d[1:].to(dev) for d in disps], lo[1:].to(dev), hi[1:].to(dev), (H, W))
        for a, b in zip(got, one):
            assert torch.equal(a[1:], b)


def test_ratios_that_are_no_powers_of_two(dev):
    disps, lo, hi = _operands(2, [(5, 9), (3, 5)], (3, 5), 7)
    _check(dev, disps, lo, hi, (12, 20))
    _check(dev, disps[::-1], hi, lo, (12, 20))                    # the coarser map first, the range the other way round
    _check(dev, disps[:1], lo, hi, (5, 9))                        # a map already at the output size: (d * W) / W, not d


def test_the_second_scaling_of_the_range_maps_shows(dev):
    """(Mn * W) / W is not Mn: the kernel must round twice more, as the reference does when it interpolates the full-size maps a
    second time."""
    disps, lo, hi = _operands(1, [(40, 264), (20, 132)], (10, 66), 11)
    got = ops_deeppruner.deeppruner_final_maps([t.to(dev) for t in disps], lo.to(dev), hi.to(dev), (40, 264))
    w, W = torch.full((), 66.0, device=dev), torch.full((), 264.0, device=dev)     # tensor divisors: IEEE division on the device
    Mn = ops.bilinear_scale((lo.to(dev) * 264) / w, (40, 264), 1.0)
    assert not torch.equal(got[2], Mn) and torch.equal(got[2], (Mn * 264) / W)
    assert torch.equal(got[4], torch.abs(got[1] - Mn))           # ... and the residuals take the un-rescaled map
